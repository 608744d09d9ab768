"""Code-generation guard for the fused max-pool + squeeze kernels (csrc/cnn_poolsq.hip; no GPU needed: hipcc cross-compiles): the
row-tile kernel k_pool_squeeze<NBLK, NWV> of the large forwards and the segment kernel k_pool_squeeze_seg<PT, NB> of the small ones.
The row-tile kernel holds a tap row of twelve float4, the running maximum, the loader's state for four pixels and one or two
accumulators in registers and promises three waves per SIMD; a spill or a register over the bound would quietly cost the occupancy it
is built on.

For every instantiation the launcher can reach (one or two 32-channel column blocks, 12, 6 or 3 waves per workgroup), from the
kernel's metadata alone: it exists, ScratchSize is 0, its registers fit the waves per SIMD that its __launch_bounds__ promise (gfx950:
512 registers per SIMD lane, allocated in eights), and its static LDS plus the dynamic LDS the launcher may request (it raises the
limit to 160 KB - 256 and is not chosen for what does not fit) stays within 160 KB - 256.  The segment kernel (one to three pixel
tiles times one or two column blocks = one to six waves per workgroup, static LDS only) is held to the same four conditions."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

LDS_BOUND = 160 * 1024 - 256
DYNAMIC_LDS_LIMIT = 160 * 1024 - 256          # launch_pool_squeeze_w: ensure_dyn_lds(..., 160 * 1024 - 256, ...)
WAVES_PER_SIMD = 3                             # __launch_bounds__(64 * NWV, 3)
INSTANTIATIONS = [(nblk, nwv) for nblk in (1, 2) for nwv in (12, 6, 3)]
SEG_INSTANTIATIONS = [(pt, nb) for pt in (1, 2, 3) for nb in (1, 2)]          # __launch_bounds__(64 * PT * NB): one or two waves per SIMD


def _register_bound(waves_per_workgroup, promised=WAVES_PER_SIMD):
    waves = max(promised, -(-waves_per_workgroup // 4))          # a workgroup's waves are spread over the CU's four SIMDs
    return 512 // waves // 8 * 8


def _dynamic_lds(cin, nblk, nwv):
    """What launch_pool_squeeze_w requests (pool_squeeze_lds): the weights [cin][32 nblk + 1], rounded up to four floats, the padded
    bias, and a pooled chunk of 32 channels x 32 pixels at pitch 34 per wave."""
    return 4 * (((cin * (32 * nblk + 1) + 3) & ~3) + 32 * nblk + nwv * 32 * 34)


def _waves(cin, nblk, row_tiles):
    """pool_squeeze_by_row_tiles: twelve waves, halved while the LDS does not hold them; None = the segment kernel (fewer row tiles than
    two rounds of the resident waves, or no room for three waves)."""
    nwv = 12
    while nwv > 3 and _dynamic_lds(cin, nblk, nwv) > DYNAMIC_LDS_LIMIT:
        nwv //= 2
    return nwv if _dynamic_lds(cin, nblk, nwv) <= DYNAMIC_LDS_LIMIT and row_tiles >= 2 * 256 * nwv else None


@pytest.fixture(scope="module")
def poolsq_asm(tmp_path_factory):
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("hipcc not available")
    from swiftwatcher_amd.csrc import build
    out = tmp_path_factory.mktemp("asm") / "cnn_poolsq.s"
    src = os.path.join(ROOT, "swiftwatcher_amd", "csrc", "cnn_poolsq.hip")
    flags = [f for f in build.FLAGS if f not in ("-Wall",)]          # the library's own flags
    subprocess.check_call([HIPCC] + flags + ["--cuda-device-only", "-S", src, "-o", str(out)])
    return open(out).read()


def _metadata(asm, nblk, nwv, name="14k_pool_squeeze"):
    """The kernel's entry in the code object's metadata (.amdgpu_metadata) and the summary the compiler prints behind its body."""
    prefix = "_ZN3swk%sILi%dELi%dEEE" % (name, nblk, nwv)
    entries = [e for e in re.split(r"\n  - (?=\.agpr_count:)", asm[asm.index(".amdgpu_metadata"):]) if re.search(r"\.name:\s+" + prefix, e)]
    assert len(entries) == 1, "no instantiation %s<%d, %d>" % (name[2:], nblk, nwv)
    summary = re.search(r"\.section\s+\.AMDGPU\.csdata.*?; Kernel info:(.*?); COMPUTE_PGM_RSRC2:USER_SGPR", asm[asm.index("\n" + prefix):], re.S)
    assert summary is not None
    return entries[0], summary.group(1)


def _field(entry, name):
    return int(re.search(r"\.%s:\s+(\d+)" % name, entry).group(1))


@pytest.mark.parametrize("nblk,nwv", INSTANTIATIONS)
def test_every_reachable_instantiation_keeps_its_registers_and_lds(poolsq_asm, nblk, nwv):
    entry, summary = _metadata(poolsq_asm, nblk, nwv)
    assert int(re.search(r"ScratchSize: (\d+)", summary).group(1)) == 0, "k_pool_squeeze<%d, %d> spills" % (nblk, nwv)
    assert _field(entry, "private_segment_fixed_size") == 0
    assert _field(entry, "max_flat_workgroup_size") == 64 * nwv
    registers = max(_field(entry, "vgpr_count"), (_field(entry, "vgpr_count") - _field(entry, "agpr_count") + 3) // 4 * 4 + _field(entry, "agpr_count"))
    assert registers <= _register_bound(nwv), "%d registers: fewer than %d waves per SIMD" % (registers, WAVES_PER_SIMD)
    static = _field(entry, "group_segment_fixed_size")
    assert static + DYNAMIC_LDS_LIMIT <= LDS_BOUND, "%d bytes of static LDS beside the dynamic weights" % static


@pytest.mark.parametrize("pt,nb", SEG_INSTANTIATIONS)
def test_every_segment_kernel_instantiation_keeps_its_registers_and_lds(poolsq_asm, pt, nb):
    entry, summary = _metadata(poolsq_asm, pt, nb, "18k_pool_squeeze_seg")
    assert int(re.search(r"ScratchSize: (\d+)", summary).group(1)) == 0, "k_pool_squeeze_seg<%d, %d> spills" % (pt, nb)
    assert _field(entry, "private_segment_fixed_size") == 0
    assert _field(entry, "max_flat_workgroup_size") == 64 * pt * nb
    registers = max(_field(entry, "vgpr_count"), (_field(entry, "vgpr_count") - _field(entry, "agpr_count") + 3) // 4 * 4 + _field(entry, "agpr_count"))
    assert registers <= _register_bound(pt * nb, promised=1)
    assert _field(entry, "group_segment_fixed_size") == 4 * 2 * 32 * (32 * pt + 1 + 32 * nb + 1) <= LDS_BOUND          # launched without dynamic LDS


def test_the_networks_weights_fit_the_lds():
    assert _register_bound(12) == _register_bound(6) == _register_bound(3) == 168
    chosen = {}
    for cin, cout, pooled in ((96, 16, 8), (256, 32, 8), (512, 64, 9)):          # the three pool -> squeeze pairs of SqueezeNet-1.0
        for segments in (1, 300, 2048, 4096, 8192):
            nwv = _waves(cin, (cout + 31) // 32, (segments * pooled * pooled + 31) // 32)
            assert nwv is None or _dynamic_lds(cin, (cout + 31) // 32, nwv) <= LDS_BOUND
            chosen[cin, segments] = nwv
    assert [chosen[96, n] for n in (300, 2048, 4096, 8192)] == [None, None, 12, 12]
    assert [chosen[256, n] for n in (300, 2048, 4096, 8192)] == [None, None, 12, 12]
    assert [chosen[512, n] for n in (300, 2048, 4096, 8192)] == [None, 6, 6, 6]
    assert _waves(640, 2, 1 << 20) is None          # 640 x 65 floats leave no room for three waves' pooled chunks
    assert _dynamic_lds(512, 2, 6) == 133376 + 6 * 4352 == 159488
