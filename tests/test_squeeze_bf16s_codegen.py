"""Code-generation guard for k_squeeze1x1_bf16s (csrc/cnn_squeeze_bf16.hip; no GPU needed: hipcc cross-compiles).  A wave keeps a ring
of six or eight activation chunks (16 registers each) beside 32 accumulator registers and two sets of split-weight operands, one wave
per SIMD: a spill would put the ring into memory, and a refill that the scheduler moved next to its use would wait out the memory
latency in every chunk.

For both instantiations the launcher reaches, from the kernel's metadata and its code: it exists, uses no scratch, fits one wave per
SIMD (512 registers), issues v_mfma_f32_32x32x16_bf16 only, in whole k-steps, uses no static LDS, and the dynamic LDS
its launcher asks for stays within 160 KB - 256."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
LDS_BOUND = 160 * 1024 - 256
INSTANTIATIONS = [(16, 8), (24, 6)]          # launch_squeeze1x1_split_bf16: <KS = cin / 16, D = chunks in the ring>


@pytest.fixture(scope="module")
def squeeze_asm(tmp_path_factory):
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("hipcc not available")
    from swiftwatcher_amd.csrc import build
    out = tmp_path_factory.mktemp("asm") / "cnn_squeeze_bf16.s"
    src = os.path.join(ROOT, "swiftwatcher_amd", "csrc", "cnn_squeeze_bf16.hip")
    flags = [f for f in build.FLAGS if f not in ("-Wall",)]          # the library's own flags
    subprocess.check_call([HIPCC] + flags + ["--cuda-device-only", "-S", src, "-o", str(out)])
    return open(out).read()


def _field(entry, name):
    return int(re.search(r"\.%s:\s+(\d+)" % name, entry).group(1))


@pytest.mark.parametrize("inst", INSTANTIATIONS, ids=lambda i: "x".join(map(str, i)))
def test_reachable_instantiations_keep_the_ring_in_registers(squeeze_asm, inst):
    ks, d = inst
    asm = squeeze_asm
    prefix = "_ZN3swk18k_squeeze1x1_bf16sILi%dELi%dEEE" % inst
    entries = [e for e in re.split(r"\n  - (?=\.agpr_count:)", asm[asm.index(".amdgpu_metadata"):]) if re.search(r"\.name:\s+" + prefix, e)]
    assert len(entries) == 1, "no instantiation k_squeeze1x1_bf16s<%d, %d>" % inst
    entry = entries[0]
    start = re.search(r"^" + prefix + r"\S*:", asm, re.M).start()
    code = asm[start:asm.index("s_endpgm", start)]
    assert _field(entry, "private_segment_fixed_size") == 0 and _field(entry, "vgpr_spill_count") == 0, "k_squeeze1x1_bf16s%r spills" % (inst,)
    assert _field(entry, "max_flat_workgroup_size") == 256
    assert _field(entry, "vgpr_count") <= 512
    assert _field(entry, "group_segment_fixed_size") == 0
    mfma = re.findall(r"^\s*(v_mfma_\w+)", code, re.M)
    assert mfma and set(mfma) == {"v_mfma_f32_32x32x16_bf16"}, sorted(set(mfma))
    assert len(mfma) % 12 == 0          # six products per k-step and column block, two column blocks (however the compiler unrolls)
    assert ks * 2 * 3 * 64 * 16 + 64 * 4 <= LDS_BOUND
    # the ring: four 16-byte loads per lane and chunk, the first fill of D chunks and a refill of every slot (the weights' loads on top)
    assert len(re.findall(r"^\s*global_load_dwordx4", code, re.M)) >= 2 * 4 * d
