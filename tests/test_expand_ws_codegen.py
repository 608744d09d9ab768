"""Code-generation guard for the weight-stationary split-bf16 expand1x1 kernel (csrc/cnn_expand_bf16.hip, k_expand1x1_bf16s_ws; no GPU
needed: hipcc cross-compiles).  A wave keeps the split weights of its column block in registers for its whole lifetime (12 per
k-step, 48 at 64 -> 256) beside an accumulator, the operands of a k-step and the staging registers, and the launcher counts on five
waves per SIMD: a spill would put the weights back into memory, a register over the bound would cost the waves that cover the stores.

For every instantiation the launcher can reach, from the kernel's metadata and its code: it exists, ScratchSize is 0, its registers
fit five waves per SIMD (gfx950: 512 registers per SIMD lane, allocated in eights), it issues v_mfma_f32_32x32x16_bf16 and no float32
MFMA, it uses no static LDS, and the dynamic LDS its launcher asks for (two stage buffers and the bias) stays within 160 KB - 256."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

LDS_BOUND = 160 * 1024 - 256
WAVES_PER_SIMD = 5                              # launch_expand_bf16s_ws: by_waves = 20 / NWV; __launch_bounds__(64 NBLK TG, 5)
# launch_expand1x1_split_bf16_ws: <NBLK, KS, TG, TPW>, the wide and the small-launch layout of every Fire shape
INSTANTIATIONS = [(2, 1, 4, 2), (2, 1, 1, 2), (4, 2, 4, 2), (4, 2, 1, 2), (6, 3, 2, 2), (6, 3, 1, 2), (8, 4, 2, 2), (8, 4, 1, 2)]
PITCH = {1: 36, 2: 34, 3: 33, 4: 33}           # ExpandWsPitch


def _dynamic_lds(nblk, ks, tg, tpw):
    """launch_expand_bf16s_ws: two buffers of TG TPW row tiles, each [2 KS items][3 parts][PITCH] x 16 bytes, and the padded bias."""
    return 2 * tg * tpw * 2 * ks * 3 * PITCH[ks] * 16 + 32 * nblk * 4


@pytest.fixture(scope="module")
def expand_asm(tmp_path_factory):
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("hipcc not available")
    from swiftwatcher_amd.csrc import build
    out = tmp_path_factory.mktemp("asm") / "cnn_expand_bf16.s"
    src = os.path.join(ROOT, "swiftwatcher_amd", "csrc", "cnn_expand_bf16.hip")
    flags = [f for f in build.FLAGS if f not in ("-Wall",)]          # the library's own flags
    subprocess.check_call([HIPCC] + flags + ["--cuda-device-only", "-S", src, "-o", str(out)])
    return open(out).read()


def _kernel(asm, inst):
    """(metadata entry, compiler summary, code) of k_expand1x1_bf16s_ws<inst>."""
    prefix = "_ZN3swk20k_expand1x1_bf16s_wsILi%dELi%dELi%dELi%dEEE" % inst
    entries = [e for e in re.split(r"\n  - (?=\.agpr_count:)", asm[asm.index(".amdgpu_metadata"):]) if re.search(r"\.name:\s+" + prefix, e)]
    assert len(entries) == 1, "no instantiation k_expand1x1_bf16s_ws<%d, %d, %d, %d>" % inst
    start = re.search(r"^" + prefix + r"\S*:", asm, re.M).start()
    summary = re.search(r"\.section\s+\.AMDGPU\.csdata.*?; Kernel info:(.*?); COMPUTE_PGM_RSRC2:USER_SGPR", asm[start:], re.S)
    assert summary is not None
    return entries[0], summary.group(1), asm[start:start + summary.start()]


def _field(entry, name):
    return int(re.search(r"\.%s:\s+(\d+)" % name, entry).group(1))


@pytest.mark.parametrize("inst", INSTANTIATIONS, ids=lambda i: "x".join(map(str, i)))
def test_every_reachable_instantiation_keeps_its_weights_in_registers(expand_asm, inst):
    nblk, ks, tg, tpw = inst
    entry, summary, code = _kernel(expand_asm, inst)
    assert int(re.search(r"ScratchSize: (\d+)", summary).group(1)) == 0, "k_expand1x1_bf16s_ws%r spills" % (inst,)
    assert _field(entry, "private_segment_fixed_size") == 0
    assert _field(entry, "max_flat_workgroup_size") == 64 * nblk * tg
    registers = max(_field(entry, "vgpr_count"), (_field(entry, "vgpr_count") - _field(entry, "agpr_count") + 3) // 4 * 4 + _field(entry, "agpr_count"))
    bound = 512 // max(WAVES_PER_SIMD, -(-nblk * tg // 4)) // 8 * 8
    assert bound == 96
    assert registers <= bound, "%d registers: fewer than %d waves per SIMD" % (registers, WAVES_PER_SIMD)
    mfma = re.findall(r"^\s*(v_mfma_\w+)", code, re.M)
    assert mfma and set(mfma) == {"v_mfma_f32_32x32x16_bf16"}, sorted(set(mfma))
    assert len(mfma) % (6 * ks) == 0          # six products per k-step and accumulator
    assert _field(entry, "group_segment_fixed_size") == 0
    assert _dynamic_lds(*inst) <= LDS_BOUND


def test_stage_buffers_leave_room_for_the_workgroups_the_launcher_counts_on():
    """What launch_expand_bf16s_ws works out as workgroups per CU (LDS and five waves per SIMD) keeps at least twelve waves on a CU for
    every layout: one workgroup of 12 or 16 waves, or several narrow ones whose stage buffers fit side by side."""
    per_cu = {}
    for inst in INSTANTIATIONS:
        nblk, ks, tg, tpw = inst
        per_cu[inst] = min(LDS_BOUND // _dynamic_lds(*inst), 4 * WAVES_PER_SIMD // (nblk * tg))
        assert per_cu[inst] >= 1 and per_cu[inst] * nblk * tg >= 12, (inst, per_cu[inst])
    assert [per_cu[i] for i in INSTANTIATIONS] == [2, 10, 1, 5, 1, 3, 1, 2]
    assert _dynamic_lds(8, 4, 2, 2) == 2 * 50688 + 1024
