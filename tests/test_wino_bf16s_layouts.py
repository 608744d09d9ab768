"""The shared-filter layouts of the split-bf16 Winograd expands (k_wino3x3_bf16s_shared_relu_place, csrc/cnn_wino3x3_bf16s.hip): the code
generated for every instantiation the launcher reaches, and the layout switch (swk_set_cnn_tuning knob 2).  No GPU needed."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

# (column blocks, k-steps per phase, tile groups per wave, waves per column block, waves per SIMD) of the launcher's instantiations:
# 32 -> 128 as 8 waves over 128 tiles, 48 -> 192 as 12 waves, 64 -> 256 as 16 waves
LAYOUTS = [(4, 2, 2, 2, 2), (6, 3, 1, 2, 3), (8, 2, 1, 2, 4)]
REGISTERS = {2: 256, 3: 168, 4: 128}          # the register file of a SIMD lane (512) over the waves, in the allocation granule of 8
SYMBOL = "_ZN3swk33k_wino3x3_bf16s_shared_relu_placeILi%dELi%dELi%dELi%dELi%dEEEv"


@pytest.fixture(scope="module")
def wino_asm(tmp_path_factory):
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("hipcc not available")
    from swiftwatcher_amd.csrc import build
    out = tmp_path_factory.mktemp("asm") / "cnn_wino3x3_bf16s.s"
    src = os.path.join(ROOT, "swiftwatcher_amd", "csrc", "cnn_wino3x3_bf16s.hip")
    flags = [f for f in build.FLAGS if f not in ("-Wall",)]
    subprocess.check_call([HIPCC] + flags + ["--cuda-device-only", "-S", src, "-o", str(out)])
    return open(out).read().splitlines()


def _labels(asm):
    return [l.split(":")[0] for l in asm if l.startswith("_ZN3swk33k_wino3x3_bf16s_shared_relu_place") and l.split(";")[0].rstrip().endswith(":")]


def test_the_instantiations_are_those_listed_here(wino_asm):
    """Nothing the launcher can reach escapes the checks below."""
    want = sorted(SYMBOL % lay for lay in LAYOUTS)
    got = sorted(re.match(r"(.*EEEv)", l).group(1) for l in _labels(wino_asm))
    assert got == want


@pytest.mark.parametrize("nblk,spp,tgw,wcb,wps", LAYOUTS)
def test_shared_filter_layout_codegen(wino_asm, nblk, spp, tgw, wcb, wps):
    """No scratch, the registers of the planned waves per SIMD (168 at three, 128 at four, 256 at two) and at least that occupancy,
    6 TGW SPP bf16 MFMAs or more and no float32 ones, the filter stream by LDS-DMA."""
    sym = SYMBOL % (nblk, spp, tgw, wcb, wps)
    start = next(i for i, l in enumerate(wino_asm) if l.startswith(sym) and l.split(";")[0].rstrip().endswith(":"))
    end = next(i for i in range(start, len(wino_asm)) if wino_asm[i].startswith(".Lfunc_end"))
    body, meta = wino_asm[start:end], "\n".join(wino_asm[end:end + 120])
    count = lambda pat: sum(1 for l in body if re.search(pat, l))
    assert count(r"scratch_") == 0
    assert int(re.search(r"ScratchSize: (\d+)", meta).group(1)) == 0
    assert int(re.search(r"NumVgprs: (\d+)", meta).group(1)) + int(re.search(r"NumAgprs: (\d+)", meta).group(1)) <= REGISTERS[wps]
    assert int(re.search(r"Occupancy: (\d+)", meta).group(1)) >= wps
    assert count(r"v_mfma_f32_32x32x16_bf16") >= 6 * tgw * spp
    assert count(r"v_mfma_f32_32x32x2_?f32") == 0
    assert count(r"global_load_lds_dwordx4") >= 1


def test_layout_knob_takes_its_values_and_refuses_others():
    from swiftwatcher_amd import _lib
    lib = _lib.load()
    try:
        for value in (0, 1, 2, 0):
            assert lib.swk_set_cnn_tuning(2, value) == 0
        for value in (-1, 3, 4, 1 << 20):
            assert lib.swk_set_cnn_tuning(2, value) != 0
        assert lib.swk_set_cnn_tuning(3, 0) != 0 and lib.swk_set_cnn_tuning(-1, 0) != 0
    finally:
        assert lib.swk_set_cnn_tuning(2, 0) == 0
