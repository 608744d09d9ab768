"""k_conv7x7s2_bf16s_relu (csrc/cnn_conv1.hip): conv1 behind swk_nhwc_conv7x7s2_bias_relu with float32 products formed from split bf16
operands (swk_set_cnn_tuning knob 4: 1, the default, takes it; 0 goes back to the float32 kernel).  Held to the project's two
criteria (tests/cnn_refs.py) over the WHOLE output block:

  * integer inputs with sum |x| |w| + |b| < 2**24, asserted from the inputs before the launch: bit-identical to float64; the three
    activation widths, post-ReLU and mixed signs;
  * the five random families: max and rms error against float64 within 3 x those of the plain sequential float32 evaluation on the
    CPU; the all-zero segment's outputs are relu(bias) exactly.

Shapes (n, side, first output, count): the plan's window (side 40, outputs 0 .. 16) on three segments (867 rows: 27 row tiles and a
ragged one); 25 outputs (less than one row tile); and a window whose last output's padded patch -- the eighth, zero-weighted row
and the 24th float of a patch row -- ends on the last float of the source (2 (first + count - 1) + 8 = side, the entry point's
limit), in the last segment.  The destination is followed by a sentinel that must survive.
Batch independence: three segments give the same bits alone and at the head of a launch that gives every wave of all 256 persistent
workgroups two row tiles or more.  Knob 4 = 0 takes another kernel (the bits differ), exact on the same integers, and the default is
as close to float64 as it is on the same data."""
import ctypes

import numpy as np
import pytest
import torch

import cnn_refs as R

pytestmark = pytest.mark.gpu
SENT = -7.0
CL = torch.channels_last
CASES = [(3, 40, 0, 17), (1, 22, 1, 5), (2, 16, 1, 4)]          # n, side, lo, m
IDS = ["plan-3x40", "25-outputs", "ends-on-last-float"]
SEED = 41


def _env():
    from swiftwatcher_amd import _lib
    dev = torch.device("cuda", 0)
    return _lib.load(), dev, ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _launch(env, case, xd, wd, bd, knob=1):
    """-> (n, 96, m, m) output on the device; the sentinel behind it is checked."""
    lib, dev, stream = env
    n, side, lo, m = case
    flat = torch.full((n * m * m * 96 + 256,), SENT, device=dev)
    torch.cuda.synchronize()
    assert lib.swk_set_cnn_tuning(4, knob) == 0
    try:
        rc = lib.swk_nhwc_conv7x7s2_bias_relu(stream, xd.data_ptr(), n, side, lo, m, wd.data_ptr(), bd.data_ptr(), 96, flat.data_ptr())
    finally:
        assert lib.swk_set_cnn_tuning(4, 1) == 0
    torch.cuda.synchronize()
    assert rc == 0, (knob, case, rc)
    assert bool((flat[n * m * m * 96:] == SENT).all()), "the kernel wrote past its output"
    return flat[:n * m * m * 96].view(n, m, m, 96)


def _device(env, x, w, b):
    dev = env[1]
    return torch.as_tensor(x).to(dev).contiguous(memory_format=CL), torch.as_tensor(w).to(dev).contiguous(), torch.as_tensor(b).to(dev)


def _patches(x, case):
    """(n m m, 147) patches of the window's outputs, rows in (segment, y, x) order, and the weights' matching reduction order."""
    n, side, lo, m = case
    ni, yi, xi = R.sample_positions(None, n, m, m, 10 ** 9)
    return R.gather_patches(x, ni, yi + lo, xi + lo, 7, 2)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_exact_on_integers(case):
    env = _env()
    n, side, lo, m = case
    rng = np.random.default_rng(SEED + side)
    widths = {}
    for family in R.INT_FAMILIES:
        for signed in (False, True):
            x, w, b, bits, v = R.int_case(rng, family, signed, (n, 3, side, side), 96, 7, lambda x, w, b: R.direct_bound(x, w, b, 2))
            assert v < R.LIMIT, (case, family, v)                    # the precondition of the zero tolerance
            widths[family] = min(bits, widths.get(family, 99))
            exp = R.f64_product(_patches(x, case), w.reshape(96, -1), b)
            for knob in (1, 0):
                got = _launch(env, case, *_device(env, x, w, b), knob=knob).reshape(-1, 96).cpu().numpy().astype(np.float64)
                assert np.array_equal(got, exp), "%s signed=%r knob=%d: %d of %d outputs differ, max |diff| %g" % (
                    family, signed, knob, int((got != exp).sum()), exp.size, float(np.abs(got - exp).max()))
    print("conv1_bf16s %r: bit-exact against float64; activation bits per family %r" % (case, widths))
    assert widths["wide_act"] >= 16          # all three bf16 parts of an activation in use


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_float32_accurate(case):
    env = _env()
    g = torch.Generator(device="cpu").manual_seed(SEED + case[1])
    bad = []
    for family in R.FAMILIES:
        case_f = (3,) + case[1:] if family == "zero_segment" and case[0] < 3 else case          # a middle segment needs neighbours
        n, side, lo, m = case_f
        x, w, b = (t.numpy() for t in R.random_case(g, family, (n, 3, side, side), 96, 7))
        a, w2 = _patches(x, case_f), w.reshape(96, -1)
        ref = R.f64_product(a, w2, b)
        ys = R.err_stats(R.seq_f32_product(a, w2, b), ref)
        got = _launch(env, case_f, *_device(env, x, w, b)).reshape(-1, 96).cpu().numpy()
        ks = R.err_stats(got, ref)
        print("ACCURACY conv1_bf16s %r %s: kernel max/rms %.3g/%.3g, float32 yardstick %.3g/%.3g, ratios %.2f/%.2f" % (
            case_f, family, *ks, *ys, *R.ratios(ks, ys)))
        if not R.within(ks, ys):
            bad.append((family, ks, ys))
        if family == "zero_segment":
            z = got.reshape(n, -1, 96)[n // 2]
            if not np.array_equal(z, np.broadcast_to(np.maximum(b, 0)[None, :], z.shape)):
                bad.append((family, "the all-zero segment's output is not relu(bias)"))
    assert not bad, repr(bad)


def test_batch_independence():
    """The plan's window: three segments alone (28 row tiles on four workgroups) and at the head of 460 (4,155 row tiles, the last
    ragged: 256 persistent workgroups of eight waves, two row tiles per wave and a third for some)."""
    env = _env()
    dev = env[1]
    g = torch.Generator(device=dev).manual_seed(SEED)
    x = torch.randn((460, 3, 40, 40), generator=g, device=dev).contiguous(memory_format=CL)
    wd = (torch.randn((96, 3, 7, 7), generator=g, device=dev) * (2.0 / 147) ** 0.5).contiguous()
    bd = (torch.randn((96,), generator=g, device=dev) * 0.3).contiguous()
    small = _launch(env, (3, 40, 0, 17), x[:3], wd, bd)
    wide = _launch(env, (460, 40, 0, 17), x, wd, bd)
    assert torch.equal(small, wide[:3])
    # and the wide launch is right throughout: its last segments against float64
    ref = torch.relu(torch.nn.functional.conv2d(x[-2:].double(), wd.double(), bd.double(), stride=2))[:, :, :17, :17].permute(0, 2, 3, 1)
    assert float((wide[-2:].double() - ref).abs().max()) <= 1e-5 * float(ref.abs().max())          # 147 terms x 2**-24 of the magnitudes' sum


def test_knob_4_on_conv1():
    """knob 4 = 0 takes the float32 kernel: other bits on random data (another summation order); the default differs from float64 by no
    more than 1.5 x that kernel's own error on the same data, floor 4e-7 of the scale (the assertion of
    test_split_bf16_expand_kernel_is_float32_accurate)."""
    env = _env()
    case = (3, 40, 0, 17)
    g = torch.Generator(device="cpu").manual_seed(SEED + 1)
    x, w, b = R.random_case(g, "relu3", (3, 3, 40, 40), 96, 7)
    dev_in = _device(env, x, w, b)
    split, f32 = _launch(env, case, *dev_in), _launch(env, case, *dev_in, knob=0)
    assert not torch.equal(split, f32), "the knob did not change the kernel"
    want = torch.relu(torch.nn.functional.conv2d(x.double(), w.double(), b.double(), stride=2))[:, :, :17, :17].permute(0, 2, 3, 1)
    scale = float(want.abs().max())
    err = {k: float((v.cpu().double() - want).abs().max()) / scale for k, v in (("split", split), ("f32", f32))}
    print("ACCURACY conv1_bf16s knob: split %.3g, float32 kernel %.3g of the scale" % (err["split"], err["f32"]))
    assert err["split"] <= max(1.5 * err["f32"], 4e-7), err
