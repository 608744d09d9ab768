"""k_squeeze1x1_bf16s (csrc/cnn_squeeze_bf16.hip): the wide plain squeezes 256 -> 48, 384 -> 48 and 384 -> 64 behind
swk_nhwc_conv1x1_bias_relu_place, float32 products formed from split bf16 operands (swk_set_cnn_tuning knob 4: 1, the default,
takes it; 0 goes back to the float32 kernel).  Held to the project's two criteria (tests/cnn_refs.py):

  * integer inputs with sum |x| |w| + |b| < 2**24, asserted from the inputs before the launch: bit-identical to float64; the three
    activation widths, post-ReLU and mixed signs;
  * the five random families: max and rms error against float64 within 3 x those of the plain sequential float32 evaluation on the
    CPU, over the WHOLE placed block (the cases are small); the all-zero segment's outputs are relu(bias) exactly.

Shapes (tests/squeeze_bf16s_cases.py, whose inputs tests/test_squeeze_bf16s_cpu.py vets on the CPU): the three (cin, cout) pairs on
two segments of 5 x 5 pixels (a whole row tile and a ragged one), 33 rows, and a crop with a placement and channel offset into a
wider destination; every launch goes into a sentinel-filled destination of which nothing outside the placed block may change.
Batch independence: three segments give the same bits alone and inside launches that fill every persistent workgroup with two
and three row tiles per wave.  Knob 4 = 0: the bits of the float32 kernel, shown on the same weights with four more output channels (which no
split kernel takes); the default is as close to float64 as that kernel on the same data."""
import ctypes

import numpy as np
import pytest
import torch

import cnn_refs as R
import squeeze_bf16s_cases as S

pytestmark = pytest.mark.gpu
SENT = -7.0
CL = torch.channels_last


def _env():
    from swiftwatcher_amd import _lib
    dev = torch.device("cuda", 0)
    return _lib.load(), dev, ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _device(env, x, w, b):
    dev = env[1]
    w = torch.as_tensor(w)
    return torch.as_tensor(x).to(dev).contiguous(memory_format=CL), w.reshape(w.shape[0], w.shape[1]).to(dev).contiguous(), torch.as_tensor(b).to(dev)


def _launch(env, case, xd, wd, bd, knob=1):
    """-> the whole sentinel-filled destination after one launch with knob 4 = knob (restored to the default, 1, afterwards)."""
    lib, dev, stream = env
    cin, cout, n, h, w, sh, sw, cy, cx, dH, dW, oy, ox, dC, c_off = case
    dst = torch.full((n, dC, dH, dW), SENT, device=dev).contiguous(memory_format=CL)
    torch.cuda.synchronize()
    assert lib.swk_set_cnn_tuning(4, knob) == 0
    try:
        rc = lib.swk_nhwc_conv1x1_bias_relu_place(stream, xd.data_ptr(), n, sh, sw, cin, cy, cx, h, w, wd.data_ptr(), bd.data_ptr(), cout,
                                                  dst.data_ptr(), dH, dW, dC, oy, ox, c_off)
    finally:
        assert lib.swk_set_cnn_tuning(4, 1) == 0
    torch.cuda.synchronize()
    assert rc == 0, (knob, case, rc)
    return dst


def _block(dst, case):
    cin, cout, n, h, w, sh, sw, cy, cx, dH, dW, oy, ox, dC, c_off = case
    return dst[:, c_off:c_off + cout, oy:oy + h, ox:ox + w]


def _outside_untouched(dst, case):
    d = dst.clone()
    _block(d, case).fill_(SENT)
    return bool((d == SENT).all())


def _rows(dst, case):
    """The placed block as (n h w, cout) on the CPU, rows in the order of squeeze_bf16s_cases.rows_of."""
    return _block(dst, case).permute(0, 2, 3, 1).reshape(-1, case[1]).cpu().numpy()


@pytest.mark.parametrize("case", S.CASES, ids=S.IDS)
def test_exact_on_integers(case):
    env = _env()
    cin, cout, n = case[:3]
    rng = np.random.default_rng(17 + cin + cout)
    widths = {}
    for family in R.INT_FAMILIES:
        for signed in (False, True):
            bound = lambda x, w, b: R.direct_bound(S.window(x, case), w, b)          # noqa: E731
            x, w, b, bits, v = R.int_case(rng, family, signed, (n, cin) + case[5:7], cout, 1, bound)
            assert v < R.LIMIT, (case, family, v)                    # the precondition of the zero tolerance
            widths[family] = min(bits, widths.get(family, 99))
            exp = R.f64_product(S.rows_of(x, case), w.reshape(cout, cin), b)
            assert float(np.abs(exp).max()) < R.LIMIT
            dst = _launch(env, case, *_device(env, x, w, b))
            got = _rows(dst, case).astype(np.float64)
            assert np.array_equal(got, exp), "%s signed=%r: %d of %d outputs differ, max |diff| %g" % (
                family, signed, int((got != exp).sum()), exp.size, float(np.abs(got - exp).max()))
            assert _outside_untouched(dst, case), (family, signed)
    print("squeeze_bf16s %r: bit-exact against float64; activation bits per family %r" % (case[:5], widths))
    assert widths["wide_act"] >= 16          # all three bf16 parts of an activation in use


@pytest.mark.parametrize("case", S.CASES, ids=S.IDS)
def test_float32_accurate(case):
    env = _env()
    bad = []
    for family in R.FAMILIES:
        case_f = S.with_segments(case, 3) if family == "zero_segment" and case[2] < 3 else case          # a middle segment needs neighbours
        cin, cout, n = case_f[:3]
        x, w, b = S.random_inputs(case_f, family)
        a, w2 = S.rows_of(x, case_f), w.reshape(cout, cin)
        ref = R.f64_product(a, w2, b)
        ys = R.err_stats(R.seq_f32_product(a, w2, b), ref)
        dst = _launch(env, case_f, *_device(env, x, w, b))
        got = _rows(dst, case_f)
        ks = R.err_stats(got, ref)
        print("ACCURACY squeeze_bf16s %r %s: kernel max/rms %.3g/%.3g, float32 yardstick %.3g/%.3g, ratios %.2f/%.2f" % (
            case_f[:5], family, *ks, *ys, *R.ratios(ks, ys)))
        if not R.within(ks, ys):
            bad.append((family, ks, ys))
        if not _outside_untouched(dst, case_f):
            bad.append((family, "the kernel wrote outside the placed block"))
        if family == "zero_segment":
            z = got.reshape(n, -1, cout)[n // 2]
            if not np.array_equal(z, np.broadcast_to(np.maximum(b, 0)[None, :], z.shape)):
                bad.append((family, "the all-zero segment's output is not relu(bias)"))
    assert not bad, repr(bad)


def test_batch_independence():
    """256 -> 48 on 10 x 10 (the plan's shape): the rows of a 3-segment launch (ten row tiles on three workgroups, one tile per wave)
    equal, bit for bit, the same segments at the head of launches of 410 segments (1,282 row tiles: all 256 persistent workgroups,
    most waves a second tile) and of 820 (2,563 row tiles, the last ragged: every wave's ring runs on into a second and a third
    tile)."""
    env = _env()
    dev = env[1]
    cin, cout, side = 256, 48, 10
    g = torch.Generator(device=dev).manual_seed(23)
    x = (torch.relu(torch.randn((820, cin, side, side), generator=g, device=dev)) * 3.0).contiguous(memory_format=CL)
    wd = (torch.randn((cout, cin), generator=g, device=dev) * (2.0 / cin) ** 0.5).contiguous()
    bd = (torch.randn((cout,), generator=g, device=dev) * 0.3).contiguous()
    got = {}
    for n in (3, 410, 820):
        case = (cin, cout, n, side, side, side, side, 0, 0, side, side, 0, 0, cout, 0)
        got[n] = _launch(env, case, x[:n], wd, bd)
    assert torch.equal(got[3], got[410][:3]) and torch.equal(got[3], got[820][:3])
    assert torch.equal(got[410], got[820][:410])
    # and the wide launch is right throughout: its last segments against float64
    ref = torch.relu(torch.einsum("nchw,kc->nkhw", x[-2:].double(), wd.double()) + bd.double().view(1, -1, 1, 1))
    assert float((got[820][-2:].double() - ref).abs().max()) <= 1.5e-5 * float(ref.abs().max())          # 256 terms x 2**-24 of the magnitudes' sum


def test_knob_4():
    """knob 4 = 0 puts 384 -> 48 on the float32 kernel: its 48 channels equal, bit for bit, the first 48 of the same launch with
    four more output channels (52: no split kernel's shape, so the float32 kernel's chain whatever the knobs say).  The default
    differs from that in the last bits (another summation order) and is as close to float64 (the assertion of
    test_split_bf16_expand_kernel_is_float32_accurate: 1.5 x the float32 kernel's error, floor 4e-7 of the scale).  Values other than
    0 and 1 are refused."""
    env = _env()
    lib = env[0]
    cin, cout, n, side = 384, 48, 3, 12
    g = torch.Generator(device="cpu").manual_seed(29)
    x = torch.relu(torch.randn((n, cin, side, side), generator=g)) * 3.0
    w = torch.zeros((52, cin))
    w[:cout] = torch.randn((cout, cin), generator=g) * (2.0 / cin) ** 0.5
    b = torch.zeros((52,))
    b[:cout] = torch.randn((cout,), generator=g) * 0.3
    case = (cin, cout, n, side, side, side, side, 0, 0, side, side, 0, 0, cout, 0)
    case52 = (cin, 52, n, side, side, side, side, 0, 0, side, side, 0, 0, 52, 0)
    f32 = _launch(env, case, *_device(env, x, w[:cout], b[:cout]), knob=0)
    wide = _launch(env, case52, *_device(env, x, w, b))
    split = _launch(env, case, *_device(env, x, w[:cout], b[:cout]))
    assert torch.equal(f32, wide[:, :cout]), "knob 4 = 0 does not give the float32 kernel's bits"
    assert not torch.equal(split, f32), "the default did not take another kernel"
    want = torch.relu(torch.einsum("nchw,kc->nkhw", x.double(), w[:cout].double()) + b[:cout].double().view(1, -1, 1, 1))
    scale = float(want.abs().max())
    err = {k: float((v.cpu().double() - want).abs().max()) / scale for k, v in (("split", split), ("f32", f32))}
    print("ACCURACY squeeze_bf16s knob: split %.3g, float32 kernel %.3g of the scale" % (err["split"], err["f32"]))
    assert err["split"] <= max(1.5 * err["f32"], 4e-7), err
    try:
        assert lib.swk_set_cnn_tuning(4, 0) == 0 and lib.swk_set_cnn_tuning(4, 1) == 0
        assert lib.swk_set_cnn_tuning(4, 2) != 0 and lib.swk_set_cnn_tuning(4, -1) != 0
    finally:
        assert lib.swk_set_cnn_tuning(4, 1) == 0
