"""The weight-stationary split-bf16 expand1x1 kernel (csrc/cnn_expand_bf16.hip, k_expand1x1_bf16s_ws; swk_set_cnn_tuning knob 1 = 2):
split weights in registers, split activations shared through LDS.

Against k_expand1x1_bf16s (knob 1 = 1): per accumulator it issues the same MFMAs on the same operands in the same order, so the
whole destination -- the placed block and the sentinel around it -- must be equal bit for bit.  Tolerance zero.
Against float64: the criterion of tests/test_cnn_accuracy.py (tests/cnn_refs.py: FACTOR x the plain float32 evaluation's error, max
and rms), which knob 1 meets on these shapes; and integer inputs with every partial sum below 2**24, where the result is exact.
Whole forward: the default route on the 40 crops of classifier_model_pt.npz within the bound of
test_forward_against_float64_network, bit-identical to a forward with knob 1 = 1, and to the same rows scored as two chains
among 1,100.

Shapes: every Fire shape at the smallest sizes with whole and ragged tiles and stages (a stage of the small-launch layout is 64
pixels), one launch of a single row tile, and every shape just past the 65,536 rows from which it takes its wide layout (several
tile groups per workgroup)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import cnn_refs as R

pytestmark = pytest.mark.gpu
SENT = -7.0
CL = torch.channels_last

# cin, n, size, source side, crop_y, crop_x, dH, dW, off_y, off_x, dC, c_off
CASES = [
    (16, 1, 8, 11, 1, 2, 11, 10, 2, 1, 136, 64),              # 64 rows: two exact tiles, one stage
    (64, 3, 9, 13, 2, 1, 12, 13, 1, 3, 520, 256),             # 243 rows: ragged tile, ragged stage
    (48, 2, 10, 14, 3, 2, 13, 12, 2, 1, 388, 192),            # 200 rows
    (32, 5, 12, 16, 2, 3, 15, 16, 1, 2, 260, 128),            # 720 rows
    (32, 1, 5, 6, 0, 1, 6, 7, 1, 1, 132, 4),                  # 25 rows: a single row tile
    # from 65,536 rows: several tile groups per workgroup, the last stage ragged
    (16, 1025, 8, 9, 1, 0, 9, 8, 1, 0, 72, 8),                # 65,600 rows
    (32, 457, 12, 13, 0, 1, 12, 13, 0, 1, 132, 4),            # 65,808 rows
    (48, 657, 10, 11, 1, 0, 11, 10, 1, 0, 196, 4),            # 65,700 rows
    (64, 811, 9, 10, 0, 1, 9, 10, 0, 1, 260, 4),              # 65,691 rows
]
IDS = ["%d-%dx%dx%d" % (c[0], c[1], c[2], c[2]) for c in CASES]
FAMILIES = ("relu3", "range1e4")


def _env():
    from swiftwatcher_amd import _lib
    dev = torch.device("cuda", 0)
    return _lib.load(), dev, ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _launch(env, knob, case, xd, wd, bd):
    """-> the whole sentinel-filled destination after one launch with knob 1 = knob (restored to the default, 3, afterwards)."""
    lib, dev, stream = env
    cin, n, size, sh, cy, cx, dH, dW, oy, ox, dC, c_off = case
    dst = torch.full((n, dC, dH, dW), SENT, device=dev).contiguous(memory_format=CL)
    torch.cuda.synchronize()
    assert lib.swk_set_cnn_tuning(1, knob) == 0
    try:
        rc = lib.swk_nhwc_conv1x1_bias_relu_place(stream, xd.data_ptr(), n, sh, sh, cin, cy, cx, size, size, wd.data_ptr(), bd.data_ptr(), 4 * cin,
                                                  dst.data_ptr(), dH, dW, dC, oy, ox, c_off)
    finally:
        assert lib.swk_set_cnn_tuning(1, 3) == 0
    torch.cuda.synchronize()
    assert rc == 0, (knob, case, rc)
    return dst


def _block(dst, case):
    cin, n, size, sh, cy, cx, dH, dW, oy, ox, dC, c_off = case
    return dst[:, c_off:c_off + 4 * cin, oy:oy + size, ox:ox + size]


def _outside_untouched(dst, case):
    d = dst.clone()
    _block(d, case).fill_(SENT)
    return bool((d == SENT).all())


def _device(env, x, w, b, cin):
    dev = env[1]
    return (torch.as_tensor(x).to(dev).contiguous(memory_format=CL), torch.as_tensor(w).reshape(4 * cin, cin).to(dev).contiguous(),
            torch.as_tensor(b).to(dev))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_ws_kernel_equals_lds_weight_kernel_and_float64(case):
    env = _env()
    cin, n, size, sh, cy, cx, dH, dW, oy, ox, dC, c_off = case
    cout = 4 * cin
    g = torch.Generator(device="cpu").manual_seed(31 + cin + n)
    rng = np.random.default_rng(31 + cin + n)
    for family in FAMILIES:
        xt, wt, bt = R.random_case(g, family, (n, cin, sh, sh), cout, 1)
        if family == "range1e4":
            xt = torch.relu(xt)          # what an expand reads: a squeeze's ReLU output
        xd, wd, bd = _device(env, xt, wt, bt, cin)
        ws, ld = _launch(env, 2, case, xd, wd, bd), _launch(env, 1, case, xd, wd, bd)
        assert torch.equal(ws, ld), "%s: %d values differ from k_expand1x1_bf16s" % (family, int((ws != ld).sum()))
        assert _outside_untouched(ws, case), "%s: the kernel wrote outside the placed block" % family
        # against float64 on sampled positions of the block, yardstick: plain sequential float32
        pos = R.sample_positions(rng, n, size, size, max(128, -(-10000 // cout)))
        a = R.gather_patches(xt.numpy()[:, :, cy:cy + size, cx:cx + size], pos[0], pos[1], pos[2], 1)
        w2, b = wt.numpy().reshape(cout, cin), bt.numpy()
        ref, yard = R.f64_product(a, w2, b), R.seq_f32_product(a, w2, b)
        got = _block(ws, case).cpu().contiguous(memory_format=torch.contiguous_format).numpy()[pos[0], :, pos[1], pos[2]]
        ks, ys = R.err_stats(got, ref), R.err_stats(yard, ref)
        print("ACCURACY expand_ws %r %s: kernel max/rms %.3g/%.3g, float32 yardstick %.3g/%.3g, ratios %.2f/%.2f" % ((cin, n, size), family, *ks, *ys, *R.ratios(ks, ys)))
        assert R.within(ks, ys), (case, family, ks, ys)


@pytest.mark.parametrize("case", CASES[:5], ids=IDS[:5])
def test_ws_kernel_exact_on_integers(case):
    """Wide activations (up to 21 bits, all three bf16 parts in use), weights +-1, +-2 on three channels: every partial sum is an integer
    below 2**24 (asserted from the inputs), so the kernel's float32 result is the float64 one bit for bit."""
    env = _env()
    cin, n, size, sh, cy, cx, dH, dW, oy, ox, dC, c_off = case
    cout = 4 * cin
    rng = np.random.default_rng(5 + cin)
    for signed in (False, True):
        bound = lambda x, w, b: R.direct_bound(x[:, :, cy:cy + size, cx:cx + size], w, b)          # noqa: E731
        x, w, b, bits, v = R.int_case(rng, "wide_act", signed, (n, cin, sh, sh), cout, 1, bound)
        assert v < R.LIMIT and bits >= 16, (case, bits, v)
        exp = torch.relu(torch.nn.functional.conv2d(torch.as_tensor(np.ascontiguousarray(x[:, :, cy:cy + size, cx:cx + size])).double(),
                                                    torch.as_tensor(w).double(), torch.as_tensor(b).double()))
        xd, wd, bd = _device(env, x, w, b, cin)
        dst = _launch(env, 2, case, xd, wd, bd)
        assert torch.equal(_block(dst, case).cpu().double(), exp), (case, signed, bits)
        assert _outside_untouched(dst, case)


def test_knob_values():
    lib = _env()[0]
    try:
        for value in (0, 1, 2, 3):
            assert lib.swk_set_cnn_tuning(1, value) == 0
        assert lib.swk_set_cnn_tuning(1, 4) != 0 and lib.swk_set_cnn_tuning(1, -1) != 0
    finally:
        assert lib.swk_set_cnn_tuning(1, 3) == 0


def test_default_forward_against_float64_and_the_lds_weight_kernel(golden_dir):
    """The default route (knob 1 = 3) on the 40 crops of the golden model: within 3 x the float32 CPU forward's error against the float64
    network (floor 4e-7 of the scale), equal bit for bit to the forward with every expand1x1 on k_expand1x1_bf16s, and the same scores
    for the same crops among 1,100 (two chains on two streams, wide launches)."""
    from swiftwatcher_amd import _lib
    from swiftwatcher_amd.segment_classification import SegmentClassifier, SqueezeNet10
    from test_cnn_accuracy import _reference_forward
    lib = _lib.load()
    g = np.load(os.path.join(golden_dir, "classifier_model_pt.npz"))
    crops = [g["crop%d" % i] for i in range(int(g["count"]))][:40]
    assert len(crops) == 40
    sd = {k[2:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("w:")}
    x = SegmentClassifier.from_state_dict(sd, device="cpu", cropped=False).preprocess(crops)
    scores = {}
    for name, model, xin in (("f32", SqueezeNet10(2), x), ("f64", SqueezeNet10(2).double(), x.double())):
        model.load_state_dict(sd, strict=True)
        scores[name] = _reference_forward(model.eval(), xin, {})[0].double()
    scale = float(scores["f64"].abs().max())
    e32 = float((scores["f32"] - scores["f64"]).abs().max())
    clf = SegmentClassifier.from_state_dict(sd, batch_size=2048)
    try:
        assert lib.swk_set_cnn_tuning(1, 3) == 0
        got = clf.scores(crops).clone()
        many = clf.scores([crops[i % 40] for i in range(1100)]).clone()
        assert lib.swk_set_cnn_tuning(1, 1) == 0
        lds_weights = clf.scores(crops).clone()
    finally:
        assert lib.swk_set_cnn_tuning(1, 3) == 0
    err = float((got.cpu().double() - scores["f64"]).abs().max())
    print("ACCURACY forward default: max |gpu - f64| %.3g, |cpu32 - f64| %.3g, scale %.3g" % (err, e32, scale))
    assert err <= max(R.FACTOR * e32, R.FLOOR * scale)
    assert torch.equal(got, lds_weights)
    assert many.shape[0] == 1100 and torch.equal(many, got.repeat(28, 1)[:1100])
