"""Every classifier kernel of the C ABI against float64 on the CPU -- never against another float32 GPU convolution.

Layer 1 (test_*_exact_on_integers): integer activations, weights and bias whose every partial sum stays below 2**24 (asserted from
the inputs before the launch, tests/cnn_refs.py): any summation order and any exact operand split then gives the float64 result bit
for bit, so the tolerance is zero.  Three families (narrow / wide activations / wide both), post-ReLU and mixed signs.
Layer 2 (test_*_float32_accurate): seeded random families; max and rms of kernel - float64 over sampled outputs of the placed block
must stay within 3 x those of the same operation evaluated in float32 on the CPU in plain sequential order (for the Winograd
kernels: a numpy float32 F(2x2, 3x3)).  tests/test_cnn_accuracy_cpu.py shows that both checks reject a split-bf16 kernel that lost
products or its third part.
Layer 3 (test_forward_against_float64_network): the classifier's scores and every persistent per-layer tile in each route against
a float64 forward of the full 224 x 224 network, bounded by 3 x the float32 CPU forward's error (floor 4e-7 of the scale).
The measured ratios are in DESIGN.md section 10b; every test prints its own (pytest -rA shows them)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import cnn_refs as R

pytestmark = pytest.mark.gpu
SENT = -7.0
CL = torch.channels_last


def _env():
    from swiftwatcher_amd import _lib
    dev = torch.device("cuda", 0)
    return _lib.load(), dev, ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _nhwc(a, dev):
    return torch.as_tensor(a).to(dev).contiguous(memory_format=CL)


def _placed(call, dev, n, dC, dH, cout, m, off, c_off):
    """Launch into a sentinel-filled destination; -> (rc, placed block on the CPU or None).  Nothing outside the block may change."""
    dst = torch.full((n, dC, dH, dH), SENT, device=dev).contiguous(memory_format=CL)
    torch.cuda.synchronize()
    rc = call(dst)
    torch.cuda.synchronize()
    if rc != 0:
        return rc, None
    blk = dst[:, c_off:c_off + cout, off:off + m, off:off + m].clone()
    dst[:, c_off:c_off + cout, off:off + m, off:off + m] = SENT
    assert bool((dst == SENT).all()), "the kernel wrote outside the placed block"
    return 0, blk.cpu().contiguous(memory_format=torch.contiguous_format)


# ------------------------------------------------------------------ the kernels: geometry of a case and its launch
# Every entry: cases, variants, and functions of a case  geom(case) -> (x shape, cout, k, stride, lo, m),  pre(x, case) -> the tensor
# whose k x k / stride convolution, outputs [lo, lo + m)^2, is the placed block,  run(env, variant, case, x, w, b) -> (rc, block).
def _conv1_geom(c):
    n, side, lo, m = c
    return (n, 3, side, side), 96, 7, 2, lo, m


def _conv1_run(env, variant, c, x, w, b):
    lib, dev, stream = env
    n, side, lo, m = c
    xd, wd, bd = _nhwc(x, dev), torch.as_tensor(w).to(dev).contiguous(), torch.as_tensor(b).to(dev)
    return _placed(lambda dst: lib.swk_nhwc_conv7x7s2_bias_relu(stream, xd.data_ptr(), n, side, lo, m, wd.data_ptr(), bd.data_ptr(), 96, dst.data_ptr()),
                   dev, n, 96, m, 96, m, 0, 0)


def _c1x1_geom(c):
    n, cin, cout, sh, crop, size, dH, off, dC, c_off = c
    return (n, cin, sh, sh), cout, 1, 1, 0, size


def _c1x1_pre(x, c):
    crop, size = c[4], c[5]
    return x[:, :, crop:crop + size, crop:crop + size]


def _c1x1_run(env, variant, c, x, w, b):
    lib, dev, stream = env
    n, cin, cout, sh, crop, size, dH, off, dC, c_off = c
    ring, split = variant
    xd, wd, bd = _nhwc(x, dev), torch.as_tensor(w).reshape(cout, cin).to(dev).contiguous(), torch.as_tensor(b).to(dev)
    assert lib.swk_set_cnn_tuning(0, ring) == 0 and lib.swk_set_cnn_tuning(1, split) == 0
    try:
        return _placed(lambda dst: lib.swk_nhwc_conv1x1_bias_relu_place(stream, xd.data_ptr(), n, sh, sh, cin, crop, crop, size, size, wd.data_ptr(),
                                                                        bd.data_ptr(), cout, dst.data_ptr(), dH, dH, dC, off, off, c_off),
                       dev, n, dC, dH, cout, size, off, c_off)
    finally:
        assert lib.swk_set_cnn_tuning(0, 0) == 0 and lib.swk_set_cnn_tuning(1, 0) == 0


def _poolsq_geom(c):
    n, cin, cout, t, dH, off, dC, lo, ln = c
    return (n, cin, t, t), cout, 1, 1, 0, (t - 3) // 2 + 1


def _poolsq_pre(x, c):
    return torch.nn.functional.max_pool2d(torch.as_tensor(x), 3, 2).numpy()


def _poolsq_shared_ring(x, c):
    """What a forward leaves in the pool tiles: outside the live square every segment holds the first one's values."""
    n, cin, cout, t, dH, off, dC, lo, ln = c
    if ln < 0:
        return x
    inside = np.zeros((1, 1, t, t), bool)
    inside[:, :, lo:lo + ln, lo:lo + ln] = True
    return np.where(inside, x, x[0:1]).astype(np.float32)


def _poolsq_run(env, variant, c, x, w, b):
    lib, dev, stream = env
    n, cin, cout, t, dH, off, dC, lo, ln = c
    p = (t - 3) // 2 + 1
    wd, bd = torch.as_tensor(w).reshape(cout, cin).to(dev).contiguous(), torch.as_tensor(b).to(dev)
    if ln < 0:
        xd, ring, a_, b_ = _nhwc(x, dev), None, 0, 0
    else:          # the shared ring: the segments' own ring pixels hold NaN and must not be read, nor the ring tile's live square
        inside = torch.zeros((1, 1, t, t), dtype=torch.bool)
        inside[:, :, lo:lo + ln, lo:lo + ln] = True
        xt = torch.as_tensor(x)
        nan = torch.full_like(xt, float("nan"))
        xd, ringt, a_, b_ = _nhwc(torch.where(inside, xt, nan), dev), _nhwc(torch.where(inside, nan[0:1], xt[0:1]), dev), lo, ln
        ring = ringt.data_ptr()
    return _placed(lambda dst: lib.swk_nhwc_maxpool3s2_conv1x1_bias_relu_place(stream, xd.data_ptr(), n, t, cin, wd.data_ptr(), bd.data_ptr(), cout,
                                                                               dst.data_ptr(), dH, dH, dC, off, off, ring, a_, b_),
                   dev, n, dC, dH, cout, p, off, 0)


def _c3_geom(c):
    n, cin, cout, t, dH, off, dC, c_off = c
    return (n, cin, t, t), cout, 3, 1, 0, t - 2


def _c3_run(env, variant, c, x, w, b):
    lib, dev, stream = env
    n, cin, cout, t, dH, off, dC, c_off = c
    xd, bd = _nhwc(x, dev), torch.as_tensor(b).to(dev)
    wc = torch.as_tensor(w).contiguous()
    if variant == "direct":
        wd = wc.permute(2, 3, 1, 0).contiguous().to(dev)
        fn = lib.swk_nhwc_conv3x3_bias_relu_place
    elif variant == "wino_f32":
        wd = torch.empty(16 * cin * 32 * (-(-cout // 32)), dtype=torch.float32)
        assert lib.swk_winograd_f2x2_3x3_weights(wc.data_ptr(), cout, cin, wd.data_ptr()) == 0
        wd, fn = wd.to(dev), lib.swk_nhwc_conv3x3_winograd_bias_relu_place
    else:
        wd = torch.empty(3 * 16 * cin * 32 * (-(-cout // 32)), dtype=torch.int16)
        assert lib.swk_winograd_f2x2_3x3_weights_bf16s(wc.data_ptr(), cout, cin, wd.data_ptr()) == 0
        if variant == "wino_bf16s_without_third_part":          # a kernel that lost u3 (the "test tests" run below): [...][part][lane][8]
            wd.view(-1, 3, 512)[:, 2] = 0
        wd, fn = wd.to(dev), lib.swk_nhwc_conv3x3_winograd_bf16s_bias_relu_place
    return _placed(lambda dst: fn(stream, xd.data_ptr(), n, t, cin, wd.data_ptr(), bd.data_ptr(), cout, dst.data_ptr(), dH, dH, dC, off, off, c_off),
                   dev, n, dC, dH, cout, t - 2, off, c_off)


_ident = lambda x, c: x          # noqa: E731

# the shapes of CroppedSqueezeNet10's plan first (test_plan_shapes_are_in_the_lists checks that), then the ragged ones of tests/test_classifier.py
C1X1_CASES = [  # n, cin, cout, sh, crop, size, dH, off, dC, c_off
    (5, 96, 16, 8, 0, 8, 12, 2, 16, 0), (5, 128, 16, 10, 0, 10, 14, 2, 16, 0), (3, 128, 32, 12, 0, 12, 16, 2, 32, 0), (3, 256, 32, 8, 0, 8, 12, 2, 32, 0),
    (7, 256, 48, 10, 0, 10, 14, 2, 48, 0), (2, 384, 48, 12, 0, 12, 16, 2, 48, 0), (2, 384, 64, 14, 0, 14, 18, 2, 64, 0), (4, 512, 64, 9, 0, 9, 13, 2, 64, 0),
    (6, 16, 64, 12, 2, 8, 10, 1, 128, 0), (6, 16, 64, 14, 2, 10, 12, 1, 128, 0), (3, 32, 128, 16, 2, 12, 17, 3, 256, 0), (3, 32, 128, 12, 2, 8, 10, 1, 256, 0),
    (2, 48, 192, 14, 2, 10, 12, 1, 384, 0), (2, 48, 192, 16, 2, 12, 14, 1, 384, 0), (3, 64, 256, 18, 2, 14, 19, 4, 512, 0), (3, 64, 256, 13, 2, 9, 11, 1, 512, 0),
    (3, 128, 32, 14, 0, 14, 16, 1, 32, 0), (7, 256, 48, 12, 0, 12, 14, 1, 48, 0), (1, 64, 96, 7, 2, 3, 5, 1, 160, 60), (9, 16, 4, 5, 0, 5, 5, 0, 8, 4),
    (3, 80, 40, 6, 1, 5, 6, 1, 40, 0), (2, 192, 24, 7, 0, 7, 7, 0, 24, 0), (37, 32, 128, 3, 0, 3, 3, 0, 128, 0),
    # batches that take the 8- and the 16-wave kernels (workgroup size follows the number of 32-pixel row tiles)
    (700, 96, 16, 8, 0, 8, 8, 0, 16, 0), (1400, 16, 64, 10, 1, 8, 8, 0, 128, 64), (160, 48, 192, 12, 0, 12, 12, 0, 384, 0),
    (300, 48, 192, 12, 0, 12, 12, 0, 384, 192), (330, 512, 64, 9, 0, 9, 11, 1, 64, 0)]
C1X1_BENCH = [(2377, 96, 16, 8, 0, 8, 8, 0, 16, 0), (2377, 16, 64, 12, 2, 8, 10, 1, 128, 0)]          # the bench's ragged batch
POOLSQ_CASES = [  # n, cin, cout, t, dH, off, dC, live_lo, live_n (live_n < 0: no shared ring)
    (5, 96, 16, 17, 12, 2, 16, -1, -1), (4, 256, 32, 17, 12, 2, 32, -1, -1), (3, 512, 64, 19, 13, 2, 64, -1, -1), (300, 512, 64, 19, 11, 1, 64, -1, -1),
    (2, 64, 8, 7, 3, 0, 8, -1, -1), (7, 128, 48, 13, 8, 2, 64, -1, -1), (1, 32, 64, 5, 2, 0, 64, -1, -1), (700, 96, 16, 17, 8, 0, 16, -1, -1),
    (37, 256, 32, 17, 12, 2, 32, 2, 12), (300, 512, 64, 19, 13, 2, 64, 3, 14), (5, 96, 16, 17, 8, 0, 16, 0, 17), (9, 64, 8, 9, 4, 0, 8, 4, 1), (3, 64, 8, 9, 4, 0, 8, 2, 0)]
C3_CASES = [  # n, cin, cout, t, dH, off, dC, c_off
    (7, 16, 64, 12, 10, 0, 128, 64), (5, 16, 64, 14, 12, 0, 128, 64), (3, 32, 128, 16, 17, 1, 256, 128), (9, 32, 128, 12, 10, 0, 256, 128),
    (2, 48, 192, 14, 12, 0, 384, 192), (3, 48, 192, 16, 14, 0, 384, 192), (2, 64, 256, 18, 19, 2, 512, 256), (5, 64, 256, 13, 11, 0, 512, 256)]
C3_DIRECT_ONLY = [(1, 16, 40, 5, 4, 1, 44, 4), (300, 16, 64, 4, 2, 0, 64, 0)]
WINO_RAGGED = [(1, 64, 256, 3, 1, 0, 256, 0), (1, 32, 128, 5, 3, 0, 128, 0), (70, 64, 256, 7, 5, 0, 256, 0), (33, 48, 192, 4, 2, 0, 192, 0),
               (130, 16, 64, 5, 3, 0, 64, 0)]
WINO_BENCH = [(2377, 32, 128, 12, 10, 0, 128, 0), (2377, 64, 256, 7, 5, 0, 256, 0)]
CONV1_CASES = [(5, 40, 0, 17), (3, 64, 4, 9), (1, 8, 0, 1), (130, 22, 1, 7)]          # n, side, lo, m


def _c1x1_variants(c):
    # (knob 0, knob 1): both workgroup layouts on the float32 kernel; the split-bf16 kernel where it takes the shape
    return [(0, 0), (1, 0)] + ([(0, 1)] if c[2] == 4 * c[1] and c[1] in (16, 32, 48, 64) else [])


KERNELS = {
    "conv7x7s2": dict(cases=CONV1_CASES, bench=[], geom=_conv1_geom, pre=_ident, run=_conv1_run, variants=lambda c: [None]),
    "conv1x1": dict(cases=C1X1_CASES, bench=C1X1_BENCH, geom=_c1x1_geom, pre=_c1x1_pre, run=_c1x1_run, variants=_c1x1_variants),
    "pool_squeeze": dict(cases=POOLSQ_CASES, bench=[], geom=_poolsq_geom, pre=_poolsq_pre, run=_poolsq_run, variants=lambda c: [None]),
    "conv3x3": dict(cases=C3_CASES + C3_DIRECT_ONLY, bench=[], geom=_c3_geom, pre=_ident, run=_c3_run, variants=lambda c: ["direct"]),
    "winograd": dict(cases=C3_CASES + WINO_RAGGED, bench=WINO_BENCH, geom=_c3_geom, pre=_ident, run=_c3_run,
                     variants=lambda c: ["wino_f32", "wino_bf16s"], wino=True),
}
KERNEL_IDS = sorted(KERNELS)


def test_plan_shapes_are_in_the_lists():
    """Every (cin, cout, tile) CroppedSqueezeNet10's plan hands to a kernel occurs in the case lists above."""
    from swiftwatcher_amd.segment_classification import SegmentClassifier
    from oracle import classifier_ref as ref
    clf = SegmentClassifier.from_state_dict(ref.random_state_dict(1))
    plan = clf.cropped.plan
    have1 = {(c[1], c[2], c[5]) for c in C1X1_CASES}
    have3 = {(c[1], c[2], c[3]) for c in C3_CASES}
    havep = {(c[1], c[2], c[3]) for c in POOLSQ_CASES}
    a, b = clf.cropped.pool1_slice
    assert (5, 40, a, b - a) in CONV1_CASES
    prev_pool = (96, b - a)
    for j, (kind, layer, tile, off, n, pad, crop) in enumerate(plan):
        if kind == "pool":
            prev_pool = (tile.shape[1], tile.shape[2])
            continue
        sq, e1, e3 = layer.squeeze, layer.expand1x1, layer.expand3x3
        assert (sq.in_channels, sq.out_channels, n) in have1, (j, "squeeze")
        assert (e1.in_channels, e1.out_channels, n) in have1, (j, "expand1x1")
        assert (e3.in_channels, e3.out_channels, clf.cropped.sq_bg[j].shape[2]) in have3, (j, "expand3x3")
        if prev_pool is not None:
            assert (prev_pool[0], sq.out_channels, prev_pool[1]) in havep, (j, "pool + squeeze")
            prev_pool = None


# ------------------------------------------------------------------ layer 1
@pytest.mark.parametrize("kernel", KERNEL_IDS)
def test_conv_kernels_exact_on_integers(kernel):
    """Tolerance zero, derived: see the module docstring.  The bound is asserted from the inputs before every launch."""
    K = KERNELS[kernel]
    env = _env()
    wino = K.get("wino", False)
    rng = np.random.default_rng(7)
    bad, launches, widths = [], 0, {}
    for case in K["cases"]:
        shape, cout, k, stride, lo, m = K["geom"](case)
        for family in R.INT_FAMILIES:
            for signed in (False, True):
                if kernel == "pool_squeeze":
                    bound = lambda x, w, b: R.direct_bound(_poolsq_pre(np.abs(x), case), w, b)          # noqa: E731
                elif wino:
                    bound = lambda x, w, b: max(R.wino_bound(x, w, b), R.direct_bound(x, w, b))         # noqa: E731
                else:
                    bound = lambda x, w, b: R.direct_bound(K["pre"](x, case), w, b, stride)             # noqa: E731
                x, w, b, bits, v = R.int_case(rng, family, signed, shape, cout, k, bound, wino=wino)
                if kernel == "pool_squeeze":
                    x = _poolsq_shared_ring(x, case)
                    v = bound(x, w, b)
                assert v < R.LIMIT, (kernel, case, family, v)                    # the precondition of the zero tolerance
                widths[family] = min(bits, widths.get(family, 99))
                xin = torch.as_tensor(np.ascontiguousarray(K["pre"](x, case))).double()
                exp = torch.relu(torch.nn.functional.conv2d(xin, torch.as_tensor(w).double(), torch.as_tensor(b).double(), stride=stride))
                exp = exp[:, :, lo:lo + m, lo:lo + m]
                assert float(exp.abs().max()) < R.LIMIT
                for variant in K["variants"](case):
                    rc, blk = K["run"](env, variant, case, x, w, b)
                    assert rc == 0, (kernel, variant, case, rc)
                    launches += 1
                    wrong = int((blk.double() != exp).sum())
                    if wrong:
                        bad.append((variant, case, family, signed, "%d of %d outputs differ, max |diff| %g" % (
                            wrong, exp.numel(), float((blk.double() - exp).abs().max()))))
    print("%s: %d launches bit-exact against float64; activation bits per family %r" % (kernel, launches - len(bad), widths))
    assert not bad, "\n".join(map(repr, bad))


def test_head_exact_on_integers():
    """swk_nhwc_head2_relu_mean with integer inputs, n_pos a power of two and an integer ring share: sum over channels, ReLU, sum over
    positions, ring and the division are all exact."""
    lib, dev, stream = _env()
    rng = np.random.default_rng(8)
    for c, side, n in ((512, 11, 37), (256, 1, 3), (1024, 4, 5), (768, 11, 2)):
        px, n_pos = side * side, 256.0
        for family in R.INT_FAMILIES:
            for signed in (False, True):
                ring = rng.integers(-1000, 1001, size=(2,)).astype(np.float32)
                bound = lambda x, w, b: px * R.direct_bound(x, w, b) + float(np.abs(ring).max())          # noqa: E731
                x, w, b, bits, v = R.int_case(rng, family, signed, (n, c, side, side), 2, 1, bound)
                assert v < R.LIMIT
                xd, wd = _nhwc(x, dev), torch.as_tensor(w).reshape(2, c).to(dev).contiguous()
                bd, rd = torch.as_tensor(b).to(dev), torch.as_tensor(ring).to(dev)
                out = torch.empty((n, 2), dtype=torch.float32, device=dev)
                assert lib.swk_nhwc_head2_relu_mean(stream, xd.data_ptr(), n, px, c, wd.data_ptr(), bd.data_ptr(), rd.data_ptr(), n_pos, out.data_ptr()) == 0
                torch.cuda.synchronize()
                y = torch.relu(torch.nn.functional.conv2d(torch.as_tensor(x).double(), torch.as_tensor(w).double(), torch.as_tensor(b).double()))
                want = (y.sum(dim=(2, 3)) + torch.as_tensor(ring).double()) / n_pos
                assert torch.equal(out.cpu().double(), want), (c, side, n, family, signed, bits)


def test_placement_helpers_are_bit_exact():
    """swk_nhwc_bias_relu_place and swk_nhwc_maxpool3s2 against the float64 statement rounded once (one float32 add, a comparison):
    random float32 inputs, crop / offset / channel offset, sentinel untouched."""
    lib, dev, stream = _env()
    g = torch.Generator().manual_seed(9)
    for n, c, sh, crop, size, dH, off, dC, c_off in ((5, 64, 12, 1, 10, 12, 2, 128, 64), (3, 96, 17, 0, 17, 17, 0, 96, 0), (1, 4, 3, 2, 1, 2, 1, 8, 4),
                                                     (130, 256, 9, 2, 5, 7, 1, 512, 256), (2377, 16, 5, 1, 3, 3, 0, 16, 0)):
        x = torch.randn((n, c, sh, sh), generator=g) * torch.pow(10.0, torch.rand((n, c, sh, sh), generator=g) * 4.0 - 2.0)
        b = torch.randn((c,), generator=g)
        xd, bd = _nhwc(x, dev), b.to(dev)
        rc, blk = _placed(lambda dst: lib.swk_nhwc_bias_relu_place(stream, xd.data_ptr(), n, sh, sh, c, crop, crop, size, size, bd.data_ptr(),
                                                                   dst.data_ptr(), dH, dH, dC, off, off, c_off), dev, n, dC, dH, c, size, off, c_off)
        assert rc == 0
        want = torch.relu(x[:, :, crop:crop + size, crop:crop + size].double() + b.double().view(1, -1, 1, 1)).float()
        assert torch.equal(blk, want), (n, c, sh)
    for n, c, h, w in ((5, 96, 17, 17), (3, 256, 14, 14), (1, 4, 3, 3), (300, 512, 19, 19), (2377, 16, 8, 6)):
        x = torch.randn((n, c, h, w), generator=g)
        x[n // 2] = -x[n // 2].abs()                  # an all-negative segment: no zero may leak in from a padding
        xd = _nhwc(x, dev)
        oh, ow = (h - 3) // 2 + 1, (w - 3) // 2 + 1
        dst = torch.full((n, c, oh, ow), SENT, device=dev).contiguous(memory_format=CL)
        assert lib.swk_nhwc_maxpool3s2(stream, xd.data_ptr(), n, h, w, c, dst.data_ptr()) == 0
        torch.cuda.synchronize()
        assert torch.equal(dst.cpu().contiguous(), torch.nn.functional.max_pool2d(x.double(), 3, 2).float()), (n, c, h, w)


# ------------------------------------------------------------------ layer 2
def _sampled(rng, K, case, x, w, b, wino):
    """Sampled output positions of the placed block with the float64 reference and the float32 yardstick there."""
    shape, cout, k, stride, lo, m = K["geom"](case)
    n = shape[0]
    xin = np.ascontiguousarray(K["pre"](x, case))
    w2 = w.reshape(cout, -1)
    if wino:
        tiles = max(64, -(-10000 // cout))          # every tile has at least one output inside the block (odd sizes: half-used tiles)
        ni, ty, tx = R.sample_wino(rng, n, m, tiles)
        (ti, a, c), pos = R.wino_positions(ni, ty, tx, m)
        yard = R.wino_f32_tiles(R.wino_tiles(x, ni, ty, tx), w, b)[ti, :, a, c]
    else:
        pos = R.sample_positions(rng, n, m, m, max(128, -(-10000 // cout)))
    a = R.gather_patches(xin, pos[0], pos[1] + lo, pos[2] + lo, k, stride)
    ref = R.f64_product(a, w2, b)
    if not wino:
        yard = R.seq_f32_product(a, w2, b)
    return pos, ref, yard


@pytest.mark.parametrize("kernel", KERNEL_IDS)
def test_conv_kernels_float32_accurate(kernel):
    """max and rms of kernel - float64 within 3 x the plain float32 evaluation's, per case and family (module docstring)."""
    K = KERNELS[kernel]
    env = _env()
    wino = K.get("wino", False)
    g = torch.Generator(device="cpu").manual_seed(11)
    rng = np.random.default_rng(11)
    bad, worst = [], {}
    for case in K["cases"] + K["bench"]:
        for family in R.FAMILIES:
            if family == "zero_segment" and case[0] < 3:
                case_f = (3,) + tuple(case[1:])          # a middle segment needs neighbours
            else:
                case_f = case
            shape, cout, k, stride, lo, m = K["geom"](case_f)
            xt, wt, bt = R.random_case(g, family, shape, cout, k)
            x, w, b = xt.numpy(), wt.numpy(), bt.numpy()
            if kernel == "pool_squeeze":
                x = _poolsq_shared_ring(x, case_f)
            pos, ref, yard = _sampled(rng, K, case_f, x, w, b, wino)
            ys = R.err_stats(yard, ref)
            for variant in K["variants"](case_f):
                rc, blk = K["run"](env, variant, case_f, x, w, b)
                assert rc == 0, (kernel, variant, case_f, rc)
                blk = blk.numpy()
                ks = R.err_stats(blk[pos[0], :, pos[1], pos[2]], ref)
                rt = R.ratios(ks, ys)
                key = (variant, family)
                worst[key] = tuple(max(p, q) for p, q in zip(worst.get(key, (0.0, 0.0)), rt))
                if not R.within(ks, ys):
                    bad.append("%s %r %r %s: kernel max/rms %.3g/%.3g, float32 yardstick %.3g/%.3g, ratios %.2f/%.2f" % (
                        kernel, variant, case_f, family, ks[0], ks[1], ys[0], ys[1], rt[0], rt[1]))
                if family == "zero_segment" and not (kernel == "pool_squeeze" and case_f[8] >= 0):
                    z = blk[shape[0] // 2]
                    if not np.array_equal(z, np.broadcast_to(np.maximum(b, 0)[:, None, None], z.shape)):
                        bad.append("%s %r %r: the all-zero segment's output is not relu(bias)" % (kernel, variant, case_f))
    for (variant, family), rt in sorted(worst.items(), key=repr):
        print("ACCURACY %s %s %s worst max ratio %.2f worst rms ratio %.2f" % (kernel, variant, family, rt[0], rt[1]))
    assert not bad, "\n".join(bad)


def test_criterion_rejects_split_winograd_without_its_third_filter_part():
    """The test tests, on the hardware: the split-bf16 Winograd kernel fed filters whose third bf16 part is zeroed (what a kernel that lost
    u3 computes) fails the criterion on every Fire shape it serves by default, in rms by more than 2 x the allowed factor, while the
    intact operands pass on the same data."""
    K = KERNELS["winograd"]
    env = _env()
    g = torch.Generator(device="cpu").manual_seed(13)
    rng = np.random.default_rng(13)
    for case in C3_CASES[2:]:
        shape, cout, k, stride, lo, m = K["geom"](case)
        xt, wt, bt = R.random_case(g, "relu3", shape, cout, k)
        x, w, b = xt.numpy(), wt.numpy(), bt.numpy()
        pos, ref, yard = _sampled(rng, K, case, x, w, b, True)
        ys = R.err_stats(yard, ref)
        got = {}
        for variant in ("wino_bf16s", "wino_bf16s_without_third_part"):
            rc, blk = K["run"](env, variant, case, x, w, b)
            assert rc == 0
            got[variant] = R.err_stats(blk.numpy()[pos[0], :, pos[1], pos[2]], ref)
        print("ACCURACY mutation %r: intact %.3g/%.3g, without u3 %.3g/%.3g, yardstick %.3g/%.3g" % (
            case, *got["wino_bf16s"], *got["wino_bf16s_without_third_part"], *ys))
        assert R.within(got["wino_bf16s"], ys), (case, got, ys)
        assert not R.within(got["wino_bf16s_without_third_part"], ys), (case, got, ys)
        assert got["wino_bf16s_without_third_part"][1] > 2 * R.FACTOR * ys[1], (case, got, ys)


def test_head_float32_accurate():
    """swk_nhwc_head2_relu_mean on the random families against float64; yardstick: sequential float32 over the channels, then over the
    positions, + ring, / n_pos.  Whole block (2 n outputs)."""
    lib, dev, stream = _env()
    g = torch.Generator(device="cpu").manual_seed(12)
    bad = []
    for c, side, n in ((512, 11, 600), (256, 1, 700), (1024, 4, 300), (768, 11, 37), (512, 11, 2377)):
        px = side * side
        n_pos = float(px + 48)
        for family in R.FAMILIES:
            xt, wt, bt = R.random_case(g, family, (n, c, side, side), 2, 1)
            ring = (torch.randn((2,), generator=g) * 3.0).numpy()
            x, w, b = xt.numpy(), wt.numpy().reshape(2, c), bt.numpy()
            xd, wd, bd, rd = _nhwc(x, dev), wt.reshape(2, c).to(dev).contiguous(), bt.to(dev), torch.as_tensor(ring).to(dev)
            out = torch.empty((n, 2), dtype=torch.float32, device=dev)
            assert lib.swk_nhwc_head2_relu_mean(stream, xd.data_ptr(), n, px, c, wd.data_ptr(), bd.data_ptr(), rd.data_ptr(), n_pos, out.data_ptr()) == 0
            torch.cuda.synchronize()
            rows = np.arange(n) if n <= 600 else np.sort(np.random.default_rng(n).choice(n, 600, replace=False))
            a = np.ascontiguousarray(x[rows].transpose(0, 2, 3, 1)).reshape(-1, c)
            ref = (R.f64_product(a, w, b).reshape(len(rows), px, 2).sum(axis=1) + ring.astype(np.float64)) / np.float64(np.float32(n_pos))
            s = R.seq_f32_product(a, w, b).reshape(len(rows), px, 2)
            acc = np.zeros((len(rows), 2), np.float32)
            for p in range(px):
                acc += s[:, p]
            yard = (acc + ring) / np.float32(n_pos)
            ks, ys = R.err_stats(out.cpu().numpy()[rows], ref), R.err_stats(yard, ref)
            rt = R.ratios(ks, ys)
            print("ACCURACY head c=%d px=%d n=%d %s max ratio %.2f rms ratio %.2f" % (c, px, n, family, rt[0], rt[1]))
            if not R.within(ks, ys):
                bad.append("head %r %s: kernel %.3g/%.3g yardstick %.3g/%.3g" % ((c, side, n), family, ks[0], ks[1], ys[0], ys[1]))
            if family == "zero_segment":
                want = (np.float32(px) * np.maximum(b, 0) + ring) / np.float32(n_pos)
                np.testing.assert_allclose(out.cpu().numpy()[n // 2], want, rtol=3e-7)
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------ layer 3
def _reference_forward(model, x, squares):
    """Scores and the activations on `squares` (name -> (lo, hi)) of a SqueezeNet10 of any dtype; x in chunks to bound the memory."""
    from swiftwatcher_amd.segment_classification import Fire
    acts, scores = {}, []
    with torch.no_grad():
        for i in range(0, x.shape[0], 16):
            h = x[i:i + 16]
            for li, layer in enumerate(model.features):
                if isinstance(layer, Fire):
                    s = torch.relu(layer.squeeze(h))
                    if ("sq", li) in squares:
                        lo, hi = squares[("sq", li)]
                        acts.setdefault(("sq", li), []).append(s[:, :, lo:hi + 1, lo:hi + 1].clone())
                    h = torch.cat([torch.relu(layer.expand1x1(s)), torch.relu(layer.expand3x3(s))], 1)
                else:
                    h = layer(h)
                if ("out", li) in squares:
                    lo, hi = squares[("out", li)]
                    acts.setdefault(("out", li), []).append(h[:, :, lo:hi + 1, lo:hi + 1].clone())
            scores.append(torch.flatten(model.classifier(h), 1))
    return torch.cat(scores), {k: torch.cat(v) for k, v in acts.items()}


def _plan_squares(net, sizes):
    """Where the live squares of the cropped network's persistent tiles sit in the full feature maps: the plan's own recurrence
    (CroppedSqueezeNet10.__init__), checked against the sizes the plan records.  -> {name: (lo, hi)}, [(name, tensor getter)]"""
    from swiftwatcher_amd.segment_classification import _affected
    feats = list(net.model.features)
    lo, hi = _affected(100, 123, 7, 2, 0, sizes[0])
    lo, hi = _affected(lo, hi, 3, 2, 0, sizes[2])
    size = sizes[2]
    squares, tiles = {}, []
    for j, (kind, layer, tile, off, n, pad, crop) in enumerate(net.plan):
        li = 3 + j
        assert feats[li] is layer and hi - lo + 1 == n
        if kind == "fire":
            squares[("sq", li)] = (lo, hi)
            tiles.append((("sq", li), "bufs", j, off + pad[0], n))
            lo, hi = max(lo - 1, 0), min(hi + 1, size - 1)
            assert hi - lo + 1 == crop[1]
            squares[("out", li)] = (lo, hi)
            nxt = net.plan[j + 1] if j + 1 < len(net.plan) else None
            if nxt is not None and nxt[0] == "pool":
                tiles.append((("out", li), "bufs", j + 1, nxt[3], nxt[4]))
            else:
                tiles.append((("out", li), "live", j, 0, crop[1]))
        else:
            lo, hi = _affected(lo, hi, 3, 2, 0, sizes[li])
            size = sizes[li]
    return squares, tiles


ROUTES = ("default", "wino_f32", "direct3x3", "unfused_pool", "full")


def _route_classifier(sd, route):
    from swiftwatcher_amd.segment_classification import SegmentClassifier
    clf = SegmentClassifier.from_state_dict(sd, cropped=route != "full", batch_size=128)
    if route == "wino_f32":
        clf.cropped.wino_split_bf16 = False
    elif route == "direct3x3":
        clf.cropped.winograd = False
    elif route == "unfused_pool":
        clf.cropped.fuse_pool = False
    if route != "full":
        assert clf.cropped.own_kernels and clf.cropped.winograd == (route != "direct3x3")
        assert clf.cropped.wino_split_bf16 == (route not in ("wino_f32",)) and clf.cropped.fuse_pool == (route != "unfused_pool")
    return clf


@pytest.mark.parametrize("weights", ["model_pt", "random"])
def test_forward_against_float64_network(weights, golden_dir):
    """Layer 3 (module docstring): all five routes; the per-layer tiles name the layer where an error enters."""
    from swiftwatcher_amd.segment_classification import SegmentClassifier, SqueezeNet10
    from oracle import classifier_ref as ref
    g = np.load(os.path.join(golden_dir, "classifier_model_pt.npz"))
    crops = [g["crop%d" % i] for i in range(int(g["count"]))]
    if weights == "model_pt":
        sd = {k[2:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("w:")}
    else:
        sd, crops = ref.random_state_dict(21), crops[:32]
    cpu = SegmentClassifier.from_state_dict(sd, device="cpu", cropped=False)
    x = cpu.preprocess(crops)
    net = _route_classifier(sd, "default").cropped
    m32 = SqueezeNet10(2)
    m32.load_state_dict(sd, strict=True)
    m32.eval()
    sizes, h = {}, x[:1]
    with torch.no_grad():
        for li, layer in enumerate(m32.features):
            h = layer(h)
            sizes[li] = h.shape[-1]
    squares, tiles = _plan_squares(net, sizes)
    s32, a32 = _reference_forward(m32, x, squares)
    m64 = SqueezeNet10(2)
    m64.load_state_dict(sd, strict=True)
    m64 = m64.double().eval()
    s64, a64 = _reference_forward(m64, x.double(), squares)
    scale = float(s64.abs().max())
    e32 = float((s32.double() - s64).abs().max())
    bad = []
    for route in ROUTES:
        clf = _route_classifier(sd, route)
        got = clf.scores(crops).cpu().double()
        err = float((got - s64).abs().max())
        bound = max(R.FACTOR * e32, R.FLOOR * scale)
        print("ACCURACY forward %s %s: max |gpu - f64| %.3g, |cpu32 - f64| %.3g, scale %.3g, ratio %.2f" % (weights, route, err, e32, scale, R.ratios((err,), (e32,))[0]))
        if not err <= bound:
            bad.append("scores %s: %.3g > %.3g" % (route, err, bound))
        if route == "full":
            continue
        bufs, live = clf.cropped._buf
        for name, which, j, off, n in tiles:
            t = (bufs if which == "bufs" else live)[j][:len(crops), :, off:off + n, off:off + n].cpu().double()
            ref64 = a64[name]
            assert t.shape == ref64.shape, (name, t.shape, ref64.shape)
            asc = float(ref64.abs().max())
            te, ce = float((t - ref64).abs().max()), float((a32[name].double() - ref64).abs().max())
            if not te <= max(R.FACTOR * ce, R.FLOOR * asc):
                bad.append("tile %s %r (features[%d]): %.3g > 3 x %.3g (scale %.3g)" % (route, name[0], name[1], te, ce, asc))
    assert not bad, "\n".join(bad)
