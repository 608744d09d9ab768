"""The patch staging of the split-bf16 Winograd expands (csrc/cnn_wino3x3_bf16s.hip) loads each patch pixel once per row of positions
and reuses it for the positions that follow: which pixel, tap and sign reaches which output, and many tasks per persistent workgroup.

Both tests compare exactly.  Activations and biases are integers and weights 4 x an integer, so that every entry of G g G^T is an
integer too; every intermediate is then an integer below 2^24, which float32 and the three-way bf16 split carry exactly in any order of
summation.  The reference is a float64 direct convolution + bias + ReLU, the comparison torch.equal.  Every case runs under
swk_set_cnn_tuning(2, v) for v = 0, 1, 2 (the default layout of the shape, k_wino3x3_bf16s_relu_place, the shared-filter layout)."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(16, 64), (32, 128), (48, 192), (64, 256)]
SENTINEL = -7.0


def _lib():
    from swiftwatcher_amd import _lib
    return _lib.load()


def _split_weights(lib, w, dev):
    cout, cin = w.shape[:2]
    assert cout % 32 == 0
    ws = torch.empty(3 * 16 * cin * cout, dtype=torch.int16)
    wc = w.contiguous()
    assert lib.swk_winograd_f2x2_3x3_weights_bf16s(wc.data_ptr(), cout, cin, ws.data_ptr()) == 0
    return ws.to(dev)


def _reference(x_nhwc, w, bias, chunk=4096):
    """float64 direct convolution + bias + ReLU of (N, t, t, cin) -> (N, o, o, cout) float32 (exact: integers), in chunks of segments
    (4,096 segments of 5 x 5 x 64 are 52 MB of float64 input and 75 MB of output)."""
    out = []
    for i in range(0, x_nhwc.shape[0], chunk):
        x = x_nhwc[i:i + chunk].permute(0, 3, 1, 2).double()
        y = torch.relu(torch.nn.functional.conv2d(x, w.double(), bias.double()))
        assert float(y.max()) < 2.0 ** 24
        out.append(y.permute(0, 2, 3, 1).float())
    return torch.cat(out).contiguous()


def _run(lib, stream, src_ptr, n, t, cin, ws, bias, cout, dst_ptr, dH, dW, dC, off_y, off_x, c_off):
    rc = lib.swk_nhwc_conv3x3_winograd_bf16s_bias_relu_place(stream, src_ptr, n, t, cin, ws.data_ptr(), bias.data_ptr(), cout, dst_ptr, dH, dW,
                                                             dC, off_y, off_x, c_off)
    assert rc == 0, (rc, n, t, cin, cout)


@pytest.mark.parametrize("t", [3, 4, 5, 6])
@pytest.mark.parametrize("cin,cout", SHAPES)
def test_every_pixel_reaches_every_output_through_its_own_tap(cin, cout, t):
    """One (input channel, output channel) pair carries 4 x nine distinct powers of two on its taps, a second pair, whose input channel
    lies in the other 4-channel half of the same 8-channel staging item, the same taps in reverse order; all other weights are zero, and
    the input is zero except one pixel of those two channels, set to 1 and stepped over every pixel of the t x t tile of the first, the
    middle and the last of three segments: an output value names the pixel, the tap and the sign that reached it.  The bias
    (4096 + co % 5) lies above every sum of taps, so that a contribution of the wrong sign shows as well.  Odd t: the patches of the last
    tile row and column reach past the tile, those of the last segment past the source (the clamped loads)."""
    lib = _lib()
    dev = torch.device("cuda", 0)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    n, o = 3, t - 2
    ci0, co0 = (7 * t + 1) % cin, (37 * t + 11) % cout
    w = torch.zeros((cout, cin, 3, 3))
    ci1, co1 = ci0 ^ 4, (co0 + 33) % cout
    w[co0, ci0] = 4.0 * torch.pow(2.0, torch.arange(9.0)).reshape(3, 3)
    w[co1, ci1] = 4.0 * torch.pow(2.0, 8.0 - torch.arange(9.0)).reshape(3, 3)
    bias = 4096.0 + (torch.arange(cout) % 5).float()
    runs = [(s, y, x) for s in range(n) for y in range(t) for x in range(t)]
    xs = torch.zeros((len(runs), n, t, t, cin))
    for k, (s, y, x) in enumerate(runs):
        xs[k, s, y, x, ci0] = xs[k, s, y, x, ci1] = 1.0
    ref = _reference(xs.reshape(-1, t, t, cin), w, bias).reshape(len(runs), n, o, o, cout).to(dev)
    # every output of the probed channel is its bias plus at most one tap, and each of the nine taps is reached
    seen = (ref[..., co0] - bias[co0]).unique().tolist()
    assert sorted(seen) == [0.0] + [4.0 * 2.0 ** k for k in range(9)]
    ws, bd, xd = _split_weights(lib, w, dev), bias.to(dev), xs.to(dev)
    try:
        for v in (0, 1, 2):
            assert lib.swk_set_cnn_tuning(2, v) == 0
            got = torch.full_like(ref, SENTINEL)
            for k in range(len(runs)):
                _run(lib, stream, xd[k].data_ptr(), n, t, cin, ws, bd, cout, got[k].data_ptr(), o, o, cout, 0, 0, 0)
            torch.cuda.synchronize()
            if not torch.equal(got, ref):
                bad = (got != ref).nonzero()[0].tolist()
                raise AssertionError("layout %d, %d -> %d, t = %d: run (segment, y, x) = %r differs at (segment, y, x, channel) = %r: %r, not %r"
                                     % (v, cin, cout, t, runs[bad[0]], bad[1:], float(got[tuple(bad)]), float(ref[tuple(bad)])))
    finally:
        assert lib.swk_set_cnn_tuning(2, 0) == 0


# n: every persistent workgroup (at most 512 of 64 tile slots for 32 -> 128, 256 for the wider shapes) runs three tasks or more, and the
# last task is partial: four tiles per segment, 98,308 and 49,156 tiles
MANY = {(32, 128): 24577, (48, 192): 12289, (64, 256): 12289}
_many_cache = {}


def _many_case(cin, cout, dev):
    """Inputs, split weights and the expected destination of a shape, computed once."""
    if (cin, cout) not in _many_cache:
        _many_cache.clear()          # one shape's tensors at a time
        n, t, o = MANY[(cin, cout)], 5, 3
        g = torch.Generator(device="cpu").manual_seed(1000 * cin + cout)
        x = torch.randint(-4, 5, (n, t, t, cin), generator=g).float()
        w = 4.0 * torch.randint(-2, 3, (cout, cin, 3, 3), generator=g).float()
        bias = torch.randint(-8, 9, (cout,), generator=g).float()
        ref = _reference(x, w, bias)
        _many_cache[(cin, cout)] = (x, w, bias, ref)
    return _many_cache[(cin, cout)]


@pytest.mark.parametrize("cin,cout", sorted(MANY))
def test_many_tasks_per_workgroup_place_exact_results(cin, cout):
    """Random integer activations in [-4, 4] and weights 4 x [-2, 2] on ragged 5 x 5 tiles (four tiles per segment, the second row and
    column of tiles half outside), so many segments that every persistent workgroup stages task after task: the staging registers of one
    task's last row of positions must not leak into the next task's first.  The outputs are placed at a nonzero row, column and channel
    offset into a destination filled with a sentinel, which stays untouched around them; the first and the last segment, run alone,
    equal their rows of the batch."""
    lib = _lib()
    dev = torch.device("cuda", 0)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    x, w, bias, ref = _many_case(cin, cout, dev)
    n, t, o = x.shape[0], 5, 3
    assert (n * 4) % 64 != 0 and (n * 4 + 63) // 64 >= 3 * (512 if cin == 32 else 256)
    dH, dW, dC, off_y, off_x, c_off = o + 1, o + 2, cout + 8, 1, 2, 4
    blk = (slice(None), slice(off_y, off_y + o), slice(off_x, off_x + o), slice(c_off, c_off + cout))
    want = torch.full((n, dH, dW, dC), SENTINEL, device=dev)
    want[blk] = ref.to(dev)
    ws, bd, xd = _split_weights(lib, w, dev), bias.to(dev), x.to(dev)
    try:
        for v in (0, 1, 2):
            assert lib.swk_set_cnn_tuning(2, v) == 0
            got = torch.full_like(want, SENTINEL)
            _run(lib, stream, xd.data_ptr(), n, t, cin, ws, bd, cout, got.data_ptr(), dH, dW, dC, off_y, off_x, c_off)
            ones = []
            for k in (0, n - 1):
                one = torch.full_like(want[k:k + 1], SENTINEL)
                _run(lib, stream, xd[k:k + 1].data_ptr(), 1, t, cin, ws, bd, cout, one.data_ptr(), dH, dW, dC, off_y, off_x, c_off)
                ones.append((k, one))
            torch.cuda.synchronize()
            if not torch.equal(got, want):          # values and sentinel at once
                bad = (got != want).nonzero()
                raise AssertionError("layout %d, %d -> %d: %d values differ, the first at (segment, y, x, channel) = %r: %r, not %r"
                                     % (v, cin, cout, len(bad), bad[0].tolist(), float(got[tuple(bad[0].tolist())]),
                                        float(want[tuple(bad[0].tolist())])))
            for k, one in ones:
                assert torch.equal(one, got[k:k + 1]), (v, cin, cout, k)
    finally:
        assert lib.swk_set_cnn_tuning(2, 0) == 0
