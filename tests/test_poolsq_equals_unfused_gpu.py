"""The fused max-pool + squeeze kernel (swk_nhwc_maxpool3s2_conv1x1_bias_relu_place, csrc/cnn_poolsq.hip) against the pair it fuses:
swk_nhwc_maxpool3s2 followed by swk_nhwc_conv1x1_bias_relu_place, placed the same way.  The pooled value is an exact maximum and the
product chain is that of the 1x1 kernel at cin % 32 == 0 (chunks of 32 channels ascending, step i of a chunk multiplies channels
{kb + i, kb + 16 + i}, one accumulator per 32-channel column block), so the two must agree as float32 VALUES: torch.equal over the
whole destination, which is created filled with a sentinel.

The entry point has two kernels behind it (csrc/cnn_poolsq.hip, pool_squeeze_by_row_tiles): a workgroup per segment below two rounds
of the row-tile kernel's resident waves, the row-tile kernel from there on.  Every shape therefore runs twice: with a few segments, and
with enough segments for the row-tile kernel (3 % beyond its threshold, so that the last row tile is ragged too).

Shapes: one row tile of four rows; ragged output widths (8, 48); the network's three pool -> squeeze pairs at a few segments, where the
81 rows of a 9 x 9 map make row tiles straddle segments, also with an even tile side (row and column t - 1 are then never read); and
96 -> 16 on 17 x 17 with a quarter more row tiles than the threshold, 2.5 times what the launcher keeps resident: every wave's load
pipeline runs on into a second and most into a third tile.

Each shape also runs with a ring shared by every tile: outside the live square the segments' own copies are NaN, inside it the ring tile
is NaN.  The result must hold no NaN and equal the run on the fully populated tiles."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

LDS_LIMIT = 160 * 1024 - 256


def _resident_waves(cin, cout):
    """Waves per workgroup of the row-tile kernel = per CU: twelve, halved while the weights [cin][32 nblk + 1], the padded bias and a
    pooled chunk of 32 x 34 floats per wave do not fit the LDS (pool_squeeze_lds): six beside 512 x 65 floats."""
    nblk, nwv = (cout + 31) // 32, 12
    while nwv > 3 and 4 * (((cin * (32 * nblk + 1) + 3) & ~3) + 32 * nblk + nwv * 32 * 34) > LDS_LIMIT:
        nwv //= 2
    return nwv


def _row_tile_segments(cin, cout, t, beyond):
    """Segments for `beyond` times the row tiles (of 32 rows) at which the launcher turns to the row-tile kernel: two rounds of its
    resident waves, 2 x 256 CUs x waves per CU.  96 -> 16 on 17 x 17 (64 rows per segment) with 25 % on top: 2 x 3,072 tiles x 1.25 x
    32 / 64 = 3,840 segments (427 MB of input)."""
    p = (t - 3) // 2 + 1
    return -(-int(2 * 256 * _resident_waves(cin, cout) * beyond * 32) // (p * p))


FEW = [  # n, cin, cout, t
    (1, 32, 64, 5), (2, 64, 8, 7), (7, 128, 48, 13), (3, 96, 16, 17), (5, 256, 32, 17), (3, 512, 64, 19), (5, 512, 64, 20)]
SHAPES = FEW + [(_row_tile_segments(cin, cout, t, 1.25),) + (cin, cout, t) for cin, cout, t in [(96, 16, 17)]] + \
    [(_row_tile_segments(cin, cout, t, 1.03), cin, cout, t) for _, cin, cout, t in FEW]
SENTINEL = -7.0


def _live_squares(t):
    """(live_lo, live_n): the network's two where they fit, the whole tile, one pixel at an odd offset, nothing."""
    return [s for s in ((2, 12), (3, 14)) if s[0] + s[1] <= t] + [(0, t), (3, 1), (2, 0)]


def _nhwc(x):
    return x.contiguous(memory_format=torch.channels_last)


def _fused(lib, stream, src, wgt, bias, cout, dH, dC, off, ring=None, live=(0, 0)):
    n, cin, t = src.shape[0], src.shape[1], src.shape[2]
    dst = _nhwc(torch.full((n, dC, dH, dH), SENTINEL, device=src.device))
    rc = lib.swk_nhwc_maxpool3s2_conv1x1_bias_relu_place(stream, src.data_ptr(), n, t, cin, wgt.data_ptr(), bias.data_ptr(), cout, dst.data_ptr(),
                                                         dH, dH, dC, off, off, None if ring is None else ring.data_ptr(), live[0], live[1])
    assert rc == 0, rc
    return dst


def _unfused(lib, stream, src, wgt, bias, cout, dH, dC, off):
    n, cin, t = src.shape[0], src.shape[1], src.shape[2]
    p = (t - 3) // 2 + 1
    pooled = _nhwc(torch.empty((n, cin, p, p), device=src.device))
    assert lib.swk_nhwc_maxpool3s2(stream, src.data_ptr(), n, t, t, cin, pooled.data_ptr()) == 0
    dst = _nhwc(torch.full((n, dC, dH, dH), SENTINEL, device=src.device))
    rc = lib.swk_nhwc_conv1x1_bias_relu_place(stream, pooled.data_ptr(), n, p, p, cin, 0, 0, p, p, wgt.data_ptr(), bias.data_ptr(), cout,
                                              dst.data_ptr(), dH, dH, dC, off, off, 0)
    assert rc == 0, rc
    return dst


@pytest.mark.parametrize("family", ["randn", "relu"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "n%d_%dto%d_t%d" % s)
def test_fused_equals_pool_then_squeeze(shape, family):
    from swiftwatcher_amd import _lib
    lib = _lib.load()
    n, cin, cout, t = shape
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(1000 * cin + 10 * t + (family == "relu"))
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    p = (t - 3) // 2 + 1
    dH, off, dC = p + 3, 2, (cout + 16 if cout % 32 else cout)          # a destination wider and deeper than the block
    x = torch.randn((n, cin, t, t), generator=g, device=dev)
    if family == "relu":
        x = 3.0 * torch.relu(x)          # what the network feeds this kernel: many exact zeros
    x = _nhwc(x)
    wgt = (torch.randn((cout, cin), generator=g, device=dev) * (2.0 / cin) ** 0.5).contiguous()
    bias = (torch.randn((cout,), generator=g, device=dev) * 0.3).contiguous()

    # ---- every segment's own tile throughout ----
    want = _unfused(lib, stream, x, wgt, bias, cout, dH, dC, off)
    got = _fused(lib, stream, x, wgt, bias, cout, dH, dC, off)
    torch.cuda.synchronize()
    assert torch.equal(got, want), shape
    block = torch.zeros_like(want, dtype=torch.bool)
    block[:, :cout, off:off + p, off:off + p] = True
    assert bool((want[~block] == SENTINEL).all()) and bool((want[block] >= 0.0).all())          # the block and only the block is written
    del want, got

    # ---- a ring shared by every tile ----
    nan = float("nan")
    for lo, ln in _live_squares(t):
        inside = torch.zeros((1, 1, t, t), dtype=torch.bool, device=dev)
        inside[:, :, lo:lo + ln, lo:lo + ln] = True
        full = _nhwc(torch.where(inside, x, x[0:1]))                   # what a forward leaves in the tiles
        src = _nhwc(torch.where(inside, full, torch.full_like(full[0:1], nan)))
        ring = _nhwc(torch.where(inside, torch.full_like(full[0:1], nan), full[0:1]))
        want = _unfused(lib, stream, full, wgt, bias, cout, dH, dC, off)
        whole = _fused(lib, stream, full, wgt, bias, cout, dH, dC, off)
        got = _fused(lib, stream, src, wgt, bias, cout, dH, dC, off, ring, (lo, ln))
        torch.cuda.synchronize()
        assert not bool(torch.isnan(got).any()), (shape, lo, ln)
        assert torch.equal(got, whole) and torch.equal(got, want), (shape, lo, ln)
        del full, src, ring, want, whole, got
