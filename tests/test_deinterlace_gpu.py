"""swk_yuv_deinterlace on the GPU against the numpy restatement of its definition (tests/deinterlace_ref.py) and, for the conversion, the
host restatement of swk_yuv_to_bgr (io_y4m.yuv_rect_to_bgr; tests/yuv_ref.py for 8-bit 4:2:0): planes and BGR bit for bit, at every
shape at which the kernel takes another path."""
import itertools

import numpy as np
import pytest

import deinterlace_cases as cases
import deinterlace_ref as ref
import frame_chunks as fc
import yuv_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from swiftwatcher_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def check(ctx, src, rect=None, planes=None, device_out=False, **params):
    """one call, both outputs, against the restatement"""
    want_bgr, want_pl = src.expected(rect=rect, **params)
    bgr, pl = ctx.yuv_deinterlace(src.planes if planes is None else planes, rect, params.pop("tff"), want_planes=True, device_out=device_out,
                                  **params, **src.kw)
    if device_out:
        bgr, pl = bgr.cpu().numpy(), tuple(None if p is None else p.cpu().numpy() for p in pl)
    what = (src.name, src.count, src.H, src.W, rect, params)
    for got, want, name in zip(pl, want_pl, "YUV"):
        assert cases.same(got, want), (name,) + what
    assert bgr.dtype == np.uint8 and np.array_equal(bgr, want_bgr), ("bgr",) + what


def test_every_width_and_height(ctx):
    """luma W = 1, 2, 3 (no admissible direction), 6 (j = +-1 at two columns), 7, 8, 9 (all), 61..67 (the dword tails); H = 1 (no
    neighbour row), 2 (one), 3.. ; every parameter combination in turn"""
    cyc, ncombos = cases.param_cycle()
    shapes = list(itertools.product((1, 2, 3, 6, 7, 8, 9, 61, 62, 63, 64, 65, 66, 67), (1, 2, 3, 4, 5, 16, 17)))
    assert len(shapes) >= ncombos          # every combination is used
    for (W, H), (count, params) in zip(shapes, cyc):
        check(ctx, cases.Source("mono", count, H, W, seed=W * 100 + H, coarse=(W + H) % 3 == 0), **params)


def test_rectangles_strides_and_parity(ctx):
    """rectangles at every x0 mod 4, odd y0, odd Hr / Wr, touching each picture border and none; row strides above the row; the three
    parity0 pairs"""
    H, W = 21, 37
    rects = [(x0, y0, Wr, Hr) for x0, y0, Wr, Hr in
             [(0, 0, W, H), (0, 0, 9, 7), (1, 1, 11, 5), (2, 3, 13, 9), (3, 5, 7, 3), (4, 7, 33, 14), (5, 1, 32, 20), (6, 0, 31, 1),
              (7, 20, 30, 1), (W - 5, H - 3, 5, 3), (W - 1, 3, 1, 9), (0, 9, 1, 3), (17, 11, 1, 1)]]
    cyc, _ = cases.param_cycle()
    k = 0
    for name in ("420", "444"):
        for rect, parity0 in itertools.product(rects, ((0, 0), (1, 0), (1, 1))):
            count, params = next(cyc)
            check(ctx, cases.Source(name, count, H, W, seed=k, pitch=(0, 3, 8)[k % 3]), rect=rect, parity0=parity0, **params)
            k += 1


@pytest.mark.parametrize("name", sorted(cases.FORMATS))
def test_formats_sources_and_outputs(ctx, name):
    """every format from host and device planes into host and device outputs"""
    import torch
    cyc, _ = cases.param_cycle()
    for k, ((H, W), rect) in enumerate([((10, 18), None), ((13, 27), (5, 3, 17, 9)), ((8, 16), (0, 0, 16, 8)), ((9, 70), (3, 1, 66, 7))]):
        count, params = next(cyc)
        src = cases.Source(name, count, H, W, seed=k, pitch=4 * (k % 2))
        for dev_src, dev_out in itertools.product((False, True), (False, True)):
            check(ctx, src, rect=rect, planes=src.on_device(torch) if dev_src else None, device_out=dev_out, **params)


def test_420_conversion_is_the_opencv_restatement(ctx):
    """8-bit 4:2:0 BGR against tests/yuv_ref.py applied to the restatement's planes"""
    src = cases.Source("420", 3, 14, 22, seed=5)
    bgr = ctx.yuv_deinterlace(src.planes, None, True, **src.kw)
    Y, U, V = ref.call(*src.values, subsampling=(1, 1), tff=True)
    assert np.array_equal(bgr, yuv_ref.bgr(Y.astype(np.uint8), U.astype(np.uint8), V.astype(np.uint8)))


@pytest.mark.parametrize("name,P", cases.DESIGNED, ids=[n for n, _ in cases.DESIGNED])
def test_designed_planes(ctx, name, P):
    """the planes on which one direction, the strict comparison, the search order or one side of the clamp decides (what they must
    give is asserted in tests/test_deinterlace_cpu.py; here the GPU equals the restatement on them)"""
    for bits, tff in ((8, 1), (10, 1), (8, 0)):
        dt = np.uint16 if bits > 8 else np.uint8
        for temporal in (0, 1):
            want = ref.pictures(P, tff, 2, temporal)
            _, (Y, _, _) = ctx.yuv_deinterlace((P.astype(dt),), None, tff, temporal=temporal, want_planes=True, bits=bits)
            assert cases.same(Y, want), (name, bits, tff, temporal)


@pytest.mark.parametrize("name", ["420", "422", "mono", "420p10", "nv12", "p010"])
def test_still_video_gives_yuv_to_bgr_bytes(ctx, name):
    src = cases.Source(name, 4, 11, 23, seed=1, still=True)
    rect = (3, 1, 19, 9)
    plain = ctx.yuv_to_bgr(*src.planes, rect=rect, **src.kw)
    for tff, rate in ((1, 2), (0, 2), (1, 1)):
        got = ctx.yuv_deinterlace(src.planes, rect, tff, rate=rate, **src.kw)
        assert np.array_equal(got, np.repeat(plain, rate, axis=0)), (name, tff, rate)


def test_66000_frames_in_one_call(ctx):
    """66,000 stored mono frames of 2 x 8 with periodic content: 132,000 pictures from one call, no grid limit in the way.  Frame t
    reads frames t - 1 and t + 1, so the expected pictures of the period come from the cyclic stack with one context frame on each
    side; the first and the last frame of the video, which have no neighbour there, are checked on their own."""
    K, F = fc.K, 66000
    stack = cases.rng("many").integers(0, 256, size=(K, 2, 8), dtype=np.uint8)
    video = fc.periodic(stack, F)
    cyclic = np.concatenate([stack[-1:], stack, stack[:1]]).astype(np.int64)
    want = ref.pictures(cyclic, 1, has_prev=True, has_next=True).astype(np.uint8).reshape(K, 2, 2, 8)
    fc.assert_outputs_tell_frames_apart(want, "deinterlaced pictures")
    bgr, (Y, _, _) = ctx.yuv_deinterlace((video,), None, True, want_planes=True)
    assert Y.shape == (2 * F, 2, 8) and bgr.shape == (2 * F, 2, 8, 3)
    Yf = Y.reshape(F, 2, 2, 8)
    fc.assert_periodic(Yf[1:F - 1], np.roll(want, -1, axis=0), "deinterlaced planes, frames 1 .. F - 2")
    assert cases.same(Yf[0].reshape(2, 2, 8), ref.pictures(video[:2].astype(np.int64), 1, has_next=True))
    assert cases.same(Yf[F - 1].reshape(2, 2, 8), ref.pictures(video[F - 2:].astype(np.int64), 1, has_prev=True))
    from swiftwatcher_amd.io_y4m import yuv_rect_to_bgr
    flat = Y.reshape(1, 2 * F * 2, 8)[0]          # (mono conversion is per sample: all pictures as one tall one)
    assert np.array_equal(bgr.reshape(2 * F * 2, 8, 3), yuv_rect_to_bgr(flat, None, None, 0, flat.shape[0], 0, 8))


def _guarded(ctx, torch, src, rect, **params):
    """device outputs between guard bytes: (bgr bytes, planes bytes), after checking the guards"""
    x0, y0, Wr, Hr = rect
    want_bgr, want_pl = src.expected(rect=rect, **params)
    nb = want_bgr.size
    npl = sum(p.size for p in want_pl if p is not None) * (2 if src.bits > 8 else 1)
    G = 64
    bbuf = torch.full((nb + 2 * G,), 0x5A, dtype=torch.uint8, device="cuda")
    pbuf = torch.full((npl + 2 * G,), 0x5A, dtype=torch.uint8, device="cuda")
    import ctypes
    from swiftwatcher_amd import _lib
    s, count, H, W, _, keep = ctx._yuv_source(*(tuple(src.planes) + (None, None))[:3], **src.kw)
    d = _lib.Deinterlace(tff=params.get("tff", 1), rate=params.get("rate", 2), temporal=params.get("temporal", 1),
                         has_prev=params.get("has_prev", 0), has_next=params.get("has_next", 0))
    ctx._check(ctx._lib.swk_yuv_deinterlace(ctx._h, ctypes.byref(s), ctypes.byref(d), count, x0, y0, Hr, Wr, ctypes.c_void_p(bbuf.data_ptr() + G),
                                            _lib.MEM_DEVICE, ctypes.c_void_p(pbuf.data_ptr() + G), _lib.MEM_DEVICE))
    b, p = bbuf.cpu().numpy(), pbuf.cpu().numpy()
    for buf in (b, p):
        assert (buf[:G] == 0x5A).all() and (buf[-G:] == 0x5A).all(), "guard bytes overwritten"
    assert np.array_equal(b[G:-G].reshape(want_bgr.shape), want_bgr)
    return b[G:-G].tobytes(), p[G:-G].tobytes()


def test_history_does_not_matter(ctx):
    """a small call after a larger call of its own, and after swk_stabilize_u8 and swk_render_review on the same context, gives the
    bytes of a fresh context; outputs sit between guard bytes"""
    import torch
    from swiftwatcher_amd import _lib
    small = cases.Source("420", 3, 9, 14, seed=2)
    rect, params = (3, 1, 9, 7), dict(tff=1, has_prev=1)
    fresh = _lib.Context(0)
    want = _guarded(fresh, torch, small, rect, **params)
    fresh.close()
    big = cases.Source("420p10", 5, 40, 70, seed=3)
    ctx.yuv_deinterlace(big.planes, None, False, want_planes=True, **big.kw)
    assert _guarded(ctx, torch, small, rect, **params) == want
    frames = cases.rng("hist").integers(0, 256, size=(4, 30, 40, 3), dtype=np.uint8)
    anchor = ctx.bgr2gray(np.ascontiguousarray(frames[0, 4:24, 4:34]))
    ctx.stabilize(frames, (4, 4, 20, 30), 2, anchor)
    assert _guarded(ctx, torch, small, rect, **params) == want
    ctx.render_review(frames)
    assert _guarded(ctx, torch, small, rect, **params) == want


def test_refusals_leave_the_context_usable(ctx):
    import ctypes
    from swiftwatcher_amd import _lib
    src = cases.Source("420", 3, 8, 12, seed=4)
    good = dict(rect=(0, 0, 12, 8), tff=1)

    def refused(planes=None, rect=(0, 0, 12, 8), kw=None, **params):
        with pytest.raises(_lib.SwkError):
            ctx.yuv_deinterlace(src.planes if planes is None else planes, rect, params.pop("tff", 1), **params, **(src.kw if kw is None else kw))
        check(ctx, src, **good)          # ... and the context still works
    refused(rate=0)
    refused(rate=3)
    refused(has_prev=True, has_next=True, planes=tuple(p[:2] for p in src.planes))          # count 2: nothing left
    refused(has_prev=True, planes=tuple(p[:1] for p in src.planes))
    refused(want_bgr=False)                                                                 # both outputs null
    refused(rect=(0, 0, 13, 8))                                                             # what swk_yuv_to_bgr refuses
    refused(rect=(-1, 0, 4, 4))
    refused(rect=(0, 0, 0, 4))
    refused(kw=dict(src.kw, bits=7))
    refused(kw=dict(src.kw, subsampling=(3, 1)))
    # a null argument, an unknown layout, an unknown mem
    s, count, H, W, _, keep = ctx._yuv_source(*src.planes, **src.kw)
    d = _lib.Deinterlace(tff=1, rate=2, temporal=1)
    out = np.empty((6, 8, 12, 3), np.uint8)
    call = lambda sp, dp, bmem=_lib.MEM_HOST, pl=None, pmem=_lib.MEM_HOST: ctx._lib.swk_yuv_deinterlace(          # noqa: E731
        ctx._h, sp, dp, count, 0, 0, 8, 12, _lib._ptr(out), bmem, pl, pmem)
    assert call(None, ctypes.byref(d)) == -1          # SWK_ERR_ARG
    assert call(ctypes.byref(s), None) == -1
    assert call(ctypes.byref(s), ctypes.byref(d), bmem=7) == -1
    assert call(ctypes.byref(s), ctypes.byref(d), pl=_lib._ptr(out), pmem=7) == -1
    s.layout = 9
    assert call(ctypes.byref(s), ctypes.byref(d)) == -1
    # an odd device address of `planes` with 2-byte samples
    import torch
    wide = cases.Source("420p10", 3, 8, 12, seed=4)
    s16, count, H, W, _, keep16 = ctx._yuv_source(*wide.planes, **wide.kw)
    room = torch.zeros(6 * 8 * 12 * 3 + 16, dtype=torch.uint8, device="cuda:0")
    odd = lambda at: ctx._lib.swk_yuv_deinterlace(ctx._h, ctypes.byref(s16), ctypes.byref(d), count, 0, 0, 8, 12, None, _lib.MEM_HOST,          # noqa: E731
                                                  ctypes.c_void_p(room.data_ptr() + at), _lib.MEM_DEVICE)
    assert odd(1) == -1 and odd(2) == 0
    check(ctx, wide, **good)
    check(ctx, src, **good)
