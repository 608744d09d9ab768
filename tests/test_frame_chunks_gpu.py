"""Every frame-indexed launcher past its first 32768 frames, and the batch calls past 65535 windows.

Each launcher of csrc/*.hip that splits its frames into launches of 32768 runs here through its public or debug entry point at
F1 = 32768 + 37 frames (F2 = 2 * 32768 + 5 for the cheapest: a middle launch with f0 > 0 and a full count), on a periodic stack of
K = 37 distinct frames (tests/frame_chunks.py).  The result must equal, bit for bit, the entry point's own results on the K distinct
frames in a lone call, tiled -- and those K must equal the CPU restatement of the stage and differ pairwise, or a launch that read
frame 0's slice again could go unseen.  Everything compared is integer or u8: no tolerance (A and E of the window-count test apart,
which depend on the Gram slab count and are held to helpers.ATOL_AE against the lone call).

tests/frame_chunks.INVENTORY names, for every `f0 += 32768` loop and every un-split window grid of the sources, the test in here
that crosses it; tests/test_frame_chunks_cpu.py holds that table to the sources."""
import numpy as np
import pytest

import frame_chunks as fc
from frame_chunks import F1, F2, K, SEG_CAP
from helpers import ATOL_AE, STAGES

pytestmark = pytest.mark.gpu

ERR_HIP, ERR_CAPACITY = -3, -4
_contexts = []


@pytest.fixture(scope="module")
def orc():
    from oracle import reference_path
    return reference_path


@pytest.fixture(scope="module")
def ctx():
    from swiftwatcher_amd import _lib
    c = _lib.Context(0)
    _contexts.append(c)
    yield c
    c.close()


def _np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def _chunks(call, distinct, F, want_K, what):
    """call(stack) -> tuple of per-frame arrays.  The K distinct frames in a lone call equal want_K (the CPU restatement) and differ
    pairwise in every output (outputs of a few bytes a frame: across the launches); the periodic stack of F frames equals the lone call tiled."""
    lone = tuple(_np(a) for a in call(distinct))
    assert len(lone) == len(want_K)
    for i, (got, want) in enumerate(zip(lone, want_K)):
        if want is None:
            continue
        assert got.dtype == want.dtype and np.array_equal(got, want), "%s output %d: the lone call differs from the CPU restatement" % (what, i)
    for i, a in enumerate(lone):
        fc.assert_outputs_tell_frames_apart(a, "%s output %d" % (what, i))
    big = tuple(_np(a) for a in call(fc.periodic(distinct, F)))
    for i, (got, want) in enumerate(zip(big, lone)):
        fc.assert_periodic(got, want, "%s output %d" % (what, i))


# ------------------------------------------------------------------ the stage entry points
@pytest.mark.parametrize("mode", [0, 1], ids=["q14", "q15"])
@pytest.mark.parametrize("H,W", [fc.SHAPE_ALIGNED, (9, 13)], ids=["8x12_k_gray4", "9x13_k_gray4g"])
def test_bgr2gray(ctx, orc, H, W, mode):
    """(single-channel frames reach k_gray through swk_batch_run only: test_batch_run[gray_forced])"""
    frames = fc.bgr_frames(H, W)
    _chunks(lambda s: (ctx.bgr2gray(s, mode),), frames, F2, (fc.orc_gray(orc, frames, mode),), "bgr2gray %dx%d mode %d" % (H, W, mode))


@pytest.mark.parametrize("d", [7, 5])
def test_bilateral_u8(ctx, orc, d):
    planes = fc.gray_planes(9, 13)
    _chunks(lambda s: (ctx.bilateral_u8(s, d=d),), planes, F1, (fc.orc_bilateral(orc, planes, d),), "bilateral_u8 d=%d" % d)


@pytest.mark.parametrize("H,W", fc.SHAPES_ODD, ids=["5x7", "9x13"])
def test_grey_open3x3_u8(ctx, orc, H, W):
    planes = fc.gray_planes(H, W, seed=1)
    _chunks(lambda s: (ctx.grey_open3x3_u8(s),), planes, F2, (fc.orc_open(orc, planes, (3, 3)),), "grey_open3x3_u8 %dx%d" % (H, W))


def test_grey_open_u8(ctx, orc):
    planes = fc.gray_planes(9, 13, seed=2)
    _chunks(lambda s: (ctx.grey_open_u8(s, (4, 7)),), planes, F1, (fc.orc_open(orc, planes, (4, 7)),), "grey_open_u8 (4, 7)")


@pytest.mark.parametrize("cap", [SEG_CAP, 1])
def test_regionprops_u8(ctx, orc, cap):
    labels = fc.label_planes(9, 13)
    _chunks(lambda s: ctx.regionprops_u8(s, seg_cap=cap), labels, F1, fc.orc_regionprops(orc, labels, cap), "regionprops_u8 cap %d" % cap)


def test_segment_shapes_u8(ctx):
    """(the library's shape-sum table of this call is 1.1 GB of device memory: the one exception of the sizing rule)"""
    labels = fc.label_planes(9, 13, seed=1)
    _chunks(lambda s: ctx.segment_shapes_u8(s, seg_cap=SEG_CAP), labels, F1, fc.ref_shapes(labels, SEG_CAP), "segment_shapes_u8")


@pytest.mark.parametrize("conn,order", [(8, 1), (4, 0)], ids=["8way_block", "4way_raster"])
def test_ccl_u8_multi_kernel(ctx, orc, conn, order):
    planes = fc.binary_planes(9, 13)
    ncomp, lab = fc.orc_ccl(orc, planes, conn, order)
    ctx.force_ccl_multi_kernel(True)
    try:
        _chunks(lambda s: ctx.ccl_u8(s, conn, order), planes, F1, (ncomp, lab), "ccl_u8 forced %d/%d" % (conn, order))
    finally:
        ctx.force_ccl_multi_kernel(False)
    # the switch changes the route, not the result
    nc, lab1 = ctx.ccl_u8(planes, conn, order)
    assert np.array_equal(nc, ncomp) and np.array_equal(lab1, lab)


# ------------------------------------------------------------------ stabilization
def test_stabilize(ctx):
    import stabilize_ref
    frames, rect, anchor, moved = fc.stabilize_case()
    want = stabilize_ref.stabilize(frames, rect, fc.STAB_S, anchor)
    assert [(int(s["dy"]), int(s["dx"])) for s in want[0]] == moved, "the restatement finds every frame's known shift"
    assert len(set(moved)) == 25

    def call(s):
        shifts, tab, out = ctx.stabilize(s, rect, fc.STAB_S, anchor, table=True)
        return shifts, tab, out
    _chunks(call, frames, F1, want, "stabilize")
    shifts, tab, out = ctx.stabilize(fc.periodic(frames, F1), rect, fc.STAB_S, anchor)
    assert tab is None
    fc.assert_periodic(shifts, want[0], "stabilize without table: shifts")
    fc.assert_periodic(out, want[2], "stabilize without table: pixels")


def test_stabilize_subpel(ctx):
    import stabilize_subpel_ref as sref
    frames, rect, anchor, moved = fc.stabilize_case(seed=1)
    shifts, (tab, sub), pixels = sref.stabilize_subpel(frames, rect, fc.STAB_S, anchor)
    assert [(int(s["dy"]), int(s["dx"])) for s in shifts] == moved

    def call(s):
        sh, tabs, out = ctx.stabilize_subpel(s, rect, fc.STAB_S, anchor, table=True)
        return sh, tabs[0], tabs[1], out
    _chunks(call, frames, F1, (shifts, tab, sub, pixels), "stabilize_subpel")
    sh, tabs, out = ctx.stabilize_subpel(fc.periodic(frames, F1), rect, fc.STAB_S, anchor)
    assert tabs is None
    fc.assert_periodic(sh, shifts, "stabilize_subpel without tables: records")
    fc.assert_periodic(out, pixels, "stabilize_subpel without tables: pixels")


# ------------------------------------------------------------------ colour conversions
def _dev(a):
    """the planes as device tensors, read in place (a host rectangle that is not the whole frame goes up in one copy per frame: 10^5
    copies for these stacks)"""
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("layout", ["i420", "nv12"])
def test_yuv420_to_bgr(ctx, layout):
    import yuv_ref
    H, W, rect = 10, 14, (3, 1, 11, 9)          # odd origin, odd size
    y, u, v = fc.yuv420_planes(H, W)
    want = yuv_ref.bgr(y, u, v, rect)
    ch, cw = u.shape[1:]

    def call(stack):
        ys, us, vs = stack[:, :H * W].reshape(-1, H, W), stack[:, H * W:H * W + ch * cw].reshape(-1, ch, cw), stack[:, H * W + ch * cw:].reshape(-1, ch, cw)
        if layout == "i420":
            return (ctx.yuv420_to_bgr(_dev(ys), _dev(us), _dev(vs), rect=rect, device_out=True),)
        return (ctx.yuv420_to_bgr(_dev(ys), _dev(np.stack([us, vs], axis=-1)), rect=rect, device_out=True),)
    packed = np.concatenate([y.reshape(K, -1), u.reshape(K, -1), v.reshape(K, -1)], axis=1)
    _chunks(call, packed, F1, (want,), "yuv420_to_bgr " + layout)


@pytest.mark.parametrize("case", ["422_8bit_planar", "420_10bit_semiplanar"])
def test_yuv_to_bgr(ctx, case):
    import yuv_formats_ref as yref
    H, W, rect = 10, 14, (3, 1, 11, 9)
    rng = np.random.default_rng(5)
    if case == "422_8bit_planar":
        sub, bits, dt, kw = (1, 0), 8, np.uint8, {}
    else:
        sub, bits, dt, kw = (1, 1), 10, np.uint16, dict(msb_aligned=True)
    ch, cw = yref.chroma_shape(H, W, *sub)
    hi = 1 << bits
    shift = 16 - bits if kw else 0
    y = (rng.integers(0, hi, size=(K, H, W)) << shift).astype(dt)
    u = (rng.integers(0, hi, size=(K, ch, cw)) << shift).astype(dt)
    v = (rng.integers(0, hi, size=(K, ch, cw)) << shift).astype(dt)
    want = yref.bgr(y, u, v, rect, subsampling=sub, bits=bits, **kw)

    def call(stack):
        ys, us, vs = stack[:, :H * W].reshape(-1, H, W), stack[:, H * W:H * W + ch * cw].reshape(-1, ch, cw), stack[:, H * W + ch * cw:].reshape(-1, ch, cw)
        if case == "422_8bit_planar":
            return (ctx.yuv_to_bgr(_dev(ys), _dev(us), _dev(vs), subsampling=sub, bits=bits, rect=rect, device_out=True),)
        return (ctx.yuv_to_bgr(_dev(ys), _dev(np.stack([us, vs], axis=-1)), subsampling=sub, bits=bits, rect=rect, device_out=True, **kw),)
    packed = np.concatenate([y.reshape(K, -1), u.reshape(K, -1), v.reshape(K, -1)], axis=1)
    _chunks(call, packed, F1, (want,), "yuv_to_bgr " + case)


# ------------------------------------------------------------------ review video
STYLES = [(0, 255, 0, 48, 256), (0, 0, 255, 128, 255), (0, 255, 255, 1, 200), (255, 128, 0, 40, 0), (255, 255, 255, 0, 256), (0, 0, 0, 160, 0)]
REVIEW_RECT = (2, 1, 13, 9)          # (x0, y0, Wc, Hc) inside 11 x 16 frames
MARKED = (0, 5, 20000, 32767, 32768, 32769, F1 - 1)          # frames that carry boxes, marks and labels: both sides of 32768, and the last


def _review_frames():
    return fc.bgr_frames(11, 16, seed=3)


def _crop(frames):
    x0, y0, Wc, Hc = REVIEW_RECT
    return frames[:, y0:y0 + Hc, x0:x0 + Wc]


def test_bgr_to_yuv420(ctx):
    import review_ref as ref
    frames = _review_frames()
    _chunks(lambda s: ctx.bgr_to_yuv420(s, rect=REVIEW_RECT), frames, F1, ref.yuv420(_crop(frames)), "bgr_to_yuv420")


def _overlay(frame_numbers, text):
    """boxes, marks (and labels) on the given frames, each with a geometry that depends on its position in the list"""
    boxes, marks, labels = [], [], []
    for i, f in enumerate(frame_numbers):
        boxes += [(f, i % 4, 1 + i % 5, 5 + i % 4, 8 + i % 5, 1 + i % 2), (f, -1, 6, 4, 20, 2)]
        marks += [(f, 4 + i % 3, 3 + i, 3)]
        labels += [(f, 1, 1 + i % 3, 5, 6, 1, "F%d" % (i % 10))]
    kw = dict(boxes=boxes, marks=marks, styles=STYLES, mark_arm=2, border=1)
    if text:
        kw["labels"] = labels
    return kw


@pytest.mark.parametrize("what", ["plain", "boxes_marks", "text"])
def test_render_review(ctx, what):
    """The overlay's records carry frame numbers: one lies in frame 32767, one in 32768, one in the last frame.  Every frame without
    a record is the plain conversion of its distinct frame (a frame border on every third); the marked frames are compared with the
    restatement of exactly their records."""
    import review_ref as ref
    import review_text_ref as tref
    from swiftwatcher_amd import _lib
    frames = _review_frames()
    crop = _crop(frames)
    if what == "plain":
        _chunks(lambda s: ctx.render_review(s, rect=REVIEW_RECT), frames, F1, ref.yuv420(crop), "render_review plain")
        return
    text = what == "text"
    font = _lib.review_font() if text else None
    render = (lambda fr, **kw: tref.render(fr, font=font, **kw)) if text else ref.render
    border_of = lambda f: 1 if f % 3 == 0 else 0          # noqa: E731
    # the K distinct frames under each of the three border phases, no records: what every unmarked frame must be
    base = {ph: render(crop, styles=STYLES, border=1, mark_arm=2, frame_style=np.array([border_of(ph)] * K, np.int32)) for ph in range(3)}
    assert not np.array_equal(base[0][0], base[1][0])
    kw = _overlay(MARKED, text)
    frame_style = np.array([border_of(f) for f in range(F1)], np.int32)
    got = ctx.render_review(fc.periodic(frames, F1), rect=REVIEW_RECT, frame_style=frame_style, **kw)
    # the marked frames: the restatement on those frames alone, records renumbered
    sel = np.array(MARKED)
    lone_kw = _overlay(range(len(MARKED)), text)
    want_marked = render(crop[sel % K], frame_style=frame_style[sel], **lone_kw)
    lone = ctx.render_review(np.ascontiguousarray(frames[sel % K]), rect=REVIEW_RECT, frame_style=frame_style[sel], **lone_kw)
    for g, w in zip(lone, want_marked):
        assert np.array_equal(g, w), "render_review %s: the lone call on the marked frames differs from the restatement" % what
    idx = np.arange(F1)
    for plane, (g, w) in enumerate(zip(got, want_marked)):
        expect = np.empty_like(g)
        for ph in range(3):
            m = idx % 3 == ph
            expect[m] = base[ph][plane][idx[m] % K]
        assert not np.array_equal(w, expect[sel]), "the records change the marked frames"
        expect[sel] = w
        bad = np.nonzero((g != expect).reshape(F1, -1).any(axis=1))[0]
        assert not len(bad), "render_review %s plane %d: %d frames differ, the first is frame %d" % (what, plane, len(bad), bad[0])


def test_render_review_panels(ctx):
    """two panels (a gray one with gain and a label one) beside the composed frame; captions on both"""
    import review_text_ref as tref
    from review_panels_ref import panel_cell, paste
    from swiftwatcher_amd import _lib
    font, palette = _lib.review_font(), _lib.review_label_palette().astype(np.int64)
    frames = _review_frames()
    crop = _crop(frames)
    x0, y0, Wc, Hc = REVIEW_RECT
    planes = [fc.gray_planes(Hc, Wc, seed=4), fc.label_planes(Hc, Wc, seed=2)]
    specs = [dict(kind="gray", gain=2, layers=0, caption=(1, 1, 5, 6, 1, "G")), dict(kind="labels", layers=0, caption=(1, 1, 3, 0, 1, "L"))]
    overlay = dict(styles=STYLES, mark_arm=2, border=1)
    cells = [tref.render(crop, font=font, **overlay)]
    cells += [panel_cell(p, s["kind"], s.get("gain", 1), s["layers"], s["caption"], overlay, font, palette) for p, s in zip(planes, specs)]
    want = paste(cells, Hc, Wc, 2)

    def call(stack):
        fr = stack[:, :frames[0].size].reshape((-1,) + frames.shape[1:])
        p0 = stack[:, frames[0].size:frames[0].size + Hc * Wc].reshape(-1, Hc, Wc)
        p1 = stack[:, frames[0].size + Hc * Wc:].reshape(-1, Hc, Wc)
        panels = [dict(plane=np.ascontiguousarray(p), **s) for p, s in zip((p0, p1), specs)]
        return ctx.render_review_panels(np.ascontiguousarray(fr), panels=panels, cols=2, rect=REVIEW_RECT, **overlay)
    packed = np.concatenate([frames.reshape(K, -1), planes[0].reshape(K, -1), planes[1].reshape(K, -1)], axis=1)
    _chunks(call, packed, F1, want, "render_review_panels")


# ------------------------------------------------------------------ the fused filter of the batch calls
def _orc_fused(orc, planes, thresh=15):
    bil = fc.orc_bilateral(orc, planes, 7)
    thr = np.stack([orc.thresh_tozero_u8(b, thresh) for b in bil])
    return bil, thr, fc.orc_open(orc, thr, (3, 3))


def test_debug_filter_fused_dense(ctx, orc):
    planes = fc.gray_planes(9, 13, seed=5)

    def call(s):
        out = ctx.debug_filter_fused(s)
        assert (out["guard"] == 0xA5).all()
        return out["bilateral"], out["thresh"], out["opened"]
    _chunks(call, planes, F1, _orc_fused(orc, planes), "debug_filter_fused dense")


def test_debug_filter_fused_geom(ctx, orc):
    """planes of three sizes cycling, at offsets into one buffer with gaps of 0..3 bytes between them: frame f has size f % 3 and shows
    distinct plane f % K of that size (111 different frames)"""
    sizes = [(5, 7), (9, 13), (8, 12)]
    distinct = [fc.gray_planes(H, W, seed=10 + i) for i, (H, W) in enumerate(sizes)]
    lone = []
    for i, planes in enumerate(distinct):
        out = ctx.debug_filter_fused(planes)
        got = (out["bilateral"], out["thresh"], out["opened"])
        for g, w in zip(got, _orc_fused(orc, planes)):
            assert np.array_equal(g, w), "size %d: the lone dense call differs from the CPU restatement" % i
        fc.assert_distinct(np.concatenate([g.reshape(K, -1) for g in got], axis=1), "fused geom size %d" % i)
        lone.append(got)
    geom, off = [], 0
    for f in range(F1):
        H, W = sizes[f % 3]
        off += f % 4
        geom.append((H, W, off))
        off += H * W
    total = off + 5
    src = np.full(total, 200, np.uint8)
    expect = [np.zeros(total, np.uint8) for _ in range(3)]
    for f, (H, W, o) in enumerate(geom):
        src[o:o + H * W] = distinct[f % 3][f % K].reshape(-1)
        for st in range(3):
            expect[st][o:o + H * W] = lone[f % 3][st][f % K].reshape(-1)
    out = ctx.debug_filter_fused(src, geom=geom)
    assert (out["guard"] == 0xA5).all()
    starts = np.array([g[2] for g in geom])
    for st, name in enumerate(("bilateral", "thresh", "opened")):
        bad = np.nonzero(out[name] != expect[st])[0]
        if len(bad):
            f = int(np.searchsorted(starts, bad[0], side="right")) - 1
            raise AssertionError("fused geom %s: %d bytes differ, the first in frame %d (launch %d)" % (name, len(bad), f, f // fc.CHUNK))


# ------------------------------------------------------------------ the batch calls
def _params(**kw):
    from swiftwatcher_amd import _lib
    return _lib.default_params(lmbda=fc.BATCH_LMBDA, **kw)


_window_refs = {}


def _windows(orc, H, W):
    """the K distinct windows of a geometry, checked on the CPU first: (windows (K, 3, H, W, 3), the oracle's results)"""
    if (H, W) not in _window_refs:
        windows = fc.batch_windows(H, W, fc.WINDOW_SEEDS[(H, W)])
        refs, with_segs, masked = fc.window_conditions(orc, windows)
        assert 3 * with_segs >= K, "only %d of the %d distinct windows have a segment on the oracle" % (with_segs, K)
        assert masked == 0, "%d elements of E lie within the band of a byte boundary" % masked
        _window_refs[(H, W)] = (windows, refs)
    return _window_refs[(H, W)]


def _flat(res, n):
    """per-WINDOW arrays of a batch result: the six planes, iters, nseg and the records"""
    nwin = len(res["iters"])
    out = [res[k].reshape(nwin, -1) for k in STAGES]
    out += [res["iters"].reshape(nwin, 1), res["nseg"].reshape(nwin, n)]
    return out, res["segs"].reshape(nwin, -1)


def _check_windows_against_oracle(res, refs, n, cap, what):
    from helpers import orc_seg_tuples, seg_tuples
    for w, ref in enumerate(refs):
        for key in STAGES:
            assert np.array_equal(res[key][w * n:(w + 1) * n], ref[key]), "%s window %d: stage %s differs from the oracle" % (what, w, key)
        assert int(res["iters"][w]) == int(ref["iters"]), (what, w)
        for j in range(n):
            want = orc_seg_tuples(ref["segments"][j])
            assert int(res["nseg"][w * n + j]) == len(want), (what, w, j)
            assert seg_tuples(res, w * n + j)[:cap] == want[:cap], (what, w, j)


def _check_periodic_windows(big, lone, n, what):
    planes_b, segs_b = _flat(big, n)
    planes_l, segs_l = _flat(lone, n)
    for name, b, l in zip(STAGES + ("iters", "nseg"), planes_b, planes_l):
        fc.assert_periodic(b, l, "%s %s (per window)" % (what, name))
    fc.assert_periodic(segs_b, segs_l, "%s records (per window)" % what)


@pytest.mark.parametrize("case", ["bgr", "bgr_forced", "gray_forced"])
def test_batch_run(ctx, orc, case):
    """n = 3, nwin = 10935: frame 32768 is the third frame of window 10922.  As it is; with the multi-kernel labeller forced
    (launch_ccl / launch_regionprops at f0 > 0, records at dsegs + f0 * capmax); and forced on single-channel frames (k_gray)."""
    n, nwin = fc.BATCH_N, fc.BATCH_NWIN
    assert nwin * n == F1
    H, W = fc.SHAPE_BATCH
    windows, refs = _windows(orc, H, W)
    if case == "gray_forced":
        from helpers import gray_u8
        windows = gray_u8(windows)
        flat = windows.reshape(K * n, H, W)
    else:
        flat = windows.reshape(K * n, H, W, 3)
    p = _params()
    ctx.force_ccl_multi_kernel(case != "bgr")
    try:
        lone = ctx.batch_run(flat, K, n, params=p, seg_cap=SEG_CAP)
        _check_windows_against_oracle(lone, refs, n, SEG_CAP, case)
        fc.assert_distinct(lone["gray"].reshape(K, -1), case + " gray")
        big = ctx.batch_run(fc.periodic(windows, nwin).reshape((F1,) + flat.shape[1:]), nwin, n, params=p, seg_cap=SEG_CAP)
    finally:
        ctx.force_ccl_multi_kernel(False)
    _check_periodic_windows(big, lone, n, "batch_run " + case)


def test_batch_run_single_channel_three_launches(ctx, orc):
    """k_gray at F2: 21847 windows of three single-channel frames, the grey plane alone asked for (it passes through)"""
    from helpers import gray_u8
    n, nwin = fc.BATCH_N, F2 // fc.BATCH_N
    assert nwin * n == F2
    H, W = fc.SHAPE_BATCH
    windows, _refs = _windows(orc, H, W)
    gray = gray_u8(windows)                                          # (K, 3, H, W)
    fc.assert_distinct(gray.reshape(K, -1), "single-channel windows")
    p = _params()
    lone = ctx.batch_run(gray.reshape(K * n, H, W), K, n, params=p, stages=("gray",), seg_cap=1)
    assert np.array_equal(lone["gray"], gray.reshape(K * n, H, W))
    big = ctx.batch_run(fc.periodic(gray, nwin).reshape(F2, H, W), nwin, n, params=p, stages=("gray",), seg_cap=1)
    fc.assert_periodic(big["gray"].reshape(nwin, -1), lone["gray"].reshape(K, -1), "batch_run single-channel gray")
    fc.assert_periodic(big["iters"].reshape(nwin, 1), lone["iters"].reshape(K, 1), "batch_run single-channel iters")


def test_batch_run_groups(ctx, orc):
    """two groups of different ROI sizes: 5000 windows of 9 x 14 (frames 0..14999) and 5935 of 12 x 20 (frames 15000..32804): frame
    32768 lies inside the second group.  launch_gray_groups, launch_filter_fused_geom and k_ccl_frame<..., GEOM> with their tables."""
    n = fc.BATCH_N
    geoms = [((9, 14), 5000), ((12, 20), 5935)]
    assert sum(nw for _, nw in geoms) * n == F1 and geoms[0][1] * n < fc.CHUNK
    p = _params()
    specs, lones = [], []
    for (H, W), nwin in geoms:
        windows, refs = _windows(orc, H, W)
        lone = ctx.batch_run(windows.reshape(K * n, H, W, 3), K, n, params=p, seg_cap=SEG_CAP)
        _check_windows_against_oracle(lone, refs, n, SEG_CAP, "lone %dx%d" % (H, W))
        fc.assert_distinct(lone["gray"].reshape(K, -1), "groups gray")
        lones.append(lone)
        specs.append(dict(frames=fc.periodic(windows, nwin).reshape(nwin * n, H, W, 3), nwin=nwin, n=n, seg_cap=SEG_CAP))
    got = ctx.batch_run_groups(specs, params=p)
    for g, (res, lone) in enumerate(zip(got, lones)):
        _check_periodic_windows(res, lone, n, "batch_run_groups group %d" % g)


# ------------------------------------------------------------------ window counts
def _n1_frames():
    return fc.bgr_frames(5, 7, seed=9)


@pytest.mark.parametrize("case", ["auto", "variant1", "want_AE"])
def test_more_windows_than_65535(ctx, orc, case):
    """n = 1: as many windows as the device's grid y extent takes if that is below 2^20, 70,000 otherwise -- every IALM kernel puts
    the window in blockIdx.y.  The default pass; the LDS pass (variant 1); and with A and E asked for (the A / Y-state MFMA pass
    and k_planes_to_pn)."""
    limit = ctx.max_windows()
    nwin = limit if limit < (1 << 20) else 70000
    assert nwin > 65535 or limit <= 65535, limit
    frames = _n1_frames()
    p = _params()
    kw = dict(want_A=True, want_E=True) if case == "want_AE" else {}
    ctx.set_ialm_variant(1 if case == "variant1" else 0)
    try:
        lone = ctx.batch_run(frames, K, 1, params=p, seg_cap=SEG_CAP, **kw)
        for w in range(K):
            ref = orc.window(np.ascontiguousarray(frames[w:w + 1]), lmbda=fc.BATCH_LMBDA)
            for key in STAGES:
                assert np.array_equal(lone[key][w:w + 1], ref[key]), (case, w, key)
            assert int(lone["iters"][w]) == int(ref["iters"]), (case, w)
        fc.assert_distinct(lone["gray"].reshape(K, -1), "n = 1 gray")
        big = ctx.batch_run(fc.periodic(frames, nwin), nwin, 1, params=p, seg_cap=SEG_CAP, **kw)
    finally:
        ctx.set_ialm_variant(0)
    _check_periodic_windows(big, lone, 1, "batch_run n = 1, %d windows, %s" % (nwin, case))
    for key in kw and ("A", "E"):
        assert np.abs(big[key] - fc.tile(lone[key], nwin)).max() <= ATOL_AE, key


def test_one_window_too_many_is_refused(ctx, orc):
    from swiftwatcher_amd import _lib
    limit = ctx.max_windows()
    if limit >= (1 << 24):
        # the frame rule (2^24 frames a call) fires first: the window rule can never
        assert limit >= (1 << 24)
        return
    frames = _n1_frames()
    p = _params()
    small = ctx.batch_run(frames, K, 1, params=p, seg_cap=SEG_CAP)
    before = ctx.device_bytes
    nwin = limit + 1
    # (the refusal comes before the frames are read: a view of the K frames stands in for the stack)
    big = np.lib.stride_tricks.as_strided(frames, shape=(nwin,) + frames.shape[1:], strides=(0,) + frames.strides[1:])
    inp, out, _res = ctx._group_io(big, nwin, 1, None, False, SEG_CAP, STAGES, False, False)
    rc = ctx._lib.swk_batch_run(ctx._h, inp, p, out)
    assert rc == ERR_CAPACITY
    msg = ctx._lib.swk_last_error(ctx._h).decode()
    assert str(limit) in msg, msg
    assert ctx.device_bytes == before
    with pytest.raises(_lib.SwkError):
        ctx.debug_ialm_start(np.zeros((nwin, 1, 16), np.uint8))
    assert ctx.device_bytes == before
    again = ctx.batch_run(frames, K, 1, params=p, seg_cap=SEG_CAP)
    for key in STAGES + ("iters", "nseg", "segs"):
        assert np.array_equal(again[key], small[key]), key


def test_resize_refuses_more_frames_than_grid_z(ctx):
    """k_resize_linear_u8 puts the frame in grid z, not split: swk_resize_linear_u8 refuses a count the extent does not take"""
    src = np.zeros((65536, 1, 1), np.uint8)
    dst = np.zeros((65536, 2, 2), np.uint8)
    before = ctx.device_bytes
    rc = ctx._lib.swk_resize_linear_u8(ctx._h, src.ctypes.data, 65536, 1, 1, 1, 2, 2, dst.ctypes.data)
    assert rc == ERR_CAPACITY and ctx.device_bytes == before
    one = ctx.resize_linear_u8(np.array([[10, 20], [30, 40]], np.uint8), (4, 4))
    from oracle import reference_path
    assert np.array_equal(one, reference_path.resize_linear_u8(np.array([[10, 20], [30, 40]], np.uint8), (4, 4)))


# ------------------------------------------------------------------ at the end: every context is still usable
def test_zz_contexts_still_usable(ctx, orc):
    """(runs last in the module) no call left an error behind: a small call on the module's context is right, and its last error is
    not a HIP error"""
    assert _contexts and all(c._h for c in _contexts)
    for c in _contexts:
        msg = c._lib.swk_last_error(c._h).decode()
        assert "failed:" not in msg, msg          # HIPCHK's message of an SWK_ERR_HIP
        planes = fc.gray_planes(5, 7)
        assert np.array_equal(c.grey_open3x3_u8(planes), fc.orc_open(orc, planes, (3, 3)))
        mask = fc.binary_planes(9, 13)[3]
        nc, lab = c.ccl_u8(mask)
        assert nc == orc.ccl_u8(mask)[0] and np.array_equal(lab, orc.ccl_u8(mask)[1])
