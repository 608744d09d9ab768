"""The review video's stage panels on the MI355X: swk_render_review_panels bit for bit, on all three planes, against a mosaic built
from the definition's restatements (tests/review_ref.py, tests/review_text_ref.py, tests/review_panels_ref.py): every panel's plane mapped to BGR in numpy (gain
or the library's palette), composed with its selected layers and its caption, converted, and pasted by _lib.panel_layout; Y = 16 and
U = V = 128 everywhere else.  All comparisons are of integers: exact."""
import ctypes

import numpy as np
import pytest

import review_ref as ref
import review_text_ref as tref
from review_panels_ref import panel_bgr, panel_cell, paste

pytestmark = pytest.mark.gpu

# (b, g, r, fill_alpha, line_alpha): 1..4 box / mark / border / mask styles, 5 opaque ink, 6 plate, 7 translucent ink and plate
STYLES = [(0, 255, 0, 48, 256), (0, 0, 255, 128, 255), (0, 255, 255, 1, 200), (255, 128, 0, 40, 0), (255, 255, 255, 0, 256), (0, 0, 0, 160, 0),
          (90, 0, 200, 77, 130)]
SIZES = [(2, 2), (3, 5), (6, 8), (7, 13), (16, 64), (47, 94)]          # a single strip, both pads, ragged last strips, an unaligned row start
ARG, CAPACITY = -1, -4


@pytest.fixture(scope="module")
def ctx():
    from swiftwatcher_amd import _lib
    return _lib.default_context(0)


@pytest.fixture(scope="module")
def font():
    from swiftwatcher_amd import _lib
    return _lib.review_font()


@pytest.fixture(scope="module")
def palette():
    from swiftwatcher_amd import _lib
    return _lib.review_label_palette().astype(np.int64)


def _np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else a


def _same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        g = _np(g)
        assert g.dtype == np.uint8 and g.shape == w.shape and np.array_equal(g, w)


# ------------------------------------------------------------------------------------------ 1. the mosaic at every size
def _checker(H, W):
    rr, cc = np.mgrid[0:H, 0:W]
    return (((rr + cc) & 1) * 255).astype(np.uint8)


def _overlay(F, H, W):
    """Boxes that leave the panel on every side, a small one, marks on and off the frame, a border on the even frames, a mask."""
    boxes, marks = [], []
    for f in range(F):
        boxes += [(f, -2, -3, H + 2, W // 2 + 1, 1), (f, H // 2, W // 3, H + 5, W + 4, 2), (f, 0, 0, 2, 3, 7)]
        marks += [(f, H // 2, W // 2, 3), (f, -1, W - 1, 7)]
    return dict(boxes=boxes, marks=marks, frame_style=[3 if f % 2 == 0 else 0 for f in range(F)], mask=_checker(H, W), styles=STYLES, mask_style=4,
                mark_arm=3, border=1)


def _planes(seed, F, H, W):
    """Four u8 planes (F, H, W): two gray ones whose values cross 63 / 64 (gain 4 saturates from 64 on), one of label values cycling
    through 0..255 from an offset, one gray again."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(4):
        p = rng.integers(0, 256, (F, H, W), dtype=np.uint8)
        if k == 2:
            p = ((np.arange(F * H * W) + 250) % 256).astype(np.uint8).reshape(F, H, W)          # (250..255, then 0, 1, ...)
        else:
            p.reshape(-1)[:4] = [63, 64, 255, 1]
        out.append(p)
    return out


_CASES = {}


def _case(H, W, F, font, palette):
    """The mosaic's parts at one size and frame count, computed once: frames, overlay, labels, the panels' planes and specs, and every
    cell's expected (y, u, v)."""
    key = (H, W, F)
    if key not in _CASES:
        frames = np.random.default_rng(H * 100 + W + F).integers(0, 256, (F, H + 2, W + 3, 3), dtype=np.uint8)
        rect = (2, 1, W, H)
        overlay = _overlay(F, H, W)
        labels = [(f, 0, 1, 7, 6, 1, "F%d" % f) for f in range(F)]
        planes = _planes(H * 1000 + W * 10 + F, F, H, W)
        specs = [dict(kind="gray", gain=1, layers=0, caption=(1, 1, 5, 6, 1, "G")),
                 dict(kind="gray", gain=4, layers=2, caption=(-2, -3, 5, 6, 2, "X4")),
                 dict(kind="labels", layers=15, caption=(1, 1, 3, 0, 1, "L")),
                 dict(kind="gray", gain=4, layers=15, caption=None)]
        cells = [tref.render(frames[:, 1:1 + H, 2:2 + W], labels=labels, font=font, **overlay)]
        cells += [panel_cell(p, s["kind"], s.get("gain", 1), s["layers"], s["caption"], overlay, font, palette) for p, s in zip(planes, specs)]
        assert int(planes[1].max()) * 4 > 255 and (planes[1] == 63).any() and (planes[1] == 64).any()          # the gain saturates, and 63 does not
        _CASES[key] = dict(frames=frames, rect=rect, overlay=overlay, labels=labels, planes=planes, specs=specs, cells=cells)
    return _CASES[key]


def _panel_dicts(case, device):
    """The four panels over their planes as the library may meet them: a device plane stored newest frame first and read backwards
    (negative frame stride), a host plane inside wider rows, a device plane inside wider rows starting at an odd address, a dense
    host plane.  Returns (dicts, what must stay alive)."""
    import torch
    p0, p1, p2, p3 = case["planes"]
    F, H, W = p0.shape
    specs = [dict(s) for s in case["specs"]]
    t0 = torch.from_numpy(p0[::-1].copy()).cuda()
    specs[0]["plane"] = {"ptr": t0.data_ptr() + (F - 1) * H * W, "frame_stride": -H * W, "row_stride": W}
    wide1 = np.full((F, H + 1, W + 5), 0xEE, np.uint8)
    wide1[:, :H, 3:3 + W] = p1
    specs[1]["plane"] = wide1[:, :H, 3:3 + W]
    wide2 = np.full((F, H, W + 7), 0xDD, np.uint8)
    wide2[:, :, 1:1 + W] = p2
    t2 = torch.from_numpy(wide2).cuda()
    specs[2]["plane"] = t2[:, :, 1:1 + W]
    specs[3]["plane"] = p3 if not device else torch.from_numpy(p3).cuda()
    return specs, (t0, t2, wide1)


@pytest.mark.parametrize("layout", ["i420", "nv12"])
@pytest.mark.parametrize("cols", [1, 2, 5])
@pytest.mark.parametrize("F", [1, 5])
@pytest.mark.parametrize("H,W", SIZES)
def test_mosaic(ctx, font, palette, H, W, F, cols, layout):
    """Five cells (cols = 2 leaves the sixth place empty): host frames into a host destination as I420, device frames into a device
    destination as NV12."""
    import torch
    case = _case(H, W, F, font, palette)
    device = layout == "nv12"
    panels, keep = _panel_dicts(case, device)
    y, u, v = paste(case["cells"], H, W, cols)
    frames = torch.from_numpy(case["frames"]).cuda() if device else case["frames"]
    got = ctx.render_review_panels(frames, panels=panels, cols=cols, rect=case["rect"], labels=case["labels"], layout=layout, device_out=device,
                                   **case["overlay"])
    _same(got, (y, u, v) if layout == "i420" else (y, ref.nv12(u, v)))
    del keep
    # the panels show something: no cell equals another, and the overlay reached the panels that asked for it
    luma = [c[0].tobytes() for c in case["cells"]]
    assert len(set(luma)) == len(luma) or H * W <= 4


@pytest.mark.parametrize("H,W", SIZES)
def test_every_label_value(ctx, font, palette, H, W):
    """A labels panel that holds every value 0..255 (as many frames as that takes at this size), beside its own gray picture."""
    F = -(-256 // (H * W))
    plane = (np.arange(F * H * W) % 256).astype(np.uint8).reshape(F, H, W)
    assert set(plane.reshape(-1).tolist()) == set(range(256))
    frames = np.random.default_rng(H + W).integers(0, 256, (F, H, W), dtype=np.uint8)          # a gray source
    overlay = dict(styles=STYLES)
    cells = [tref.render(frames, font=font, **overlay), panel_cell(plane, "labels", 1, 0, None, overlay, font, palette),
             panel_cell(plane, "gray", 1, 0, None, overlay, font, palette)]
    bgr = panel_bgr(plane, "labels", 1, palette)
    assert (bgr[plane == 0] == 0).all() and bgr[plane != 0].any(axis=-1).all()                 # 0 is black, nothing else is
    got = ctx.render_review_panels(frames, panels=[dict(plane=plane, kind="labels", gain=0), dict(plane=plane)], cols=3, **overlay)
    _same(got, paste(cells, H, W, 3))


# ------------------------------------------------------------------------------------------ 2. no panels: the labels call
@pytest.mark.parametrize("H,W", [(2, 2), (6, 8), (16, 64)])
def test_no_panels_is_render_review_with_labels(ctx, H, W):
    """npanels == 0, cols == 1 at even sizes: byte for byte what swk_render_review_labels writes, into a destination of the same
    strides (wider than the rows: the bytes between the rows stay as they were in both)."""
    from swiftwatcher_amd import _lib
    F = 3
    frames = np.random.default_rng(H + W).integers(0, 256, (F, H, W, 3), dtype=np.uint8)
    overlay = _overlay(F, H, W)
    labels = [(f, 0, 1, 7, 6, 1, "F%d" % f) for f in range(F)]
    for layout in ("i420", "nv12"):
        backs = []
        for call in (ctx.render_review_panels, ctx.render_review):
            dst, back = _dst(_lib, F, H, W, layout)
            call(frames, labels=labels, dst=dst, **overlay)
            backs.append(back)
        assert all(np.array_equal(a, b) for a, b in zip(*backs))
        assert not (backs[0][0] == 0xA5).all() and (backs[0][0][:, H:] == 0xA5).all() and (backs[0][0][:, :, W:] == 0xA5).all()
    _same(ctx.render_review_panels(frames, **overlay), ctx.render_review(frames, **overlay))          # (and without labels: swk_render_review)


# ------------------------------------------------------------------------------------------ 3. fill
def _dst(_lib, F, Hd, Wd, layout="i420", mem=None):
    """A host destination of Hd x Wd frames with strides above the rows, pre-filled with 0xA5: (Yuv420Dst, [y, u, v] backing arrays)."""
    hc, wc = (Hd + 1) // 2, (Wd + 1) // 2
    cb = 1 if layout == "i420" else 2
    back = [np.full(s, 0xA5, np.uint8) for s in [(F, Hd + 1, Wd + 3), (F, hc + 1, wc * cb + 5), (F, hc + 1, wc * cb + 5)]]
    dst = _lib.Yuv420Dst(y=back[0].ctypes.data, u=back[1].ctypes.data, v=back[2].ctypes.data if layout == "i420" else None, mem=_lib.MEM_HOST,
                         layout=_lib.YUV_I420 if layout == "i420" else _lib.YUV_NV12, y_row_stride=Wd + 3, y_frame_stride=(Hd + 1) * (Wd + 3),
                         c_row_stride=wc * cb + 5, c_frame_stride=(hc + 1) * (wc * cb + 5))
    return dst, back


@pytest.mark.parametrize("layout", ["i420", "nv12"])
def test_fill_and_bytes_outside_the_mosaic(ctx, font, palette, layout):
    """7 x 13 with two panels in two columns: pad row and column in every cell (cell 0's too) and the empty fourth cell are Y = 16,
    U = V = 128; the destination's bytes outside the 16 x 28 mosaic stay as they were."""
    from swiftwatcher_amd import _lib
    H, W, F = 7, 13, 2
    case = _case(H, W, 5, font, palette)
    frames, planes = case["frames"][:F], [p[:F] for p in case["planes"][:2]]
    overlay = _overlay(F, H, W)
    cells = [tref.render(frames[:, 1:1 + H, 2:2 + W], font=font, **overlay)]
    cells += [panel_cell(p, "gray", g, 15, None, overlay, font, palette) for p, g in zip(planes, (1, 4))]
    y, u, v = paste(cells, H, W, 2)
    assert y.shape == (F, 16, 28)
    dst, back = _dst(_lib, F, 16, 28, layout)
    ctx.render_review_panels(frames, panels=[dict(plane=planes[0], layers=15), dict(plane=planes[1], gain=4, layers=15)], cols=2, rect=case["rect"], dst=dst,
                             **overlay)
    assert np.array_equal(back[0][:, :16, :28], y)
    if layout == "i420":
        assert np.array_equal(back[1][:, :8, :14], u) and np.array_equal(back[2][:, :8, :14], v)
        assert (back[1][:, 8:] == 0xA5).all() and (back[1][:, :, 14:] == 0xA5).all() and (back[2][:, 8:] == 0xA5).all() and (back[2][:, :, 14:] == 0xA5).all()
    else:
        assert np.array_equal(back[1][:, :8, :28].reshape(F, 8, 14, 2), ref.nv12(u, v))
        assert (back[1][:, 8:] == 0xA5).all() and (back[1][:, :, 28:] == 0xA5).all() and (back[2] == 0xA5).all()
    assert (back[0][:, 16:] == 0xA5).all() and (back[0][:, :, 28:] == 0xA5).all()
    # what the fill is, spelled out: pads of the three cells, the whole fourth cell
    got_y = back[0][:, :16, :28]
    assert (got_y[:, 7] == 16).all() and (got_y[:, 15] == 16).all() and (got_y[:, :, 13] == 16).all() and (got_y[:, :, 27] == 16).all()
    assert (got_y[:, 8:, 14:] == 16).all() and (u[:, 4:, 7:] == 128).all() and (v[:, 4:, 7:] == 128).all()
    assert not (got_y[:, :7, :13] == 16).all()


# ------------------------------------------------------------------------------------------ 4. refusals
def test_refusals_leave_the_destination_untouched(ctx, font):
    """Every refusal of the header's list for panels: SWK_ERR_ARG (-1) or SWK_ERR_CAPACITY (-4), the destination as it was, the
    context usable afterwards."""
    from swiftwatcher_amd import _lib
    lib = _lib.load()
    H, W, F = 6, 8, 2
    frames = np.random.default_rng(3).integers(0, 256, (F, H, W, 3), dtype=np.uint8)
    plane = np.random.default_rng(4).integers(0, 256, (F, H, W), dtype=np.uint8)
    styles = np.zeros(2, _lib.REVIEW_STYLE_DTYPE)
    styles["fill_alpha"], styles["line_alpha"] = 100, 200
    inp = _lib.Input(frames=frames.ctypes.data, mem=_lib.MEM_HOST, channels=3, nwin=1, n=F, Hc=H, Wc=W, x0=0, y0=0, frame_stride=frames.strides[0],
                     row_stride=frames.strides[1])
    rv = _lib.Review(mask=None, mask_style=0, boxes=None, nboxes=0, marks=None, nmarks=0, mark_arm=2, frame_style=None, border=1,
                     styles=styles.ctypes.data, nstyles=2)

    def call(npanels=2, cols=2, null_panels=False, null_rv=False, narrow=None, caption=None, which=1, **change):
        """The call with fifteen good panels (even ones gray, odd ones labels) and panel `which` or its caption changed."""
        panels = (_lib.ReviewPanel * 15)()
        for k in range(15):
            p = panels[k]
            p.plane, p.mem, p.kind, p.frame_stride, p.row_stride, p.gain, p.layers = plane.ctypes.data, _lib.MEM_HOST, k % 2, H * W, W, 3, 5
            rec = _lib.label_records([(0, 1, 1, 1, 2, 1, "AB")])
            ctypes.memmove(ctypes.addressof(p.caption), rec.ctypes.data, 64)
        for name, value in change.items():
            setattr(panels[which], name, value)
        for name, value in (caption or {}).items():
            if name == "text":
                ctypes.memmove(ctypes.addressof(panels[which].caption.text), value, len(value))
            else:
                setattr(panels[which].caption, name, value)
        cells = 1 + max(0, min(npanels, 15))
        c = max(1, min(cols, 16))
        dst, back = _dst(_lib, F, -(-cells // c) * H, c * W)
        if narrow == "y":
            dst.y_row_stride = c * W - 1
        if narrow == "c":
            dst.c_row_stride = c * W // 2 - 1
        rc = lib.swk_render_review_panels(ctx._h, ctypes.byref(inp), None if null_rv else ctypes.byref(rv), None, 0, None if null_panels else panels,
                                          npanels, cols, ctypes.byref(dst))
        return rc, all((b == 0xA5).all() for b in back)

    assert call() == (0, False)                                                       # the unchanged call draws
    assert call(npanels=0, cols=1) == (0, False) and call(npanels=0, cols=1, null_panels=True) == (0, False)
    assert call(npanels=15, cols=16) == (0, False) and call(which=0, gain=255) == (0, False) and call(layers=0) == (0, False)
    assert call(caption=dict(len=0)) == (0, False)
    assert call(which=1, gain=0) == (0, False) and call(which=1, gain=256) == (0, False)          # a labels panel ignores its gain
    refused = [dict(npanels=-1), dict(npanels=16), dict(cols=0), dict(cols=-1), dict(cols=17), dict(null_panels=True), dict(null_rv=True),
               dict(plane=None), dict(kind=2), dict(kind=-1), dict(mem=2), dict(mem=-1), dict(which=0, gain=0), dict(which=0, gain=256),
               dict(which=0, gain=-4), dict(which=0, plane=None), dict(which=0, row_stride=W - 1),
               dict(row_stride=W - 1), dict(row_stride=0), dict(row_stride=-W), dict(layers=16), dict(layers=-1),
               dict(caption=dict(scale=0)), dict(caption=dict(scale=9)), dict(caption=dict(len=33)), dict(caption=dict(len=-1)),
               dict(caption=dict(style=3)), dict(caption=dict(style=-1)), dict(caption=dict(plate=3)), dict(caption=dict(plate=-1)),
               dict(caption=dict(text=b"a")), dict(caption=dict(text=b"A!")), dict(caption=dict(text=b"\xc1")),
               dict(narrow="y"), dict(narrow="c")]
    for change in refused:
        assert call(**dict(change)) == (ARG, True), change
    assert ctx._lib.swk_last_error(ctx._h)
    assert call(caption=dict(frame=99)) == (0, False) and call(caption=dict(frame=-5)) == (0, False)          # a caption's frame is ignored
    # a mosaic side above 32768: 2 x 4096 cells, sixteen columns
    wide = np.zeros((1, 2, 4096, 3), np.uint8)
    wplane = np.zeros((1, 2, 4096), np.uint8)
    winp = _lib.Input(frames=wide.ctypes.data, mem=_lib.MEM_HOST, channels=3, nwin=1, n=1, Hc=2, Wc=4096, x0=0, y0=0, frame_stride=wide.strides[0],
                      row_stride=wide.strides[1])
    panels = (_lib.ReviewPanel * 15)()
    for p in panels:
        p.plane, p.mem, p.kind, p.frame_stride, p.row_stride, p.gain = wplane.ctypes.data, _lib.MEM_HOST, 0, 2 * 4096, 4096, 1
        p.caption.scale = 1                                                          # (no caption: len 0 at a valid scale)
    for npanels, cols, want in ((8, 9, CAPACITY), (15, 16, CAPACITY), (7, 8, 0)):
        dst, back = _dst(_lib, 1, 2, cols * 4096)
        rc = lib.swk_render_review_panels(ctx._h, ctypes.byref(winp), ctypes.byref(rv), None, 0, panels, npanels, cols, ctypes.byref(dst))
        assert rc == want and all((b == 0xA5).all() for b in back) == (want != 0)
    tall = np.zeros((1, 4096, 2, 3), np.uint8)
    tplane = np.zeros((1, 4096, 2), np.uint8)
    tinp = _lib.Input(frames=tall.ctypes.data, mem=_lib.MEM_HOST, channels=3, nwin=1, n=1, Hc=4096, Wc=2, x0=0, y0=0, frame_stride=tall.strides[0],
                      row_stride=tall.strides[1])
    for p in panels:
        p.plane, p.frame_stride, p.row_stride = tplane.ctypes.data, 2 * 4096, 2
    dst, back = _dst(_lib, 1, 9 * 4096, 2)
    assert lib.swk_render_review_panels(ctx._h, ctypes.byref(tinp), ctypes.byref(rv), None, 0, panels, 8, 1, ctypes.byref(dst)) == CAPACITY
    assert all((b == 0xA5).all() for b in back)
    # the context still renders
    _same(ctx.render_review_panels(frames, panels=[dict(plane=plane)], cols=2, styles=STYLES),
          paste([ref.yuv420(frames), ref.yuv420(np.repeat(plane[..., None], 3, axis=-1))], H, W, 2))
