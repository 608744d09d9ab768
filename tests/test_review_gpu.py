"""The review video on the MI355X: swk_bgr_to_yuv420 and swk_render_review bit for bit against tests/review_ref.py (the definition's
scalar formulas over int64 arrays), and pipeline's review= / --review: the written file, frame by frame, against the same
restatement applied to the crop with the boxes, marks, borders and mask that ReviewWriter documents."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import review_ref as ref
from test_yuv_gpu import CROP, CROP_ODD, _event_records

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CORNERS = ((40, 71), (116, 71))          # the top edge of the clip's chimney (tests/test_y4m_stream_gpu.py)


@pytest.fixture(scope="module")
def ctx():
    from swiftwatcher_amd import _lib
    return _lib.default_context(0)


def _same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        g = g.cpu().numpy() if hasattr(g, "cpu") else g
        assert g.dtype == np.uint8 and g.shape == w.shape and np.array_equal(g, w)


# ------------------------------------------------------------------------------------------ 1. the conversion
def test_every_triple(ctx):
    """64 frames of 512 x 512 holding every (B, G, R) exactly once (the pattern of test_yuv_gpu.test_every_triple): frame f, 2 x 2 cell
    (i, j) carries G = i, R = j and the four B values 4 f .. 4 f + 3.  Chroma comes from the cell's top-left pixel (B = 4 f)."""
    i, j = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    bgr = np.empty((64, 512, 512, 3), np.uint8)
    bgr[..., 1] = np.repeat(np.repeat(i, 2, 0), 2, 1)[None]
    bgr[..., 2] = np.repeat(np.repeat(j, 2, 0), 2, 1)[None]
    for dr in (0, 1):
        for dc in (0, 1):
            bgr[:, dr::2, dc::2, 0] = (4 * np.arange(64) + 2 * dr + dc).astype(np.uint8)[:, None, None]
    key = (bgr[..., 0].astype(np.int64) << 16) | (bgr[..., 1].astype(np.int64) << 8) | bgr[..., 2]
    assert np.array_equal(np.sort(key.ravel()), np.arange(1 << 24))
    y, u, v = ref.yuv420(bgr)
    _same(ctx.bgr_to_yuv420(bgr), (y, u, v))
    _same(ctx.bgr_to_yuv420(bgr, layout="nv12"), (y, ref.nv12(u, v)))


def _rects(H, W):
    """Rectangles of every origin parity with both parities of Hr / Wr, inside an (H + 5) x (W + 6) frame, and the whole frame."""
    out = [(0, 0, W + 6, H + 5)]
    for px in (0, 1):
        for py in (0, 1):
            out.append((2 + px, 2 + py, W, H))
            out.append((2 + px, 2 + py, max(W - 1, 1), max(H - 1, 1)))
    return out


@pytest.mark.parametrize("H,W", [(2, 2), (3, 5), (16, 64), (47, 94), (67, 131)])
def test_geometry_layouts_and_sources(ctx, H, W):
    import torch
    rng = np.random.default_rng(H * 1000 + W)
    frames = rng.integers(0, 256, (3, H + 5, W + 6, 3), dtype=np.uint8)
    gray = np.ascontiguousarray(frames[..., 1])
    dev = torch.from_numpy(frames).cuda()
    for rect in _rects(H, W):
        x0, y0, Wr, Hr = rect
        y, u, v = ref.yuv420(frames[:, y0:y0 + Hr, x0:x0 + Wr])
        _same(ctx.bgr_to_yuv420(frames, rect=rect), (y, u, v))
        _same(ctx.bgr_to_yuv420(frames, rect=rect, layout="nv12"), (y, ref.nv12(u, v)))
        _same(ctx.bgr_to_yuv420(dev, rect=rect, device_out=True), (y, u, v))
        _same(ctx.bgr_to_yuv420(dev, rect=rect, layout="nv12", device_out=True), (y, ref.nv12(u, v)))
        # gray input is B = G = R; a negative frame stride reads the frames backwards
        _same(ctx.bgr_to_yuv420(gray, rect=rect), ref.yuv420(gray[:, y0:y0 + Hr, x0:x0 + Wr]))
        _same(ctx.bgr_to_yuv420(frames[::-1], rect=rect), (y[::-1], u[::-1], v[::-1]))


def _strided_dst(_lib, F, Hr, Wr, layout, device, pad=(3, 5)):
    """A destination whose row strides exceed the rows and whose frames lie apart: (Yuv420Dst, backing arrays, views of the planes)."""
    import torch
    hc, wc = (Hr + 1) // 2, (Wr + 1) // 2
    cbytes = 1 if layout == "i420" else 2
    shapes = [(F, Hr + 1, Wr + pad[0])] + [(F, hc + 1, wc * cbytes + pad[1])] * (2 if layout == "i420" else 1)
    if device:
        back = [torch.full(s, 0xA5, dtype=torch.uint8, device="cuda:0") for s in shapes]
        ptrs = [b.data_ptr() for b in back]
    else:
        back = [np.full(s, 0xA5, np.uint8) for s in shapes]
        ptrs = [b.ctypes.data for b in back]
    dst = _lib.Yuv420Dst(y=ptrs[0], u=ptrs[1], v=ptrs[2] if layout == "i420" else None,
                         mem=_lib.MEM_DEVICE if device else _lib.MEM_HOST, layout=_lib.YUV_I420 if layout == "i420" else _lib.YUV_NV12,
                         y_row_stride=shapes[0][2], y_frame_stride=shapes[0][1] * shapes[0][2],
                         c_row_stride=shapes[1][2], c_frame_stride=shapes[1][1] * shapes[1][2])
    return dst, back


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("layout", ["i420", "nv12"])
def test_destination_strides(ctx, layout, device):
    from swiftwatcher_amd import _lib
    rng = np.random.default_rng(5)
    frames = rng.integers(0, 256, (4, 47, 94, 3), dtype=np.uint8)
    rect = (1, 2, 91, 43)
    y, u, v = ref.yuv420(frames[:, 2:45, 1:92])
    want = (y, u, v) if layout == "i420" else (y, ref.nv12(u, v).reshape(4, 22, 92))
    dst, back = _strided_dst(_lib, 4, 43, 91, layout, device)
    assert ctx.bgr_to_yuv420(frames, rect=rect, dst=dst) is None
    for b, w in zip(back, want):
        b = b.cpu().numpy() if device else b
        assert np.array_equal(b[:, :w.shape[1], :w.shape[2]], w)
        untouched = b.copy()
        untouched[:, :w.shape[1], :w.shape[2]] = 0xA5
        assert (untouched == 0xA5).all(), "bytes outside the planes' rows were written"


# ------------------------------------------------------------------------------------------ 2. the overlay
STYLES = [(0, 255, 0, 48, 256), (0, 0, 255, 128, 255), (0, 255, 255, 1, 200), (255, 128, 0, 40, 0), (10, 20, 30, 0, 1), (255, 255, 255, 256, 128),
          (90, 0, 200, 255, 256)]
H47, W94 = 47, 94


def _overlay(F, seed):
    """Per frame one of the cases of the issue's list (frame k takes case k % 12); 300 boxes in frame 5 (three LDS chunks)."""
    rng = np.random.default_rng(seed)
    boxes, marks = [], []
    for f in range(F):
        case = f % 12
        if case == 1:
            boxes.append((f, 5, 7, 20, 31, 1))
        elif case == 2:                                  # overlapping boxes of different styles
            boxes += [(f, 4, 4, 30, 50, 1), (f, 10, 20, 40, 70, 2), (f, 12, 22, 28, 48, 3)]
        elif case == 3:                                  # partly and wholly outside
            boxes += [(f, -5, -7, 9, 12, 2), (f, 40, 80, 60, 120, 1), (f, -20, -20, -3, -1, 6), (f, 47, 94, 60, 100, 6), (f, -3, -3, 50, 97, 7)]
        elif case == 4:                                  # 1 x 1, 2 x 2 and empty boxes, at both pixel parities
            boxes += [(f, 3, 3, 4, 4, 6), (f, 4, 8, 5, 9, 6), (f, 9, 9, 11, 11, 7), (f, 20, 30, 22, 32, 7), (f, 30, 30, 30, 40, 6),
                      (f, 31, 31, 35, 31, 6), (f, 40, 40, 38, 38, 6), (f, 46, 93, 47, 94, 2)]
        elif case == 5:                                  # 300 boxes
            r0, c0 = rng.integers(-6, H47, 300), rng.integers(-6, W94, 300)
            boxes += [(f, int(a), int(b), int(a + h), int(b + w), int(s)) for a, b, h, w, s in
                      zip(r0, c0, rng.integers(0, 14, 300), rng.integers(0, 22, 300), rng.integers(0, len(STYLES) + 1, 300))]
        elif case == 6:                                  # marks at the four corners and outside the frame
            marks += [(f, 0, 0, 3), (f, 0, W94 - 1, 2), (f, H47 - 1, 0, 1), (f, H47 - 1, W94 - 1, 7), (f, -2, 40, 3), (f, 20, W94 + 1, 2),
                      (f, -50, -50, 1), (f, 23, 47, 6), (f, 24, 48, 5), (f, 23, 47, 0)]
        elif case == 7:                                  # boxes and marks on one frame
            boxes += [(f, 10, 10, 30, 60, 3)]
            marks += [(f, 20, 35, 2), (f, 10, 10, 1)]
        elif case == 8:
            boxes += [(f, 0, 0, H47, W94, 4), (f, 1, 1, H47 - 1, W94 - 1, 5)]
        elif case == 9:
            marks += [(f, int(r), int(c), int(s)) for r, c, s in zip(rng.integers(-3, H47 + 3, 150), rng.integers(-3, W94 + 3, 150),
                                                                     rng.integers(0, len(STYLES) + 1, 150))]
    return boxes, marks


def _mask_checker():
    rr, cc = np.mgrid[0:H47, 0:W94]
    return (((rr + cc) & 1) * 255).astype(np.uint8)


@pytest.fixture(scope="module")
def scene():
    rng = np.random.default_rng(77)
    return rng.integers(0, 256, (43, H47 + 4, W94 + 3, 3), dtype=np.uint8)


@pytest.mark.parametrize("F", [1, 43])
@pytest.mark.parametrize("arm,border", [(0, 0), (3, 1), (200, 30)])
def test_overlay(ctx, scene, F, arm, border):
    """43 frames = two windows and one frame: a grid of many frames.  mark_arm 0 / larger than the frame; border 0, 1 and larger than
    half the frame (every pixel).  The checkerboard mask alternates at every pixel, so chroma (even pixels only) and luma disagree
    about it wherever the kernel samples anything but pixel (2 i, 2 j)."""
    import torch
    frames = scene[:F] if F > 1 else scene[5:6]
    boxes, marks = _overlay(F, 3) if F > 1 else ([(0,) + b[1:] for b in _overlay(12, 3)[0] if b[0] in (2, 3, 4, 5)],
                                                  [(0,) + m[1:] for m in _overlay(12, 3)[1] if m[0] == 6])
    frame_style = np.array([(k * 5) % (len(STYLES) + 1) for k in range(F)], np.int32) if F > 1 else np.array([2], np.int32)
    rect = (2, 3, W94, H47)
    kw = dict(boxes=boxes, marks=marks, frame_style=frame_style, mask=_mask_checker(), styles=STYLES, mask_style=4, mark_arm=arm, border=border)
    y, u, v = ref.render(frames[:, 3:3 + H47, 2:2 + W94], **kw)
    plain = ref.yuv420(frames[:, 3:3 + H47, 2:2 + W94])
    assert not np.array_equal(y, plain[0]) and not np.array_equal(u, plain[1])
    _same(ctx.render_review(frames, rect=rect, **kw), (y, u, v))
    _same(ctx.render_review(torch.from_numpy(frames).cuda(), rect=rect, layout="nv12", device_out=True, **kw), (y, ref.nv12(u, v)))
    _same(ctx.render_review(np.ascontiguousarray(frames[..., 2]), rect=rect, **kw), ref.render(frames[:, 3:3 + H47, 2:2 + W94, 2], **kw))


@pytest.mark.parametrize("fill,line", [(0, 0), (1, 255), (128, 128), (255, 1), (256, 256), (0, 256), (256, 0)])
def test_alphas(ctx, scene, fill, line):
    styles = [(12, 200, 77, fill, line)]
    kw = dict(boxes=[(0, 3, 4, 30, 60, 1), (1, -2, -2, 20, 20, 1)], marks=[(0, 35, 70, 1), (1, 5, 5, 1)], frame_style=[1, 0], mask=_mask_checker(),
              styles=styles, mask_style=1, mark_arm=4, border=2)
    frames = scene[:2, :H47, :W94]
    _same(ctx.render_review(frames, **kw), ref.render(frames, **kw))
    if fill == 0 and line == 0:
        _same(ctx.render_review(frames, **kw), ref.yuv420(frames))


def test_box_order_matters(ctx, scene):
    """The blends do not commute: two overlapping boxes with 0 < alpha < 256 in both orders."""
    frames = scene[:1, :H47, :W94]
    a, b = (0, 5, 5, 30, 50, 1), (0, 15, 25, 40, 80, 2)
    kw = dict(styles=STYLES)
    ab, ba = ctx.render_review(frames, boxes=[a, b], **kw), ctx.render_review(frames, boxes=[b, a], **kw)
    assert not np.array_equal(ab[0], ba[0])
    _same(ab, ref.render(frames, boxes=[a, b], **kw))
    _same(ba, ref.render(frames, boxes=[b, a], **kw))


def test_no_overlay_is_the_conversion(ctx, scene):
    frames = scene[:3, :H47, :W94]
    _same(ctx.render_review(frames, styles=STYLES, mask=np.zeros((H47, W94), np.uint8), mask_style=4, frame_style=[0, 0, 0], border=3),
          ctx.bgr_to_yuv420(frames))


def test_refusals_leave_the_destination_untouched(ctx, scene):
    """Every refusal of the header: SWK_ERR_ARG (-1) before anything is launched, the destination as it was, the context usable."""
    from swiftwatcher_amd import _lib
    lib = _lib.load()
    frames = np.ascontiguousarray(scene[:2, :H47, :W94])
    styles = np.zeros(2, _lib.REVIEW_STYLE_DTYPE)
    styles["fill_alpha"], styles["line_alpha"] = 100, 200
    keep = []

    def call(render=True, **change):
        dst, back = _strided_dst(_lib, 2, H47, W94, change.pop("layout", "i420"), False)
        inp = _lib.Input(frames=frames.ctypes.data, mem=_lib.MEM_HOST, channels=3, nwin=1, n=2, Hc=H47, Wc=W94, x0=0, y0=0,
                         frame_stride=frames.strides[0], row_stride=frames.strides[1])
        boxes = np.zeros(2, _lib.REVIEW_BOX_DTYPE)
        boxes["frame"], boxes["r1"], boxes["c1"], boxes["style"] = [0, 1], 9, 9, 1
        marks = np.zeros(2, _lib.REVIEW_MARK_DTYPE)
        marks["frame"], marks["style"] = [0, 1], 2
        fs = np.array([1, 2], np.int32)
        st = styles.copy()
        rv = _lib.Review(mask=None, mask_style=0, boxes=boxes.ctypes.data, nboxes=2, marks=marks.ctypes.data, nmarks=2, mark_arm=2,
                         frame_style=fs.ctypes.data, border=1, styles=st.ctypes.data, nstyles=2)
        keep.append((boxes, marks, fs, st))
        for name, value in change.items():
            where, field = name.split("__")
            if where in ("boxes", "marks", "fs", "st"):
                target = {"boxes": boxes, "marks": marks, "fs": fs, "st": st}[where]
                if where == "fs":
                    target[:] = value
                else:
                    target[field] = value
            else:
                setattr({"dst": dst, "inp": inp, "rv": rv}[where], field, value)
        if render:
            rc = lib.swk_render_review(ctx._h, ctypes.byref(inp), ctypes.byref(rv), ctypes.byref(dst))
        else:
            rc = lib.swk_bgr_to_yuv420(ctx._h, ctypes.byref(inp), ctypes.byref(dst))
        return rc, all((b == 0xA5).all() for b in back)

    assert call() == (0, False) and call(render=False) == (0, False)          # the unchanged call draws
    refused = [dict(dst__y=None), dict(dst__u=None), dict(dst__v=None), dict(layout="nv12", dst__u=None),
               dict(dst__y_row_stride=W94 - 1), dict(dst__c_row_stride=W94 // 2 - 1), dict(layout="nv12", dst__c_row_stride=W94 - 1),
               dict(dst__layout=2), dict(dst__layout=-1), dict(inp__channels=2), dict(inp__channels=4), dict(inp__channels=0)]
    for change in refused:
        for render in (True, False):
            assert call(render=render, **dict(change)) == (-1, True), (change, render)
    refused = [dict(st__fill_alpha=[0, 257]), dict(st__line_alpha=[-1, 0]), dict(st__fill_alpha=[300, 0]),
               dict(boxes__style=[3, 0]), dict(boxes__style=[0, -1]), dict(marks__style=[0, 3]), dict(fs__=[0, 3]), dict(fs__=[-1, 0]),
               dict(rv__mask_style=3), dict(rv__mask_style=-1),
               dict(boxes__frame=[0, 2]), dict(boxes__frame=[-1, 0]), dict(marks__frame=[0, 2]), dict(marks__frame=[-1, 1]),
               dict(boxes__frame=[1, 0]), dict(marks__frame=[1, 0]), dict(rv__mark_arm=-1), dict(rv__border=-1)]
    for change in refused:
        assert call(**dict(change)) == (-1, True), change
    assert ctx._lib.swk_last_error(ctx._h)
    _same(ctx.bgr_to_yuv420(frames), ref.yuv420(frames))


# ------------------------------------------------------------------------------------------ 3. the counting loops write the review
EVENT_HOLD, MARK_ARM, BORDER = 15, 4, 3          # ReviewWriter's documented defaults
PALETTE = [(0, 255, 0, 32, 256), (0, 0, 255, 0, 160), (0, 255, 255, 0, 256), (255, 128, 0, 40, 0)]          # its documented palette


def _roi_mask():
    m = np.zeros((64, 96), np.uint8)
    m[28:, :] = 255
    return m


@pytest.fixture(scope="module")
def clip(tmp_path_factory):
    """tests/test_y4m_stream_gpu.py's seeded 52-frame 110 x 160 clip: BGR frames, and an 8-bit 4:2:0 file of them."""
    import yuv_ref
    from swiftwatcher_amd import synthetic
    from swiftwatcher_amd.io_y4m import Y4MWriter
    bgr = synthetic.full_frames(500, 52, CROP, frame_hw=(110, 160), birds=4, bird_len=(8, 12), bird_wid=(3, 5))[::-1].copy()
    folder = tmp_path_factory.mktemp("review_gpu")
    y, u, v = yuv_ref.bgr_to_yuv420(bgr)
    paths = {}
    for name, count in (("y4m", 52), ("y4m_23", 23)):
        paths[name] = str(folder / (name + ".y4m"))
        with Y4MWriter(paths[name], 160, 110, 30) as w:
            for k in range(count):
                w.append(y[k], u[k], v[k])
    return dict(bgr=bgr, folder=folder, **paths)


class _Recorder:
    """Stands in for a ReviewWriter: keeps what the loop hands over."""

    def __init__(self):
        self.windows = []

    def write_window(self, popped, rejected=None, new_events=()):
        self.windows.append((list(popped), [list(r or ()) for r in (rejected if rejected is not None else [None] * len(popped))],
                             [list(ev) for ev in new_events]))


def _expected(recorder, crop, roi_mask):
    """The frames ReviewWriter documents for what the loop handed over, by the test-side restatement: (y, u, v) stacks."""
    (x0, y0), (x1, y1) = crop
    frames, boxes, events = [], [], []
    for popped, rejected, new_events in recorder.windows:
        for ev in new_events:
            first = ev[-1].parent_frame_number + 1
            events.append((first, [(int(np.floor(s.centroid[0] + 0.5)), int(np.floor(s.centroid[1] + 0.5))) for s in ev]))
        for fr, gone in zip(popped, rejected):
            if fr.frame_number < 0:
                continue
            frames.append(fr)
            boxes.append([tuple(s.bbox) + (1,) for s in fr.segments] + [tuple(b) + (2,) for b in gone])
    crops = np.stack([np.asarray(fr.frame)[y0:y1, x0:x1] for fr in frames])
    all_boxes = [(k,) + b for k, per in enumerate(boxes) for b in per]
    marks, frame_style = [], []
    for k, fr in enumerate(frames):
        shown = [pts for first, pts in events if first <= fr.frame_number < first + EVENT_HOLD]
        frame_style.append(3 if shown else 0)
        marks += [(k, r, c, 3) for pts in shown for r, c in pts]
    want = ref.render(crops, boxes=all_boxes, marks=marks, frame_style=frame_style, mask=roi_mask, styles=PALETTE, mask_style=4,
                      mark_arm=MARK_ARM, border=BORDER)
    return want, dict(frames=len(frames), boxes=len(all_boxes), rejected=sum(len(g) for _, rej, _ in recorder.windows for g in rej),
                      marks=len(marks), bordered=int(np.count_nonzero(frame_style)), plain=ref.yuv420(crops))


def _read_review(path, crop):
    from swiftwatcher_amd.io_y4m import open_y4m
    reader = open_y4m(path)
    (x0, y0), (x1, y1) = crop
    assert tuple(reader.frame_shape[:2]) == (y1 - y0, x1 - x0)
    frames = [reader.frames[k] for k in range(reader.total_frames)]
    got = tuple(np.stack([np.asarray(getattr(f, p)) for f in frames]) for p in "yuv")
    if hasattr(reader, "close"):
        reader.close()
    return got


def _check_run(run, crop, roi_mask, path):
    """run(review) -> (count, events): with a recorder, with the path, and with no review: equal counts and events, and the file holds
    what ReviewWriter documents for the recorded hand-over."""
    recorder = _Recorder()
    recorded = run(recorder)
    plain = run(None)
    written = run(path)
    assert len(plain[1]) >= 1, "no event: equality would be vacuous"
    for got in (recorded, written):
        assert got[0] == plain[0] and _event_records(got[1]) == _event_records(plain[1])
    assert sum(len(ev) for _, _, ev in recorder.windows) == len(plain[1])
    want, info = _expected(recorder, crop, roi_mask)
    got = _read_review(path, crop)
    print(path, info["frames"], "frames,", info["boxes"], "boxes,", info["rejected"], "rejected,", info["marks"], "marks,", info["bordered"], "bordered")
    assert got[0].shape[0] == info["frames"] >= 52 and info["boxes"] > 0 and info["marks"] > 0 and 0 < info["bordered"] < info["frames"]
    _same(got, want)
    assert not np.array_equal(got[0], info["plain"][0])
    return recorder, info


def test_review_of_a_bgr_array(clip):
    from swiftwatcher_amd import pipeline
    path = str(clip["folder"] / "bgr_review.y4m")
    _check_run(lambda rv: pipeline.count_swifts(clip["bgr"], crop_region=CROP, roi_mask=_roi_mask(), review=rv), CROP, _roi_mask(), path)


@pytest.mark.parametrize("wpc", [1, 2])
def test_review_of_a_y4m_file(clip, wpc):
    """4:2:0 frames (converted to a device BGR stack for the review as for the count), an odd crop origin, one and two windows per call."""
    from swiftwatcher_amd import pipeline
    path = str(clip["folder"] / ("y4m_review_%d.y4m" % wpc))
    _check_run(lambda rv: pipeline.count_swifts(clip["y4m"], crop_region=CROP_ODD, roi_mask=_roi_mask(), windows_per_call=wpc, review=rv),
               CROP_ODD, _roi_mask(), path)


def test_review_through_count_swifts_videos(clip):
    """Two videos of different crop regions in one groups call; the first gets a review, the second none."""
    from swiftwatcher_amd import pipeline
    path = str(clip["folder"] / "videos_review.y4m")
    small = [(40, 30), (40 + 64, 30 + 48)]
    mask2 = np.zeros((48, 64), np.uint8)
    mask2[20:, :] = 255
    regions = [(CROP, _roi_mask()), (small, mask2)]
    seen = []

    def run(rv):
        out = pipeline.count_swifts_videos([clip["bgr"], clip["y4m"]], regions=regions, reviews=None if rv is None else [rv, None])
        seen.append(out[1])
        return out[0]
    _check_run(run, CROP, _roi_mask(), path)
    assert all(o[0] == seen[0][0] and _event_records(o[1]) == _event_records(seen[0][1]) for o in seen[1:])          # the other video's count
    with pytest.raises(ValueError):
        pipeline.count_swifts_videos([clip["bgr"]], regions=regions[:1], reviews=[None, None])


class _RejectFirst:
    """A classifier's surface for the loops: removes the segment with the smallest label from every frame that has two or more, and
    relabels the kept ones 1..k (as SegmentClassifier does)."""

    def __call__(self, segments):
        kept = list(segments[1:]) if len(segments) >= 2 else list(segments)
        for j, s in enumerate(kept):
            s.label = j + 1
        return kept

    def classify_frames(self, frames):
        for fr in frames:
            fr.segments = self(fr.segments)


@pytest.mark.parametrize("wpc", [1, 2])
def test_boxes_the_classifier_removed_appear_in_style_2(clip, wpc):
    from swiftwatcher_amd import pipeline
    bare = _Recorder()
    pipeline.count_swifts(clip["bgr"], crop_region=CROP, roi_mask=_roi_mask(), windows_per_call=wpc, review=bare)
    first_boxes = {fr.frame_number: tuple(fr.segments[0].bbox) for popped, _, _ in bare.windows for fr in popped
                   if fr.frame_number >= 0 and len(fr.segments) >= 2}
    assert first_boxes
    path = str(clip["folder"] / ("rejected_review_%d.y4m" % wpc))
    recorder, info = _check_run(lambda rv: pipeline.count_swifts(clip["bgr"], crop_region=CROP, roi_mask=_roi_mask(), windows_per_call=wpc,
                                                                 classifier=_RejectFirst(), review=rv), CROP, _roi_mask(), path)
    removed = {fr.frame_number: [tuple(b) for b in gone] for popped, rejected, _ in recorder.windows for fr, gone in zip(popped, rejected)
               if fr.frame_number >= 0 and gone}
    assert removed == {k: [b] for k, b in first_boxes.items()} and info["rejected"] == len(first_boxes)
    # (_check_run compared the file with the restatement drawing exactly these boxes in style 2, after the kept segments' boxes)


def test_a_frame_with_nothing_drawn_is_the_plain_conversion(clip, ctx):
    """No segment, no event, a zero mask: the written frames are the conversion of the crop; null frames are not written."""
    from swiftwatcher_amd.data_structures import Frame
    from swiftwatcher_amd.review import ReviewWriter
    path = str(clip["folder"] / "plain_review.y4m")
    popped = [Frame(clip["bgr"][k], k, "00:00:00.000") for k in range(3)] + [Frame(np.zeros_like(clip["bgr"][0]), -1)]
    with ReviewWriter(path, CROP_ODD, np.zeros((64, 96), np.uint8), 30) as w:
        w.write_window(popped)
        w.write_window(popped[3:])
        assert w.frames == 3
    (x0, y0), (x1, y1) = CROP_ODD
    want = ref.yuv420(clip["bgr"][:3, y0:y1, x0:x1])
    _same(_read_review(path, CROP_ODD), want)
    _same(ctx.bgr_to_yuv420(clip["bgr"][:3], rect=(x0, y0, x1 - x0, y1 - y0)), want)


def test_y4m_writer_append_bgr(clip, ctx):
    from swiftwatcher_amd.io_y4m import Y4MWriter
    path = str(clip["folder"] / "append_bgr.y4m")
    with Y4MWriter(path, 160, 110, 30) as w:
        w.append_bgr(clip["bgr"][:2], ctx)
        w.append_bgr(clip["bgr"][2])
        assert w.frames == 3
    _same(_read_review(path, [(0, 0), (160, 110)]), ref.yuv420(clip["bgr"][:3]))


def test_cli_writes_the_review(clip):
    """python -m swiftwatcher_amd --review in a fresh child process, on the 23-frame file."""
    out = str(clip["folder"] / "cli_review.y4m")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    p = subprocess.run([sys.executable, "-m", "swiftwatcher_amd", clip["y4m_23"], "--corners", "%d,%d,%d,%d" % (CORNERS[0] + CORNERS[1]),
                        "--review", out], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert p.returncode == 0, p.stdout + p.stderr
    line = json.loads(p.stdout.strip().splitlines()[-1])
    assert line["source"] == clip["y4m_23"] and line["frames"] == 23
    from swiftwatcher_amd import image_filtering as img
    from swiftwatcher_amd.io_y4m import open_y4m
    first = open_y4m(clip["y4m_23"])
    crop, _, _ = img.generate_regions(first.read_frame(0, increment=False), CORNERS)
    first.close() if hasattr(first, "close") else None
    y, u, v = _read_review(out, crop)
    assert y.shape[0] >= 23
