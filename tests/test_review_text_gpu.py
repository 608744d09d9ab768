"""The review video's text on the MI355X: swk_render_review_labels bit for bit, on all three planes, against tests/review_text_ref.py
(the definition's restatement with the library's font table), and pipeline's review_text= / --review-text: the written file, frame
by frame, against the same restatement applied to the status line and event numbers that ReviewWriter documents."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import review_ref as ref
import review_text_ref as tref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CROP = [(30, 20), (30 + 96, 20 + 64)]
CROP_ODD = [(31, 21), (31 + 96, 21 + 64)]
CORNERS = ((40, 71), (116, 71))          # the top edge of the clip's chimney (tests/test_y4m_stream_gpu.py)
CHARSET = tref.CHARSET.decode("ascii")
# (b, g, r, fill_alpha, line_alpha): 1..4 box / mark / border / mask styles, 5 opaque ink, 6 plate, 7 translucent ink and plate
STYLES = [(0, 255, 0, 48, 256), (0, 0, 255, 128, 255), (0, 255, 255, 1, 200), (255, 128, 0, 40, 0), (255, 255, 255, 0, 256), (0, 0, 0, 160, 0),
          (90, 0, 200, 77, 130)]


@pytest.fixture(scope="module")
def ctx():
    from swiftwatcher_amd import _lib
    return _lib.default_context(0)


@pytest.fixture(scope="module")
def font():
    from swiftwatcher_amd import _lib
    return _lib.review_font()


def _same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        g = g.cpu().numpy() if hasattr(g, "cpu") else g
        assert g.dtype == np.uint8 and g.shape == w.shape and np.array_equal(g, w)


def _frames(seed, F, H, W):
    return np.random.default_rng(seed).integers(0, 256, (F, H, W, 3), dtype=np.uint8)


# ------------------------------------------------------------------------------------------ 1. every glyph
@pytest.mark.parametrize("scale", [1, 3])
def test_every_glyph(ctx, font, scale):
    """The whole set in one label row (45 bytes: a label of 32 and one of 13), shifted left by 108 pixels (six cells at scale 3) per frame so that every
    glyph lies inside some frame whole: 45 * 6 * 3 = 810 pixels at scale 3, eight frames of 131."""
    import torch
    from swiftwatcher_amd import _lib
    F, H, W = 8, 31, 131
    frames = _frames(scale, F, H, W)
    labels = []
    for f in range(F):
        c = 2 - 108 * f
        labels += [(f, 4, c, 5, 6, scale, CHARSET[:32]), (f, 4, c + 6 * scale * 32, 7, 6, scale, CHARSET[32:])]
    whole = {k for k in range(45) if any(0 <= 2 - 108 * f + 6 * scale * k and 2 - 108 * f + 6 * scale * (k + 1) <= W for f in range(F))}
    assert whole == set(range(45)) and len(CHARSET) == 45                # every glyph of the set is drawn whole on some frame
    kw = dict(labels=labels, styles=STYLES)
    y, u, v = tref.render(frames, font=font, **kw)
    plain = ref.yuv420(frames)
    assert not np.array_equal(y, plain[0]) and not np.array_equal(u, plain[1]) and not np.array_equal(v, plain[2])
    dev = torch.from_numpy(frames).cuda()
    _same(ctx.render_review(frames, **kw), (y, u, v))                                                     # host source and destination
    _same(ctx.render_review(frames, layout="nv12", **kw), (y, ref.nv12(u, v)))
    _same(ctx.render_review(dev, device_out=True, **kw), (y, u, v))                                       # device source and destination
    _same(ctx.render_review(dev, layout="nv12", device_out=True, **kw), (y, ref.nv12(u, v)))
    gray = np.ascontiguousarray(frames[..., 1])                                                          # a 1-channel source
    _same(ctx.render_review(gray, **kw), tref.render(gray, font=font, **kw))
    _same(ctx.render_review(frames, labels=_lib.label_records(labels), styles=STYLES), (y, u, v))          # REVIEW_LABEL_DTYPE records pass through


# ------------------------------------------------------------------------------------------ 2. geometry
def _geometry_labels(H, W):
    """One frame per case: (labels, the cases' names in frame order)."""
    cases = []
    for r in range(3):                                   # the strip alignment: a strip is 8 x 2 pixels
        for c in range(9):
            cases.append(("sweep", [(r, c, 5, 6, 1, "A1")]))
    long = "0123456789ABCDEFGHIJKLMNOPQRSTUV"
    cases += [("edge", [(-3, 2, 5, 6, 2, "EDGE-08")]), ("edge", [(1, -4, 5, 6, 2, "EDGE-08")]), ("edge", [(H - 4, 1, 5, 6, 2, "EDGE-08")]),
              ("edge", [(1, W - 7, 5, 6, 2, "EDGE-08")]),
              ("negative", [(-5, -9, 5, 6, 2, "N=7")]), ("negative", [(-1, -1, 7, 6, 1, "+/-")]),
              # wholly outside, by one pixel and by far: rows [r - s, r + 8 s), columns [c - s, c + 6 s len)
              ("outside", [(-8, 0, 5, 6, 1, "OUT"), (H + 1, 0, 5, 6, 1, "OUT"), (0, -18, 5, 6, 1, "OUT"), (0, W + 1, 5, 6, 1, "OUT"), (-100, -100, 5, 6, 8, "OUT"),
                           (H + 10, W + 10, 5, 6, 8, "OUT")]),
              # ... and inside by one pixel
              ("inside", [(-7, 0, 5, 6, 1, "IN.")]), ("inside", [(H, 0, 5, 6, 1, "IN.")]), ("inside", [(0, -17, 5, 6, 1, "IN.")]), ("inside", [(0, W, 5, 6, 1, "IN.")]),
              ("len0", [(1, 1, 5, 6, 1, "")]), ("len32", [(1, 1, 5, 6, 1, long)]), ("len32", [(2, -150, 5, 6, 1, long)]),
              ("scale8", [(1, 2, 5, 6, 8, "#8")]), ("scale8", [(-30, -40, 5, 6, 8, "%Z")]),
              # near +-2^31: nothing is drawn, nothing wraps
              ("far", [(2**31 - 1, 2**31 - 1, 5, 6, 8, long), (-2**31, -2**31, 5, 6, 8, long), (2**31 - 1, 0, 5, 6, 8, long), (0, -2**31, 5, 6, 8, long),
                       (-2**31, 5, 5, 6, 1, "A"), (3, 2**31 - 1, 5, 6, 1, "A"), (2**31 - 9, 1, 5, 6, 8, "A"), (1, 2**31 - 1537, 5, 6, 8, long)])]
    labels = [(f,) + lab for f, (_, labs) in enumerate(cases) for lab in labs]
    return labels, [name for name, _ in cases]


@pytest.mark.parametrize("H,W", [(2, 2), (3, 5), (16, 64), (47, 94), (67, 131)])
def test_geometry(ctx, font, H, W):
    import torch
    labels, names = _geometry_labels(H, W)
    F = len(names)
    frames = _frames(H * 1000 + W, F, H + 3, W + 5)
    rect = (2, 1, W, H)
    crop = frames[:, 1:1 + H, 2:2 + W]
    kw = dict(labels=labels, styles=STYLES)
    composed = tref.compose(crop, font=font, **kw)
    y, u, v = ref.yuv420(composed)
    plain = ref.to_bgr3(crop)
    drawn = [not np.array_equal(composed[f], plain[f]) for f in range(F)]
    assert not any(d for d, name in zip(drawn, names) if name in ("outside", "len0", "far"))          # these draw nothing
    assert all(d for d, name in zip(drawn, names) if name in ("inside", "edge", "negative", "scale8"))
    assert sum(d for d, name in zip(drawn, names) if name == "sweep") >= (27 if W >= 16 else 9)
    _same(ctx.render_review(frames, rect=rect, **kw), (y, u, v))
    _same(ctx.render_review(torch.from_numpy(frames).cuda(), rect=rect, layout="nv12", device_out=True, **kw), (y, ref.nv12(u, v)))


# ------------------------------------------------------------------------------------------ 3. layers
H47, W94 = 47, 94


def _mask_checker():
    rr, cc = np.mgrid[0:H47, 0:W94]
    return (((rr + cc) & 1) * 255).astype(np.uint8)


def test_labels_lie_over_the_other_layers(ctx, font):
    """A label over the mask, a box, a mark and the border: layer 5 comes last.  Then two overlapping labels in both orders."""
    frames = _frames(11, 2, H47, W94)
    kw = dict(boxes=[(0, 2, 2, 30, 60, 1), (1, 2, 2, 30, 60, 2)], marks=[(0, 10, 12, 3), (1, 10, 12, 3)], frame_style=[3, 0], mask=_mask_checker(),
              styles=STYLES, mask_style=4, mark_arm=6, border=4)
    labels = [(0, 1, 1, 7, 7, 2, "OVER"), (1, 6, 3, 5, 6, 1, "R01 E007"), (1, 40, 80, 7, 0, 1, "X")]
    want = tref.render(frames, labels=labels, font=font, **kw)
    under = ref.render(frames, **kw)
    assert not np.array_equal(want[0], under[0])
    _same(ctx.render_review(frames, labels=labels, **kw), want)
    # the translucent label shows what lies under it: the same label over the bare frames differs
    assert not np.array_equal(want[0], tref.render(frames, labels=labels, font=font, styles=STYLES)[0])
    a, b = (0, 5, 5, 7, 7, 2, "AB"), (0, 9, 11, 7, 6, 2, "BA")
    ab, ba = ctx.render_review(frames, labels=[a, b], styles=STYLES), ctx.render_review(frames, labels=[b, a], styles=STYLES)
    assert not np.array_equal(ab[0], ba[0])
    _same(ab, tref.render(frames, labels=[a, b], font=font, styles=STYLES))
    _same(ba, tref.render(frames, labels=[b, a], font=font, styles=STYLES))


def test_plate_0_and_style_0(ctx, font):
    frames = np.repeat(_frames(12, 1, H47, W94), 4, axis=0)          # one picture four times
    labels = [(0, 5, 5, 5, 0, 2, "INK"), (1, 5, 5, 0, 6, 2, "PLATE"), (2, 5, 5, 0, 0, 2, "NONE"), (3, 5, 5, 5, 6, 2, "BOTH")]
    want = tref.render(frames, labels=labels, font=font, styles=STYLES)
    plain = ref.yuv420(frames)
    assert np.array_equal(want[0][2], plain[0][2]) and all(not np.array_equal(want[0][f], plain[0][f]) for f in (0, 1, 3))
    assert len({want[0][f, 3:21].tobytes() for f in range(4)}) == 4
    _same(ctx.render_review(frames, labels=labels, styles=STYLES), want)


@pytest.mark.parametrize("alpha", [0, 1, 128, 255, 256])
def test_alphas(ctx, font, alpha):
    frames = _frames(13, 1, H47, W94)
    styles = [(12, 200, 77, 0, alpha), (240, 10, 130, alpha, 0)]
    labels = [(0, 4, 3, 1, 2, 2, "A=%d" % alpha), (0, 26, -2, 1, 2, 1, "0 1 128 255 256")]
    want = tref.render(frames, labels=labels, font=font, styles=styles)
    _same(ctx.render_review(frames, labels=labels, styles=styles), want)
    if alpha == 0:
        _same(want, ref.yuv420(frames))
    if alpha == 256:          # opaque: ink pixels are the ink's colour, the plate's the plate's
        composed = tref.compose(frames, labels=labels[:1], font=font, styles=styles)[0]
        assert {tuple(p) for p in composed[2:20, 1:60].reshape(-1, 3).tolist()} == {(12, 200, 77), (240, 10, 130)}


# ------------------------------------------------------------------------------------------ 4. counts
def _many_labels(F, seed):
    """300 labels on frame 5 (more than six LDS chunks of 48), no label on every third frame, a few on the others."""
    rng = np.random.default_rng(seed)
    labels = []
    for f in range(F):
        if f == 5 % F:
            for k in range(300):
                labels.append((f, int(rng.integers(-8, H47)), int(rng.integers(-20, W94)), int(rng.integers(0, 8)), int(rng.integers(0, 8)),
                               int(rng.integers(1, 3)), "".join(CHARSET[j] for j in rng.integers(0, 45, int(rng.integers(0, 5))))))
        elif f % 3 != 1:
            labels += [(f, H47 - 3 - 8, 4, 5, 6, 1, "F%06d 00:00:00.%03d" % (f, f)), (f, int(rng.integers(0, 30)), int(rng.integers(0, 80)), 3, 6, 1, "#%d" % f)]
    return labels


@pytest.mark.parametrize("F", [1, 43])
def test_counts(ctx, font, F):
    frames = _frames(14, F, H47 + 2, W94 + 3)
    labels = _many_labels(F, F)
    per = np.bincount([lab[0] for lab in labels], minlength=F)
    assert per.max() == 300 and (F == 1 or (per[1] == 0 and per[0] > 0 and per[2] > 0))
    kw = dict(labels=labels, styles=STYLES, boxes=[(0, 3, 3, 20, 40, 1)], frame_style=[3] * F, border=2)
    rect = (3, 1, W94, H47)
    _same(ctx.render_review(frames, rect=rect, **kw), tref.render(frames[:, 1:1 + H47, 3:3 + W94], font=font, **kw))


# ------------------------------------------------------------------------------------------ 5. equivalence
def test_no_labels_is_render_review(ctx):
    frames = _frames(15, 3, H47, W94)
    kw = dict(boxes=[(0, 2, 2, 30, 60, 1), (2, -2, 2, 30, 60, 2)], marks=[(1, 10, 12, 3)], frame_style=[3, 0, 2], mask=_mask_checker(), styles=STYLES,
              mask_style=4, mark_arm=6, border=4)
    for layout in ("i420", "nv12"):
        _same(ctx.render_review(frames, labels=[], layout=layout, **kw), ctx.render_review(frames, layout=layout, **kw))
    _same(ctx.render_review(frames, labels=[(1, 3, 3, 5, 6, 1, "")], **kw), ctx.render_review(frames, **kw))          # len 0 draws nothing


# ------------------------------------------------------------------------------------------ 6. refusals
def _dst(_lib, F, Hr, Wr):
    hc, wc = (Hr + 1) // 2, (Wr + 1) // 2
    back = [np.full(s, 0xA5, np.uint8) for s in [(F, Hr + 1, Wr + 3), (F, hc + 1, wc + 5), (F, hc + 1, wc + 5)]]
    dst = _lib.Yuv420Dst(y=back[0].ctypes.data, u=back[1].ctypes.data, v=back[2].ctypes.data, mem=_lib.MEM_HOST, layout=_lib.YUV_I420,
                         y_row_stride=Wr + 3, y_frame_stride=(Hr + 1) * (Wr + 3), c_row_stride=wc + 5, c_frame_stride=(hc + 1) * (wc + 5))
    return dst, back


def test_refusals_leave_the_destination_untouched(ctx, font):
    """Every refusal of the header's list for labels: SWK_ERR_ARG (-1), the destination as it was, the context usable afterwards."""
    from swiftwatcher_amd import _lib
    lib = _lib.load()
    frames = _frames(16, 2, H47, W94)
    styles = np.zeros(2, _lib.REVIEW_STYLE_DTYPE)
    styles["fill_alpha"], styles["line_alpha"] = 100, 200
    inp = _lib.Input(frames=frames.ctypes.data, mem=_lib.MEM_HOST, channels=3, nwin=1, n=2, Hc=H47, Wc=W94, x0=0, y0=0,
                     frame_stride=frames.strides[0], row_stride=frames.strides[1])
    rv = _lib.Review(mask=None, mask_style=0, boxes=None, nboxes=0, marks=None, nmarks=0, mark_arm=2, frame_style=None, border=1,
                     styles=styles.ctypes.data, nstyles=2)

    def call(count=None, null=False, null_rv=False, **change):
        labels = _lib.label_records([(0, 3, 3, 1, 2, 1, "AB"), (1, 3, 3, 2, 1, 2, "CD")])
        for name, value in change.items():
            if name == "text":
                labels["text"][1][:len(value)] = np.frombuffer(value, np.uint8)
            else:
                labels[name] = value
        dst, back = _dst(_lib, 2, H47, W94)
        rc = lib.swk_render_review_labels(ctx._h, ctypes.byref(inp), None if null_rv else ctypes.byref(rv), None if null else labels.ctypes.data,
                                          len(labels) if count is None else count, ctypes.byref(dst))
        return rc, all((b == 0xA5).all() for b in back)

    assert call() == (0, False)                                                     # the unchanged call draws
    assert call(null=True, count=0) == (0, False) and call(count=0) == (0, False)   # no labels: swk_render_review
    refused = [dict(null=True), dict(count=-1), dict(null=True, count=-1), dict(null_rv=True),
               dict(frame=[0, 2]), dict(frame=[-1, 0]), dict(frame=[1, 0]),
               dict(scale=[1, 0]), dict(scale=[9, 1]), dict(scale=[-1, 1]), dict(len=[2, 33]), dict(len=[-1, 2]),
               dict(style=[3, 0]), dict(style=[0, -1]), dict(plate=[0, 3]), dict(plate=[-1, 0]),
               dict(text=b"Cd"), dict(text=b"\x00D"), dict(text=b"C\xc1"), dict(text=b"C!"), dict(text=b"C\x7f"), dict(text=b"_D")]
    for change in refused:
        assert call(**dict(change)) == (-1, True), change
    assert ctx._lib.swk_last_error(ctx._h)
    # every byte outside the set is refused, every byte of it is taken; bytes past len are not looked at
    for ch in range(256):
        ok = ch < 128 and font[ch, 7] == 1
        assert call(text=bytes([ch, 65]))[0] == (0 if ok else -1), ch
    assert call(text=b"CD!\xff") == (0, False)
    _same(ctx.render_review(frames, labels=[(0, 3, 3, 1, 2, 1, "AB")], styles=STYLES), tref.render(frames, labels=[(0, 3, 3, 1, 2, 1, "AB")], font=font, styles=STYLES))


# ------------------------------------------------------------------------------------------ 7. the counting loops write the text
EVENT_HOLD, MARK_ARM, BORDER = 15, 4, 3          # ReviewWriter's documented defaults
PALETTE = [(0, 255, 0, 32, 256), (0, 0, 255, 0, 160), (0, 255, 255, 0, 256), (255, 128, 0, 40, 0), (255, 255, 255, 0, 256), (0, 0, 0, 160, 0)]


def _roi_mask():
    m = np.zeros((64, 96), np.uint8)
    m[28:, :] = 255
    return m


def _event_records(events):
    return [[(s.parent_frame_number, str(s.parent_timestamp), tuple(s.centroid), tuple(s.bbox), np.array(s.segment_image).tobytes()) for s in ev]
            for ev in events]


@pytest.fixture(scope="module")
def clip(tmp_path_factory):
    """tests/test_review_gpu.py's seeded 52-frame 110 x 160 clip: BGR frames, and an 8-bit 4:2:0 file of them (and of the first 23)."""
    import yuv_ref
    from swiftwatcher_amd import synthetic
    from swiftwatcher_amd.io_y4m import Y4MWriter
    bgr = synthetic.full_frames(500, 52, CROP, frame_hw=(110, 160), birds=4, bird_len=(8, 12), bird_wid=(3, 5))[::-1].copy()
    folder = tmp_path_factory.mktemp("review_text_gpu")
    y, u, v = yuv_ref.bgr_to_yuv420(bgr)
    paths = {}
    for name, count in (("y4m", 52), ("y4m_23", 23)):
        paths[name] = str(folder / (name + ".y4m"))
        with Y4MWriter(paths[name], 160, 110, 30) as w:
            for k in range(count):
                w.append(y[k], u[k], v[k])
    return dict(bgr=bgr, folder=folder, **paths)


class _Recorder:
    """Stands in for a ReviewWriter: keeps what the loop hands over -- the frames as the classifier and the tracker left them."""

    def __init__(self):
        self.windows = []

    def write_window(self, popped, rejected=None, new_events=()):
        self.windows.append((list(popped), [list(r or ()) for r in (rejected if rejected is not None else [None] * len(popped))],
                             [list(ev) for ev in new_events]))


def _stamp(timestamp):
    if hasattr(timestamp, "strftime"):
        return timestamp.strftime("%H:%M:%S.%f")[:12]
    return "".join(ch if ch in CHARSET else " " for ch in str(timestamp).upper()[:12])


def _expected(recorder, crop, roi_mask, font):
    """The frames ReviewWriter documents, text included, for what the loop handed over, by the test-side restatement."""
    (x0, y0), (x1, y1) = crop
    Hc, Wc = y1 - y0, x1 - x0
    s = max(1, min(4, (Wc - 2 * BORDER) // (6 * 33 + 1), (Hc // 8) // 9))
    frames, boxes, gone_count, events = [], [], [], []
    for popped, rejected, new_events in recorder.windows:
        for ev in new_events:
            first = ev[-1].parent_frame_number + 1
            events.append((first, [(int(np.floor(p.centroid[0] + 0.5)), int(np.floor(p.centroid[1] + 0.5))) for p in ev], len(events) + 1))
        for fr, gone in zip(popped, rejected):
            if fr.frame_number < 0:
                continue
            frames.append((fr, len(events)))          # (the events received when the frame's window was written)
            boxes.append([tuple(b.bbox) + (1,) for b in fr.segments] + [tuple(b) + (2,) for b in gone])
            gone_count.append(len(gone))
    crops = np.stack([np.asarray(fr.frame)[y0:y1, x0:x1] for fr, _ in frames])
    all_boxes = [(k,) + b for k, per in enumerate(boxes) for b in per]
    marks, frame_style, labels, lines = [], [], [], []
    for k, (fr, received) in enumerate(frames):
        known = events[:received]
        shown = [ev for ev in known if ev[0] <= fr.frame_number < ev[0] + EVENT_HOLD]
        frame_style.append(3 if shown else 0)
        marks += [(k, r, c, 3) for _, pts, _ in shown for r, c in pts]
        line = "F%06d %s S%02d R%02d E%03d" % (fr.frame_number, _stamp(fr.timestamp), len(fr.segments), gone_count[k],
                                               sum(1 for ev in known if ev[0] <= fr.frame_number))
        lines.append(line)
        for at in range(0, len(line), 32):
            labels.append((k, Hc - BORDER - 8 * s, BORDER + s + 6 * s * at, 5, 6, s, line[at:at + 32]))
        for _, pts, ordinal in shown:
            text = "#%d" % ordinal
            r = max(min(pts[-1][0] + MARK_ARM + 2 * s, Hc - BORDER - 8 * s), BORDER + s)
            c = max(min(pts[-1][1] + MARK_ARM + 2 * s, Wc - BORDER - 6 * s * len(text)), BORDER + s)
            labels.append((k, r, c, 3, 6, s, text))
    kw = dict(boxes=all_boxes, marks=marks, frame_style=frame_style, mask=roi_mask, styles=PALETTE, mask_style=4, mark_arm=MARK_ARM, border=BORDER)
    want = tref.render(crops, labels=labels, font=font, **kw)
    return want, dict(frames=len(frames), labels=len(labels), numbers=sum(1 for lab in labels if lab[3] == 3), lines=lines, no_text=ref.render(crops, **kw))


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


def _check_run(run, crop, roi_mask, path, font, min_frames=52, min_events=1):
    """run(review, review_text) -> (count, events): with a recorder, with no review, with a plain review and with a text review at
    `path`: equal counts and events, the text file holds what ReviewWriter documents for the recorded hand-over, and the plain file
    is that without the labels."""
    recorder = _Recorder()
    recorded = run(recorder, False)
    plain = run(None, False)
    written = run(path, True)
    assert len(plain[1]) >= min_events, "no event: no event number would be drawn"
    for got in (recorded, written):
        assert got[0] == plain[0] and _event_records(got[1]) == _event_records(plain[1])
    want, info = _expected(recorder, crop, roi_mask, font)
    got = _read_review(path, crop)
    print(path, info["frames"], "frames,", info["labels"], "labels,", info["numbers"], "event numbers;", info["lines"][0], "...", info["lines"][-1])
    assert got[0].shape[0] == info["frames"] >= min_frames and info["labels"] >= 2 * info["frames"] and (min_events == 0 or info["numbers"] > 0)
    _same(got, want)
    assert all(not np.array_equal(got[0][k], info["no_text"][0][k]) for k in range(info["frames"]))          # every frame carries its line
    return recorder, info


@pytest.mark.parametrize("wpc", [1, 2])
def test_text_review_of_a_y4m_file(clip, font, wpc):
    from swiftwatcher_amd import pipeline
    path = str(clip["folder"] / ("y4m_text_%d.y4m" % wpc))
    _, info = _check_run(lambda rv, text: pipeline.count_swifts(clip["y4m"], crop_region=CROP_ODD, roi_mask=_roi_mask(), windows_per_call=wpc, review=rv,
                                                                review_text=text), CROP_ODD, _roi_mask(), path, font)
    assert info["lines"][0].startswith("F000000 00:00:00.000 ") and info["lines"][30].startswith("F000030 00:00:01.")
    # without review_text the file is the review as it was
    plain_path = str(clip["folder"] / ("y4m_plain_%d.y4m" % wpc))
    pipeline.count_swifts(clip["y4m"], crop_region=CROP_ODD, roi_mask=_roi_mask(), windows_per_call=wpc, review=plain_path)
    _same(_read_review(plain_path, CROP_ODD), info["no_text"])


def test_text_review_through_count_swifts_videos(clip, font):
    """Two videos of different crop regions in one groups call; the first gets a text review, the second none."""
    from swiftwatcher_amd import pipeline
    path = str(clip["folder"] / "videos_text.y4m")
    small = [(40, 30), (40 + 64, 30 + 48)]
    mask2 = np.zeros((48, 64), np.uint8)
    mask2[20:, :] = 255
    regions = [(CROP, _roi_mask()), (small, mask2)]
    seen = []

    def run(rv, text):
        out = pipeline.count_swifts_videos([clip["bgr"], clip["y4m"]], regions=regions, reviews=None if rv is None else [rv, None], review_text=text)
        seen.append(out[1])
        return out[0]
    _check_run(run, CROP, _roi_mask(), path, font)
    assert all(o[0] == seen[0][0] and _event_records(o[1]) == _event_records(seen[0][1]) for o in seen[1:])          # the other video's count


def test_a_writer_handed_in_carries_its_own_setting(clip, font):
    """review_text is for writers made from a path: a ReviewWriter(text=True) handed in writes text whatever review_text says."""
    from swiftwatcher_amd import pipeline
    from swiftwatcher_amd.review import ReviewWriter
    path = str(clip["folder"] / "own_writer.y4m")

    def run(rv, text):
        if not isinstance(rv, str):
            return pipeline.count_swifts(clip["bgr"], crop_region=CROP, roi_mask=_roi_mask(), review=rv)
        with ReviewWriter(rv, CROP, _roi_mask(), 30, text=True) as w:
            return pipeline.count_swifts(clip["bgr"], crop_region=CROP, roi_mask=_roi_mask(), review=w, review_text=False)
    _check_run(run, CROP, _roi_mask(), path, font)


def test_cli_writes_the_text_review(clip, font):
    """python -m swiftwatcher_amd --review PATH --review-text in a fresh child process, on the 23-frame file: the same bytes as the
    in-process count with the same corners, which is checked against the restatement."""
    from swiftwatcher_amd import image_filtering as img
    from swiftwatcher_amd import pipeline
    from swiftwatcher_amd.io_y4m import open_y4m
    first = open_y4m(clip["y4m_23"])
    crop, roi_mask, _ = img.generate_regions(first.read_frame(0, increment=False), CORNERS)
    first.close() if hasattr(first, "close") else None
    here = str(clip["folder"] / "inproc_text.y4m")
    _check_run(lambda rv, text: pipeline.count_swifts(clip["y4m_23"], corners=CORNERS, review=rv, review_text=text), crop, roi_mask, here, font,
               min_frames=23, min_events=0)
    out = str(clip["folder"] / "cli_text.y4m")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    p = subprocess.run([sys.executable, "-m", "swiftwatcher_amd", clip["y4m_23"], "--corners", "%d,%d,%d,%d" % (CORNERS[0] + CORNERS[1]),
                        "--review", out, "--review-text"], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert p.returncode == 0, p.stdout + p.stderr
    line = json.loads(p.stdout.strip().splitlines()[-1])
    assert line["source"] == clip["y4m_23"] and line["frames"] == 23
    assert open(out, "rb").read() == open(here, "rb").read()
