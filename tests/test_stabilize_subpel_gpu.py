"""swk_stabilize_subpel_u8 (csrc/stabilize.hip) against the numpy restatement (tests/stabilize_subpel_ref.py), equal on every record,
every entry of both tables and every output byte; its refusals; the frames left at q = (0, 0) against swk_stabilize_u8; and the
counting loop over the sub-pixel shaken clip with stabilize=5, stabilize_subpel=True, which must segment exactly the bytes that the
restatement resamples.

Kernel cases, named from the score kernel's anchor tile TR x TC (_lib.STABILIZE_SUBPEL_TILE): rectangles of 4 x 4 and 5 x 7 (less than
one tile), one less than, equal to and one more than the tile in each dimension ((TR + 1) x (TC + 1): two tile rows and two tile
columns with ragged ends); x0 of every residue mod 4; S = 0, 1, 8, 16 with stage-1 winners at +-S; 1 and 21 frames; host and device
sources, anchors and outputs; a negative frame stride and an odd row stride; both grey modes; a null-frame tail; nominal rectangles
0, 1 and 2 px from each edge of the picture; the 0 / 255 step plane.  Outputs lie in sentinel-filled buffers."""
import os
import threading

import numpy as np
import pytest

import stabilize_ref as ref1
import stabilize_subpel_ref as ref
from helpers import Guarded

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from swiftwatcher_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def _tile():
    from swiftwatcher_amd import _lib
    return _lib.STABILIZE_SUBPEL_TILE


def _cases():
    TR, TC = _tile()
    # (id, Ho, Wo, S, count, options)
    cases = [
        ("4x4_s0_n1", 4, 4, 0, 1, {}),
        ("4x4_s1_n21_dev", 4, 4, 1, 21, dict(src_dev=True, out_dev=True, x_res=1, extreme=True)),
        ("5x7_s8_n1_oddstride", 5, 7, 8, 1, dict(x_res=1, row_pad="odd", extreme=True)),
        ("5x7_s16_n21_devsrc", 5, 7, 16, 21, dict(x_res=3, src_dev=True, anchor_dev=True, extreme=True)),
        ("tile-1_s8_n21_reversed", TR - 1, TC - 1, 8, 21, dict(x_res=2, reverse=True, frame_pad=5, extreme=True)),
        ("tile_s1_n1_q15", TR, TC, 1, 1, dict(gray_mode=1, out_shift=3, extreme=True)),
        ("tile_s8_n21_dev", TR, TC, 8, 21, dict(x_res=3, src_dev=True, anchor_dev=True, out_dev=True)),
        ("tile+1_s16_n21_dev_q15_reversed", TR + 1, TC + 1, 16, 21, dict(x_res=1, src_dev=True, anchor_dev=True, out_dev=True, gray_mode=1,
                                                                        reverse=True, row_pad="odd", frame_pad=3, out_shift=1, extreme=True)),
        ("tile+1_s8_n21_nulltail", TR + 1, TC + 1, 8, 21, dict(x_res=3, null_tail=3)),
        ("tile+1_s8_n21_nulltail_dev", TR + 1, TC + 1, 8, 21, dict(x_res=2, null_tail=3, src_dev=True, out_dev=True)),
        ("rows+1_cols-1_s16_n1", TR + 1, TC - 1, 16, 1, dict(x_res=3, out_shift=2, extreme=True)),
        ("rows-1_cols+1_s0_n21", TR - 1, TC + 1, 0, 21, dict(x_res=1)),
        ("tile+1_s2_n5_steps", TR + 1, TC + 1, 2, 5, dict(x_res=2, steps=True)),
        ("5x7_s1_n3_steps_dev", 5, 7, 1, 3, dict(x_res=1, steps=True, src_dev=True, out_dev=True)),
    ]
    cases += [("5x7_s1_n1_x%d" % k, 5, 7, 1, 1, dict(x_res=k, pad=(4, 4))) for k in range(4)]
    cases += [("tile+1_s2_n5_%s_gap%d" % (e, gap), TR + 1, TC + 1, 2, 5, dict(edge=e, gap=gap, x_res=k, src_dev=bool(gap == 1)))
              for k, e in enumerate(("top", "bottom", "left", "right")) for gap in (0, 1, 2)]
    return cases


CASES = _cases()
SCENE_KEYS = ("x_res", "null_tail", "edge", "gap", "pad", "steps", "extreme")


def build_case(case):
    """(frames, rect, anchor, the restatement's result, the options of the call); asserts that the case exercises what it is named for"""
    name, Ho, Wo, S, count, opt = case
    opt = dict(opt)
    scene = {k: opt.pop(k) for k in SCENE_KEYS if k in opt}
    frames, rect, anchor = ref.designed_case(Ho, Wo, S, count, seed=len(name) * 7919 + Ho * Wo + S, **scene)
    mode = opt.get("gray_mode", 0)
    want = ref.stabilize_subpel(frames, rect, S, anchor, mode)
    recs, (table, sub), pixels = want
    assert rect[1] % 4 == scene.get("x_res", rect[1] % 4) or "edge" in scene
    live = recs[:count - scene.get("null_tail", 0)]
    if "edge" in scene:
        assert (sub == ref.EXCLUDED).any() and (sub != ref.EXCLUDED).any()
        assert (sub[:, 2, 2] != ref.EXCLUDED).all()
    else:
        assert not (sub == ref.EXCLUDED).any() and not (table == ref.EXCLUDED).any()
    if count > 1 and not scene.get("steps"):          # (the step plane's frames move by whole pixels under one anchor phase)
        assert len({(int(r["qy_total"]) & 3, int(r["qx_total"]) & 3) for r in live}) > 1, "one phase only"
    if scene.get("extreme") and S:
        assert (int(recs[0]["dy"]), int(recs[0]["dx"])) in ((S, -S), (-S, S))
        if count > 1:
            assert (int(recs[1]["dy"]), int(recs[1]["dx"])) == (-int(recs[0]["dy"]), -int(recs[0]["dx"]))
    if scene.get("null_tail"):
        k = scene["null_tail"]
        assert not frames[-k:].any() and not pixels[-k:].any()
        assert all(int(r["qy_total"]) == int(r["qx_total"]) == 0 and r["sad"] == r["sad_int"] == r["sad_unshifted"] for r in recs[-k:])
    if scene.get("steps"):          # the clamp works in both directions, in the scores and in the pixels handed out
        lo = hi = False
        for f, r in enumerate(recs):
            Qy, Qx = int(r["qy_total"]), int(r["qx_total"])
            assert (Qy & 3, Qx & 3) != (0, 0)
            v = (ref.resample_unclamped(frames[f], rect, Qy, Qx) + 8192) >> 14
            lo, hi = lo or bool((v < 0).any()), hi or bool((v > 255).any())
        assert lo and hi, "the chosen phases do not reach the clamp"
    return frames, rect, anchor, want, opt


def _embed(frames, row_pad, frame_pad, reverse):
    """(byte buffer, offset of frame 0, frame stride, row stride): noise everywhere, the frames at their place"""
    count, Hs, Ws, _ = frames.shape
    rs = Ws * 3
    if row_pad == "odd":
        rs += 1 if rs % 2 == 0 else 2
    fs = Hs * rs + frame_pad
    base = 3
    buf = np.random.default_rng(count * 1000 + Hs).integers(1, 256, size=base + count * fs + 8, dtype=np.uint8)
    view = np.lib.stride_tricks.as_strided(buf[base:], shape=(count, Hs, Ws, 3), strides=(fs, rs, 3, 1), writeable=True)
    view[:] = frames[::-1] if reverse else frames
    if reverse:
        return buf, base + (count - 1) * fs, -fs, rs
    return buf, base, fs, rs


def _run(ctx, frames, rect, S, anchor, gray_mode=0, src_dev=False, anchor_dev=False, out_dev=False, row_pad=0, frame_pad=0, reverse=False,
         out_shift=0):
    """the raw call with every output in a guarded buffer -> (records, (table, sub_table), pixels)"""
    import torch
    from swiftwatcher_amd import _lib
    count, Hs, Ws, _ = frames.shape
    y0, x0, Ho, Wo = rect
    side = 2 * S + 1
    buf, off, fs, rs = _embed(frames, row_pad, frame_pad, reverse)
    keep = [buf]
    if src_dev:
        t = torch.from_numpy(buf).cuda()
        keep.append(t)
        fptr, fmem = t.data_ptr() + off, _lib.MEM_DEVICE
    else:
        fptr, fmem = buf.ctypes.data + off, _lib.MEM_HOST
    a = np.ascontiguousarray(anchor)
    if anchor_dev:
        ta = torch.from_numpy(np.concatenate([np.zeros(1, np.uint8), a.ravel()])).cuda()          # (one byte past a 256-byte boundary)
        keep.append(ta)
        aptr, amem = ta.data_ptr() + 1, _lib.MEM_DEVICE
    else:
        aptr, amem = a.ctypes.data, _lib.MEM_HOST
    g_out = Guarded(count * Ho * Wo * 3, out_dev, shift=out_shift)
    g_recs = Guarded(count * _lib.SUBSHIFT_DTYPE.itemsize, False)
    g_table = Guarded(count * side * side * 8, False)
    g_sub = Guarded(count * 25 * 8, False)
    recs = g_recs.buf[g_recs.lead:g_recs.lead + g_recs.nbytes].view(_lib.SUBSHIFT_DTYPE)
    table = g_table.buf[g_table.lead:g_table.lead + g_table.nbytes].view(np.uint64)
    sub = g_sub.buf[g_sub.lead:g_sub.lead + g_sub.nbytes].view(np.uint64)
    ctx.stabilize_subpel_raw(fptr, fmem, count, Hs, Ws, fs, rs, y0, x0, Ho, Wo, S, aptr, amem, a.size, gray_mode, recs, table, sub, g_out.ptr,
                             _lib.MEM_DEVICE if out_dev else _lib.MEM_HOST)
    del keep
    return (g_recs.read(_lib.SUBSHIFT_DTYPE), (g_table.read(np.uint64, (count, side, side)), g_sub.read(np.uint64, (count, 5, 5))),
            g_out.read(np.uint8, (count, Ho, Wo, 3)))


def _assert_equal(got, want, label=""):
    recs, (table, sub), pixels = got
    w_recs, (w_table, w_sub), w_pixels = want
    assert np.array_equal(table, w_table), "%s: %d entries of stage 1's table differ" % (label, int((table != w_table).sum()))
    assert np.array_equal(sub, w_sub), "%s: %d entries of the quarter-pixel table differ" % (label, int((sub != w_sub).sum()))
    for key in ref.SUBSHIFT_DTYPE.names:
        assert np.array_equal(recs[key], w_recs[key]), "%s: %s" % (label, key)
    assert np.array_equal(pixels, w_pixels), "%s: %d output bytes differ" % (label, int((pixels != w_pixels).sum()))


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_kernel_equals_the_restatement(ctx, case):
    frames, rect, anchor, want, opt = build_case(case)
    _assert_equal(_run(ctx, frames, rect, case[3], anchor, **opt), want, case[0])


def test_wrapper_equals_the_restatement(ctx):
    """Context.stabilize_subpel: numpy in and out, strided numpy views, tensors in and out; with and without the tables"""
    import torch
    from swiftwatcher_amd import _lib
    assert _lib.SUBSHIFT_DTYPE == ref.SUBSHIFT_DTYPE
    frames, rect, anchor = ref.designed_case(33, 67, 8, 5, seed=77, x_res=1)
    want = ref.stabilize_subpel(frames, rect, 8, anchor)
    _assert_equal(ctx.stabilize_subpel(frames, rect, 8, anchor, table=True), want, "numpy")
    assert ctx.stabilize_subpel(frames, rect, 8, anchor)[1] is None
    wide = np.zeros((5, frames.shape[1], frames.shape[2] + 3, 3), np.uint8)
    wide[:, :, :-3] = frames
    _assert_equal(ctx.stabilize_subpel(wide[::-1][::-1][:, :, :-3], rect, 8, anchor, table=True), want, "strided view")
    r2, t2, p2 = ctx.stabilize_subpel(torch.from_numpy(frames).cuda(), rect, 8, torch.from_numpy(anchor).cuda(), device_out=True, table=True)
    assert p2.is_cuda
    _assert_equal((r2, t2, p2.cpu().numpy()), want, "tensors")


def test_refusals_leave_the_outputs_and_the_context(ctx):
    """every refusal of swk_stabilize_u8, with the outputs untouched; then both calls alternating on the one context"""
    from swiftwatcher_amd import _lib
    frames, rect, anchor = ref.designed_case(33, 67, 8, 2, seed=5)
    y0, x0, Ho, Wo = rect
    count, Hs, Ws, _ = frames.shape
    frames = np.ascontiguousarray(frames)

    def raw(count=count, Hs=Hs, Ws=Ws, rs=Ws * 3, rect=rect, S=8, abytes=anchor.size, mode=0, fmem=_lib.MEM_HOST, omem=_lib.MEM_HOST,
            amem=_lib.MEM_HOST, fptr=frames.ctypes.data, aptr=anchor.ctypes.data, null_out=False, null_recs=False):
        g_out, g_recs, g_tab, g_sub = Guarded(2 * Ho * Wo * 3, False), Guarded(2 * 40, False), Guarded(2 * 33 * 33 * 8, False), Guarded(2 * 200, False)
        views = [g.buf[g.lead:g.lead + g.nbytes] for g in (g_recs, g_tab, g_sub)]
        with pytest.raises(_lib.SwkError) as exc:
            ctx.stabilize_subpel_raw(fptr, fmem, count, Hs, Ws, Hs * rs, rs, *rect, S, aptr, amem, abytes, mode, None if null_recs else views[0],
                                     views[1], views[2], None if null_out else g_out.ptr, omem)
        for g in (g_out, g_recs, g_tab, g_sub):
            assert (g.read() == Guarded.SENTINEL).all(), "a refused call wrote an output"
        return str(exc.value)

    assert "search" in raw(S=17) and "search" in raw(S=-1)
    for bad in [(Hs - Ho + 1, x0, Ho, Wo), (y0, Ws - Wo + 1, Ho, Wo), (-1, x0, Ho, Wo), (y0, -1, Ho, Wo), (y0, x0, 0, Wo)]:
        assert "rectangle" in raw(rect=bad)
    assert "anchor" in raw(abytes=anchor.size - 1)
    assert "gray_mode" in raw(mode=2)
    assert "count" in raw(count=0)
    assert "frame size" in raw(Hs=0) and "frame size" in raw(Ws=32769)
    assert "row stride" in raw(rs=Ws * 3 - 1)
    assert "mem" in raw(fmem=7) and "mem" in raw(omem=7) and "mem" in raw(amem=-1)
    assert "null" in raw(fptr=None) and "null" in raw(aptr=None) and "null" in raw(null_out=True) and "null" in raw(null_recs=True)
    assert "too many" in raw(count=(1 << 24) + 1)
    with pytest.raises(_lib.SwkError, match="search"):
        ctx.stabilize_subpel(frames, rect, 17, anchor)
    want1, want2 = ref1.stabilize(frames, rect, 8, anchor), ref.stabilize_subpel(frames, rect, 8, anchor)
    small = ref.designed_case(5, 7, 1, 3, seed=6)
    for _ in range(2):
        _assert_equal(ctx.stabilize_subpel(frames, rect, 8, anchor, table=True), want2, "after the refusals")
        s, t, p = ctx.stabilize(frames, rect, 8, anchor, table=True)
        assert np.array_equal(s, want1[0]) and np.array_equal(t, want1[1]) and np.array_equal(p, want1[2])
        _assert_equal(ctx.stabilize_subpel(small[0], small[1], 1, small[2], table=True), ref.stabilize_subpel(small[0], small[1], 1, small[2]),
                      "a smaller call in between")


def test_frames_left_at_q00_are_the_integer_calls(ctx):
    """an integer-jitter clip cut from a noise-free scene: the restatement leaves every frame at q = (0, 0), and the call's pixels and
    dy, dx are swk_stabilize_u8's"""
    from swiftwatcher_amd.stabilize import search_rect
    shaken, _, jitter = ref.subpel_clip(total=21, noise=0.0, integer_jitter=True)
    assert (jitter % 4 == 0).all() and len({tuple(j) for j in jitter}) > 10
    (ya, yb, xa, xb), (sa, sb, ta, tb) = search_rect(ref.CLIP["frame_hw"], ref.CLIP["crop_region"], 7)
    rect = (ya - sa, xa - ta, yb - ya, xb - xa)
    src = np.ascontiguousarray(shaken[:, sa:sb, ta:tb])
    anchor = ref1.gray(shaken[0][ya:yb, xa:xb])
    want = ref.stabilize_subpel(src, rect, 5, anchor)
    assert (want[0]["qy_total"] == 4 * want[0]["dy"]).all() and (want[0]["qx_total"] == 4 * want[0]["dx"]).all()
    assert np.array_equal(np.stack([want[0]["dy"], want[0]["dx"]], 1) * 4, -jitter)
    recs, _, pixels = ctx.stabilize_subpel(src, rect, 5, anchor)
    shifts, _, pixels1 = ctx.stabilize(src, rect, 5, anchor)
    assert np.array_equal(pixels, pixels1)
    for a, b in (("dy", "dy"), ("dx", "dx"), ("sad_int", "sad"), ("sad", "sad"), ("sad_unshifted", "sad_unshifted")):
        assert np.array_equal(recs[a], shifts[b]), a
    assert np.array_equal(recs["qy_total"], 4 * shifts["dy"]) and np.array_equal(recs["qx_total"], 4 * shifts["dx"])


# ------------------------------------------------------------------ the counting loop
CROP = ref.CLIP["crop_region"]
S_LOOP = 5


def _roi_mask():
    m = np.zeros((64, 96), np.uint8)
    m[32:, 10:86] = 255
    return m


def _count(monkeypatch, source, videos=False, **kw):
    """pipeline.count_swifts (or count_swifts_videos on the one video) with the tracker spied on -> (segments per frame number, count,
    events as tuples, the StabilizingReaders made, calls of Context.stabilize, calls of Context.stabilize_subpel)"""
    from swiftwatcher_amd import _lib, pipeline, stabilize
    seen, made, calls, subcalls = {}, [], [], []

    class Spy(pipeline.SegmentTracker):
        def set_current_frame(self, frame):
            if frame.frame_number >= 0:
                seen[frame.frame_number] = [(s.label, tuple(s.bbox), tuple(s.centroid), s.area) for s in frame.segments]
            super().set_current_frame(frame)

        def step_window(self, frames):
            for frame in frames:
                if frame.frame_number >= 0:
                    seen[frame.frame_number] = [(s.label, tuple(s.bbox), tuple(s.centroid), s.area) for s in frame.segments]
            return super().step_window(frames)

    init, call, subcall = stabilize.StabilizingReader.__init__, _lib.Context.stabilize, _lib.Context.stabilize_subpel

    def spy_init(self, *a, **k):
        made.append(self)
        init(self, *a, **k)

    def spy_call(self, *a, **k):
        calls.append(1)
        return call(self, *a, **k)

    def spy_subcall(self, *a, **k):
        subcalls.append(1)
        return subcall(self, *a, **k)

    with monkeypatch.context() as m:
        m.setattr(pipeline, "SegmentTracker", Spy)
        m.setattr(stabilize.StabilizingReader, "__init__", spy_init)
        m.setattr(_lib.Context, "stabilize", spy_call)
        m.setattr(_lib.Context, "stabilize_subpel", spy_subcall)
        if videos:
            (count, events), = pipeline.count_swifts_videos([source], regions=[(CROP, _roi_mask())], **kw)
        else:
            count, events = pipeline.count_swifts(source, CROP, _roi_mask(), **kw)
    sig = [[(s.parent_frame_number, s.label, tuple(s.bbox)) for s in ev] for ev in events]
    return seen, count, sig, made, len(calls), len(subcalls)


_pasted = {}


def _restated(source, subpel):
    """(full frames of the clip `source` with the restatement's stabilized rectangles pasted at their unshifted place, the reader that
    made them): StabilizingReader over RefSubpelBackend, window by window as the counting loop reads"""
    from swiftwatcher_amd.io_frames import ArrayReader
    from swiftwatcher_amd.stabilize import StabilizingReader
    key = (id(source), subpel)
    if key not in _pasted:
        total = len(source)
        reader = StabilizingReader(ArrayReader(list(source)), CROP, S_LOOP, backend=ref.RefSubpelBackend(), subpel=subpel)
        out = np.array(source)
        while reader.next_frame_number <= total:
            frames, numbers, _ = reader.get_n_frames(21)
            for fr, num in zip(frames, numbers):
                if 0 <= num < total:
                    (ya, xa), (h, w) = fr.origin, fr.roi.shape[:2]
                    out[num, ya:ya + h, xa:xa + w] = fr.roi
        _pasted[key] = (out, reader)
    return _pasted[key]


@pytest.mark.parametrize("windows_per_call", [1, 2])
def test_counting_loop_segments_the_restatements_bytes(monkeypatch, windows_per_call):
    shaken, _, jitter = ref.subpel_clip()
    pasted, ref_reader = _restated(shaken, True)
    assert sum(1 for v in ref_reader.subshifts.values() if v[0] % 4 or v[1] % 4) > len(shaken) // 2
    want_seen, want_count, want_events, made0, calls0, sub0 = _count(monkeypatch, list(pasted), windows_per_call=windows_per_call)
    assert not made0 and calls0 == 0 and sub0 == 0
    seen, count, events, made, calls, subcalls = _count(monkeypatch, list(shaken), windows_per_call=windows_per_call, stabilize=S_LOOP,
                                                        stabilize_subpel=True)
    assert len(made) == 1 and made[0].subpel and (calls, subcalls) == (0, 3)
    assert made[0].subshifts == ref_reader.subshifts and made[0].shifts == ref_reader.shifts
    assert sorted(seen) == sorted(want_seen)
    for k in sorted(want_seen):
        assert seen[k] == want_seen[k], "frame %d" % k
    assert (count, events) == (want_count, want_events)


def test_counting_loop_yields_fewer_segments_than_the_integer_stage(monkeypatch):
    shaken, still, _ = ref.subpel_clip()
    seen1, _, _, made1, calls1, sub1 = _count(monkeypatch, list(shaken), stabilize=S_LOOP)
    seen2, _, _, made2, calls2, sub2 = _count(monkeypatch, list(shaken), stabilize=S_LOOP, stabilize_subpel=True)
    assert (calls1, sub1, calls2, sub2) == (3, 0, 0, 3) and not made1[0].subpel and not made1[0].subshifts
    n1, n2 = sum(len(v) for v in seen1.values()), sum(len(v) for v in seen2.values())
    print("segments: integer stage %d, quarter-pixel stage %d" % (n1, n2))
    assert n2 < n1


def _write_y4m(path, frames, chroma):
    from swiftwatcher_amd.io_y4m import Y4MWriter
    with Y4MWriter(str(path), frames.shape[2], frames.shape[1], 30, chroma=chroma) as w:
        for f in frames:
            w.append(*ref1.yuv_planes(f, chroma))
    return str(path)


def test_pipe_stabilized_to_a_quarter_pixel(monkeypatch, tmp_path):
    """8-bit 4:2:0 from a pipe: the stream reader holds the rectangle grown by S + 2, and the loop segments what the restatement
    resamples from the frames a reader of that file hands out"""
    shaken, _, _ = ref.subpel_clip()
    decoded = ref1.yuv420_round_trip(shaken)
    pasted, ref_reader = _restated(decoded, True)
    want_seen, want_count, want_events, _, _, _ = _count(monkeypatch, list(pasted))
    with open(_write_y4m(tmp_path / "shaken.y4m", shaken, "420"), "rb") as fh:
        data = fh.read()
    rd, wr = os.pipe()

    def feed():
        with os.fdopen(wr, "wb") as out:
            out.write(data)

    feeder = threading.Thread(target=feed, daemon=True)
    feeder.start()
    with os.fdopen(rd, "rb", buffering=0) as source:
        seen, count, events, made, calls, subcalls = _count(monkeypatch, source, stabilize=S_LOOP, stabilize_subpel=True)
    feeder.join()
    assert len(made) == 1 and (calls, subcalls) == (0, 3)
    # the margin rectangle (8, 96, 18, 138) grown by S + 2 = 7 is (1, 103, 11, 145); a 4:2:0 reader holds it from the even row and column
    assert made[0].reader.min_seg_size == (24 + 14, 24 + 14) and made[0].reader._rect == (0, 103, 10, 145)
    assert made[0].subshifts == ref_reader.subshifts
    assert seen == want_seen and (count, events) == (want_count, want_events)


def test_cli_writes_the_quarter_pixel_shifts(tmp_path, capsys):
    """python -m swiftwatcher_amd --stabilize 5 --stabilize-subpel --out DIR on the clip as an 8-bit 4:2:0 file (main(argv))"""
    import csv
    import json
    from swiftwatcher_amd import __main__ as cli
    shaken, _, jitter = ref.subpel_clip()
    total = len(shaken)
    path = _write_y4m(tmp_path / "shaken.y4m", shaken, "420")
    corners = "%d,%d,%d,%d" % (ref1.CORNERS[0] + ref1.CORNERS[1])
    out = tmp_path / "tables"
    assert cli.main([path, "--corners", corners, "--stabilize", "5", "--stabilize-subpel", "--out", str(out)]) == 0
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["frames"] == total and line["stabilize"]["subpel"] is True and line["stabilize"]["search"] == 5
    with open(out / "stabilization.csv", newline="") as fh:
        rows = list(csv.reader(fh))
    assert rows[0] == ["frame_number", "dy", "dx", "sad", "sad_unshifted", "shift_y", "shift_x", "sad_subpel"] and len(rows) == 1 + total + 1
    got = np.array([[float(r[5]), float(r[6])] for r in rows[1:total + 1]]) * 4
    assert np.abs(got + jitter).max() <= 1                                          # within a quarter pixel of the true jitter
    assert line["stabilize"]["fractional_frames"] == sum(1 for r in rows[1:] if float(r[5]) % 1 or float(r[6]) % 1) > total // 2
    assert all(int(r[7]) <= int(r[3]) <= int(r[4]) for r in rows[1:])
    assert all(len(r[5].split(".")[1]) == 2 for r in rows[1:])
