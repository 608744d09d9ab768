"""swk_stabilize_u8 (csrc/stabilize.hip) against the numpy restatement (tests/stabilize_ref.py), equal on every entry of the SAD table,
every shift record and every output byte; its refusals; and the counting loop over a shaken clip with stabilize=8, which must hand
the tracker the segments of the still twin (tests/test_stabilize_cpu.py shows that the restatement alone recovers that clip's jitter).

Kernel cases: rectangles below one 16 x 256 tile, with odd widths (rows of the anchor and of the output start on every byte
alignment), and of more than one tile row (33, 47, 67 rows: 3, 3 and 5 tile rows with a partial last one); S = 0, 1, 8, 16 (1, 9, 289 and
1089 candidates: below, at and above the 256 threads of a workgroup); 1 and 21 frames; x0 of every residue mod 4; an odd row stride;
a negative frame stride; host and device sources, anchors and outputs; both grey modes; a nominal rectangle one pixel from each edge
of the picture; a window whose newest three frames are null.  Outputs lie in sentinel-filled buffers."""
import os
import threading

import numpy as np
import pytest

import stabilize_ref as ref
from helpers import Guarded

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from swiftwatcher_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


# (id, Ho, Wo, S, count, options)
CASES = [
    ("4x4_s0_n1", 4, 4, 0, 1, {}),
    ("4x4_s1_n21_dev", 4, 4, 1, 21, dict(src_dev=True, out_dev=True, x_res=1)),
    ("5x7_s8_n1_oddstride", 5, 7, 8, 1, dict(x_res=1, row_pad="odd")),
    ("5x7_s16_n21_devsrc", 5, 7, 16, 21, dict(x_res=3, src_dev=True, anchor_dev=True)),
    ("33x67_s8_n21_reversed", 33, 67, 8, 21, dict(x_res=2, reverse=True, frame_pad=5)),
    ("33x67_s1_n1_q15", 33, 67, 1, 1, dict(gray_mode=1, out_shift=3)),
    ("47x94_s16_n21_dev_q15_reversed", 47, 94, 16, 21, dict(x_res=1, src_dev=True, anchor_dev=True, out_dev=True, gray_mode=1, reverse=True,
                                                            row_pad="odd", frame_pad=3, out_shift=1)),
    ("47x94_s8_n21_nulltail", 47, 94, 8, 21, dict(x_res=3, null_tail=3)),
    ("47x94_s8_n21_nulltail_dev", 47, 94, 8, 21, dict(x_res=2, null_tail=3, src_dev=True, out_dev=True)),
    ("67x95_s16_n1", 67, 95, 16, 1, dict(x_res=3, out_shift=2)),
    ("67x95_s8_n21_dev_oddstride", 67, 95, 8, 21, dict(src_dev=True, row_pad="odd", anchor_dev=True)),
    ("67x95_s0_n21", 67, 95, 0, 21, dict(x_res=1)),
    ("5x300_s1_n1_two_tile_columns", 5, 300, 1, 1, dict(x_res=2)),
] + [("33x67_s8_n1_edge_%s" % e, 33, 67, 8, 1, dict(edge=e, x_res=k)) for k, e in enumerate(("top", "bottom", "left", "right"))] \
  + [("5x7_s1_n1_x%d" % k, 5, 7, 1, 1, dict(x_res=k, pad=(3, 4))) for k in range(4)] \
  + [("47x94_s16_n1_edge_%s" % e, 47, 94, 16, 1, dict(edge=e, src_dev=True)) for e in ("top", "right")]


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
    """the raw call with every output in a guarded buffer -> (shifts, table, pixels)"""
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
    g_shifts = Guarded(count * _lib.SHIFT_DTYPE.itemsize, False)
    g_table = Guarded(count * side * side * 8, False)
    shifts = g_shifts.buf[g_shifts.lead:g_shifts.lead + g_shifts.nbytes].view(_lib.SHIFT_DTYPE)
    table = g_table.buf[g_table.lead:g_table.lead + g_table.nbytes].view(np.uint64)
    ctx.stabilize_raw(fptr, fmem, count, Hs, Ws, fs, rs, y0, x0, Ho, Wo, S, aptr, amem, a.size, gray_mode, shifts, table, g_out.ptr,
                      _lib.MEM_DEVICE if out_dev else _lib.MEM_HOST)
    del keep
    return (g_shifts.read(_lib.SHIFT_DTYPE), g_table.read(np.uint64, (count, side, side)), g_out.read(np.uint8, (count, Ho, Wo, 3)))


def _assert_equal(got, want, label=""):
    shifts, table, pixels = got
    w_shifts, w_table, w_pixels = want
    assert np.array_equal(table, w_table), "%s: %d table entries differ" % (label, int((table != w_table).sum()))
    for key in ("dy", "dx", "sad", "sad_unshifted"):
        assert np.array_equal(shifts[key], w_shifts[key]), "%s: %s" % (label, key)
    assert np.array_equal(pixels, w_pixels), label


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_kernel_equals_the_restatement(ctx, case):
    name, Ho, Wo, S, count, opt = case
    opt = dict(opt)
    scene = {k: opt.pop(k) for k in ("x_res", "null_tail", "edge", "pad") if k in opt}
    frames, rect, anchor = ref.designed_case(Ho, Wo, S, count, seed=len(name) * 7919 + Ho * Wo + S, **scene)
    mode = opt.get("gray_mode", 0)
    want = ref.stabilize(frames, rect, S, anchor, mode)
    # the scene exercises what the case is about
    assert rect[1] % 4 == scene.get("x_res", rect[1] % 4) or "edge" in scene
    if "edge" in scene:
        assert (want[1] == ref.EXCLUDED).any() and (want[1] != ref.EXCLUDED).any()
    else:
        assert not (want[1] == ref.EXCLUDED).any()
    if S and count > 1:
        assert len({(int(s["dy"]), int(s["dx"])) for s in want[0]}) > 1
    if scene.get("null_tail"):
        assert not frames[-3:].any() and all(int(s["dy"]) == int(s["dx"]) == 0 and s["sad"] == s["sad_unshifted"] for s in want[0][-3:])
    _assert_equal(_run(ctx, frames, rect, S, anchor, **opt), want, name)


def test_wrapper_equals_the_restatement(ctx):
    """Context.stabilize: numpy in and out, strided numpy views, tensors in and out; with and without the table"""
    import torch
    frames, rect, anchor = ref.designed_case(33, 67, 8, 5, seed=77, x_res=1)
    want = ref.stabilize(frames, rect, 8, anchor)
    shifts, table, pixels = ctx.stabilize(frames, rect, 8, anchor, table=True)
    _assert_equal((shifts, table, pixels), want, "numpy")
    assert ctx.stabilize(frames, rect, 8, anchor)[1] is None
    wide = np.zeros((5, frames.shape[1], frames.shape[2] + 3, 3), np.uint8)
    wide[:, :, :-3] = frames
    _assert_equal(ctx.stabilize(wide[::-1][::-1][:, :, :-3], rect, 8, anchor, table=True), want, "strided view")
    s2, t2, p2 = ctx.stabilize(torch.from_numpy(frames).cuda(), rect, 8, torch.from_numpy(anchor).cuda(), device_out=True, table=True)
    assert p2.is_cuda
    _assert_equal((s2, t2, p2.cpu().numpy()), want, "tensors")


def test_refusals_leave_the_context_working(ctx):
    from swiftwatcher_amd import _lib
    frames, rect, anchor = ref.designed_case(33, 67, 8, 2, seed=5)
    y0, x0, Ho, Wo = rect
    Hs, Ws = frames.shape[1:3]
    with pytest.raises(_lib.SwkError, match="search"):
        ctx.stabilize(frames, rect, 17, anchor)
    for bad in [(Hs - Ho + 1, x0, Ho, Wo), (y0, Ws - Wo + 1, Ho, Wo), (-1, x0, Ho, Wo), (y0, -1, Ho, Wo), (y0, x0, 0, Wo)]:
        with pytest.raises(_lib.SwkError, match="rectangle"):
            ctx.stabilize(frames, bad, 8, anchor)
    for bad in (anchor[:-1], anchor[:, :-1], np.zeros((Ho + 1, Wo), np.uint8)):
        with pytest.raises(_lib.SwkError, match="anchor"):
            ctx.stabilize(frames, rect, 8, bad)
    with pytest.raises(_lib.SwkError, match="gray_mode"):
        ctx.stabilize(frames, rect, 8, anchor, gray_mode=2)
    _assert_equal(ctx.stabilize(frames, rect, 8, anchor, table=True), ref.stabilize(frames, rect, 8, anchor), "after the refusals")


# ------------------------------------------------------------------ the counting loop
CROP = ref.CLIP["crop_region"]
N = 21


def _roi_mask():
    m = np.zeros((64, 96), np.uint8)
    m[32:, 10:86] = 255
    return m


def _count(monkeypatch, source, videos=False, **kw):
    """pipeline.count_swifts (or count_swifts_videos on the one video) with the tracker spied on -> (segments per frame number, count,
    events as tuples, the StabilizingReaders made, calls of Context.stabilize)"""
    from swiftwatcher_amd import _lib, pipeline, stabilize
    seen, made, calls = {}, [], []

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

    init, call = stabilize.StabilizingReader.__init__, _lib.Context.stabilize

    def spy_init(self, *a, **k):
        made.append(self)
        init(self, *a, **k)

    def spy_call(self, *a, **k):
        calls.append(1)
        return call(self, *a, **k)

    with monkeypatch.context() as m:
        m.setattr(pipeline, "SegmentTracker", Spy)
        m.setattr(stabilize.StabilizingReader, "__init__", spy_init)
        m.setattr(_lib.Context, "stabilize", spy_call)
        if videos:
            (count, events), = pipeline.count_swifts_videos([source], regions=[(CROP, _roi_mask())], **kw)
        else:
            count, events = pipeline.count_swifts(source, CROP, _roi_mask(), **kw)
    sig = [[(s.parent_frame_number, s.label, tuple(s.bbox)) for s in ev] for ev in events]
    return seen, count, sig, made, len(calls)


def _assert_shifts(reader, jitter):
    total = len(jitter)
    assert set(range(total)) <= set(reader.shifts)
    for k in sorted(reader.shifts):
        jy, jx = jitter[min(k, total - 1)]
        assert reader.shifts[k][:2] == (-jy, -jx), "frame %d" % k


_still = {}


def _still_count(monkeypatch, wpc):
    if wpc not in _still:
        _still[wpc] = _count(monkeypatch, list(ref.shaken_clip()[1]), windows_per_call=wpc)
    return _still[wpc]


@pytest.mark.parametrize("windows_per_call", [1, 2])
def test_counting_loop_stabilized_equals_the_still_clip(monkeypatch, windows_per_call):
    shaken, still, jitter = ref.shaken_clip()
    want_seen, want_count, want_events, made0, calls0 = _still_count(monkeypatch, windows_per_call)
    assert not made0 and calls0 == 0                                                 # off: no wrapper, no call of the new entry point
    assert sorted(want_seen) == list(range(len(still) + 1)) and sum(len(v) for v in want_seen.values()) > 30
    seen, count, events, made, calls = _count(monkeypatch, list(shaken), windows_per_call=windows_per_call, stabilize=8)
    assert len(made) == 1 and calls == 3
    _assert_shifts(made[0], jitter)
    assert sorted(seen) == sorted(want_seen)
    for k in sorted(want_seen):
        assert seen[k] == want_seen[k], "frame %d" % k
    assert (count, events) == (want_count, want_events)
    # the same shaken clip as it is: other segments (this is what makes the test say something)
    raw_seen, _, _, made, calls = _count(monkeypatch, list(shaken), windows_per_call=windows_per_call)
    assert not made and calls == 0
    assert sum(raw_seen[k] != want_seen[k] for k in want_seen) > len(want_seen) // 2


def test_count_swifts_videos_stabilized(monkeypatch):
    shaken, _, jitter = ref.shaken_clip()
    want_seen, want_count, want_events, _, _ = _still_count(monkeypatch, 1)
    seen, count, events, made, calls = _count(monkeypatch, shaken, videos=True, stabilize=True)
    assert len(made) == 1 and made[0].search == 8 and calls == 3
    _assert_shifts(made[0], jitter)
    assert seen == want_seen and (count, events) == (want_count, want_events)


def _write_y4m(path, frames, chroma):
    from swiftwatcher_amd.io_y4m import Y4MWriter
    with Y4MWriter(str(path), frames.shape[2], frames.shape[1], 30, chroma=chroma) as w:
        for f in frames:
            w.append(*ref.yuv_planes(f, chroma))
    return str(path)


def test_y4m_file_stabilized(monkeypatch, tmp_path):
    """4:4:4 through YuvReader: the search rectangle is converted on the GPU and the call reads device memory"""
    shaken, still, jitter = ref.shaken_clip()
    want_seen, want_count, want_events, _, _ = _count(monkeypatch, _write_y4m(tmp_path / "still.y4m", still, "444"))
    assert sum(len(v) for v in want_seen.values()) > 30
    seen, count, events, made, calls = _count(monkeypatch, _write_y4m(tmp_path / "shaken.y4m", shaken, "444"), stabilize=8)
    assert len(made) == 1 and calls == 3
    _assert_shifts(made[0], jitter)
    assert seen == want_seen and (count, events) == (want_count, want_events)


def test_pipe_stabilized(monkeypatch, tmp_path):
    """8-bit 4:2:0 from a pipe: the stream reader holds the rectangle grown by the search range"""
    shaken, still, jitter = ref.shaken_clip()
    want_seen, want_count, want_events, _, _ = _count(monkeypatch, _write_y4m(tmp_path / "still.y4m", still, "420"))
    assert sum(len(v) for v in want_seen.values()) > 30
    with open(_write_y4m(tmp_path / "shaken.y4m", shaken, "420"), "rb") as fh:
        data = fh.read()
    rd, wr = os.pipe()

    def feed():
        with os.fdopen(wr, "wb") as out:
            out.write(data)

    feeder = threading.Thread(target=feed, daemon=True)
    feeder.start()
    with os.fdopen(rd, "rb", buffering=0) as source:
        seen, count, events, made, calls = _count(monkeypatch, source, stabilize=8)
    feeder.join()
    assert len(made) == 1 and calls == 3
    assert made[0].reader._rect == (0, 104, 10, 146) and made[0].reader.min_seg_size == (40, 40)
    _assert_shifts(made[0], jitter)
    assert seen == want_seen and (count, events) == (want_count, want_events)


def test_cli_writes_the_shifts(tmp_path, capsys):
    """python -m swiftwatcher_amd --stabilize --out DIR on the shaken clip as an 8-bit 4:2:0 file (in this process: main(argv)); without
    the option the JSON line has no "stabilize" entry and no stabilization.csv is written"""
    import csv
    import json
    from swiftwatcher_amd import __main__ as cli
    shaken, _, jitter = ref.shaken_clip()
    total = len(shaken)
    path = _write_y4m(tmp_path / "shaken.y4m", shaken, "420")
    corners = "%d,%d,%d,%d" % (ref.CORNERS[0] + ref.CORNERS[1])
    out = tmp_path / "tables"
    assert cli.main([path, "--corners", corners, "--stabilize", "--out", str(out)]) == 0
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    moved = int((jitter != 0).any(axis=1).sum()) + int(jitter[-1].any())           # (the frame one past the end is the last one again)
    assert line["frames"] == total and line["stabilize"] == {"search": 8, "moved_frames": moved, "max_shift": ref.JITTER}
    with open(out / "stabilization.csv", newline="") as fh:
        rows = list(csv.reader(fh))
    assert rows[0] == ["frame_number", "dy", "dx", "sad", "sad_unshifted"] and len(rows) == 1 + total + 1
    assert [[int(x) for x in r[:3]] for r in rows[1:total + 1]] == [[k, -jy, -jx] for k, (jy, jx) in enumerate(jitter)]
    assert all(int(r[3]) <= int(r[4]) for r in rows[1:])
    plain = tmp_path / "plain"
    assert cli.main([path, "--corners", corners, "--out", str(plain)]) == 0
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert "stabilize" not in line and not (plain / "stabilization.csv").exists()
