"""Stabilization without a GPU: the numpy restatement of swk_stabilize_u8 (tests/stabilize_ref.py) on designed planes, the shaken
scene the GPU tests count (the restatement alone must recover its jitter exactly, so that the GPU tests rest on inputs known to be
decidable), stabilize.StabilizingReader with the restatement injected in place of the GPU call, and the CLI's option and CSV."""
import csv

import numpy as np
import pytest

import stabilize_ref as ref


def _textured(seed, H, W):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)


# ------------------------------------------------------------------ 1. the restatement on designed planes
def test_grey_is_the_oracles_formula():
    from oracle import reference_path as orc
    bgr = _textured(1, 9, 13)
    for mode in (0, 1):
        assert np.array_equal(ref.gray(bgr, mode), orc.bgr2gray(np.ascontiguousarray(bgr), mode))


@pytest.mark.parametrize("shift", [(0, 0), (3, -2), (-4, 4), (1, 0), (-4, -4)])
def test_moved_scene_gives_its_shift_with_sad_zero(shift):
    scene = _textured(2, 60, 70)
    y0, x0, Ho, Wo, S = 10, 12, 30, 40, 4
    anchor = ref.gray(scene[y0:y0 + Ho, x0:x0 + Wo])
    dy, dx = shift
    # the picture whose rectangle at (y0 + dy, x0 + dx) shows what the anchor shows
    frame = np.roll(scene, (dy, dx), axis=(0, 1))
    shifts, table, pixels = ref.stabilize(frame[None], (y0, x0, Ho, Wo), S, anchor)
    assert (int(shifts[0]["dy"]), int(shifts[0]["dx"]), int(shifts[0]["sad"])) == (dy, dx, 0)
    assert int(shifts[0]["sad_unshifted"]) == int(table[0, S, S])
    assert np.array_equal(pixels[0], scene[y0:y0 + Ho, x0:x0 + Wo])
    assert (table[0] == 0).sum() == 1


def test_flat_frame_gives_no_shift():
    frame = np.full((1, 40, 50, 3), 90, np.uint8)
    anchor = np.full((20, 30), 120, np.uint8)
    shifts, table, _ = ref.stabilize(frame, (10, 10, 20, 30), 8, anchor)
    assert (int(shifts[0]["dy"]), int(shifts[0]["dx"])) == (0, 0)
    assert len(np.unique(table[0])) == 1 and int(shifts[0]["sad"]) == int(shifts[0]["sad_unshifted"]) == 20 * 30 * 30


def test_ties_go_to_the_smallest_norm_then_dy_then_dx():
    # period 3 in x, constant in y: every (dy, 3 k) scores zero; the smallest norm is (0, 0)
    row = np.tile(np.array([10, 120, 240], np.uint8), 30)[:64]
    frame = np.repeat(np.repeat(row[None, :, None], 40, 0), 3, 2)
    y0, x0, Ho, Wo, S = 8, 9, 20, 30, 4
    anchor = ref.gray(frame[y0:y0 + Ho, x0:x0 + Wo])
    shifts, table, _ = ref.stabilize(frame[None], (y0, x0, Ho, Wo), S, anchor)
    zeros = {(dy - S, dx - S) for dy, dx in zip(*np.nonzero(table[0] == 0))}
    assert zeros == {(dy, dx) for dy in range(-S, S + 1) for dx in (-3, 0, 3)}
    assert (int(shifts[0]["dy"]), int(shifts[0]["dx"])) == (0, 0)
    # the anchor one column further: zero scores at dx = -2, 1, 4; norm 1 at (0, 1) alone
    anchor = ref.gray(frame[y0:y0 + Ho, x0 + 1:x0 + 1 + Wo])
    shifts, table, _ = ref.stabilize(frame[None], (y0, x0, Ho, Wo), S, anchor)
    assert (int(shifts[0]["dy"]), int(shifts[0]["dx"]), int(shifts[0]["sad"])) == (0, 1, 0)
    # the rule's order on a hand-made table: equal score and norm -> the smaller dy, then the smaller dx
    t = np.full((3, 3), 7, np.uint64)
    t[1, 1] = 9
    assert ref.choose(t, 1) == (-1, 0)               # norm 1: (-1, 0), (0, -1), (0, 1), (1, 0)
    t[0, 1] = 9
    assert ref.choose(t, 1) == (0, -1)


def test_crop_at_the_corner_excludes_candidates():
    frame = _textured(3, 30, 40)[None]
    Ho, Wo, S = 20, 25, 3
    anchor = ref.gray(frame[0][:Ho, :Wo])
    shifts, table, _ = ref.stabilize(frame, (0, 0, Ho, Wo), S, anchor)
    inside = np.array([[dy >= 0 and dx >= 0 for dx in range(-S, S + 1)] for dy in range(-S, S + 1)])
    assert np.array_equal(table[0] == ref.EXCLUDED, ~inside)
    assert (int(shifts[0]["dy"]), int(shifts[0]["dx"]), int(shifts[0]["sad"])) == (0, 0, 0)
    # bottom right: only dy <= 2, dx <= 1 remain
    shifts, table, _ = ref.stabilize(frame, (30 - Ho - 2, 40 - Wo - 1, Ho, Wo), S, anchor)
    inside = np.array([[dy <= 2 and dx <= 1 for dx in range(-S, S + 1)] for dy in range(-S, S + 1)])
    assert np.array_equal(table[0] == ref.EXCLUDED, ~inside)


def test_null_frames_are_not_matched():
    frames = np.stack([_textured(4, 30, 40), np.zeros((30, 40, 3), np.uint8)])
    anchor = ref.gray(frames[0][6:26, 9:29])
    shifts, table, pixels = ref.stabilize(frames, (5, 8, 20, 20), 4, anchor)
    assert (int(shifts[0]["dy"]), int(shifts[0]["dx"]), int(shifts[0]["sad"])) == (1, 1, 0)
    assert (int(shifts[1]["dy"]), int(shifts[1]["dx"])) == (0, 0)
    assert int(shifts[1]["sad"]) == int(shifts[1]["sad_unshifted"]) == int(anchor.astype(np.int64).sum())
    assert not pixels[1].any()


def test_refusals_of_the_restatement():
    frame = _textured(5, 30, 40)[None]
    anchor = np.zeros((20, 20), np.uint8)
    for rect, S, a in [((5, 8, 20, 20), 17, anchor), ((11, 8, 20, 20), 4, anchor), ((5, 8, 20, 20), 4, anchor[:19])]:
        with pytest.raises(ValueError):
            ref.stabilize(frame, rect, S, a)


# ------------------------------------------------------------------ 2. the shaken scene
def _margin_and_search(S=8):
    from swiftwatcher_amd.stabilize import search_rect
    return search_rect(ref.CLIP["frame_hw"], ref.CLIP["crop_region"], S)


@pytest.mark.parametrize("reanchor", [0, 1])
def test_restatement_recovers_the_jitter_of_the_shaken_scene(reanchor):
    shaken, still, jitter = ref.shaken_clip()
    assert np.abs(jitter).max() == ref.JITTER and (jitter[0] == 0).all() and len({tuple(j) for j in jitter}) > 30
    (ya, yb, xa, xb), _ = _margin_and_search()
    rect = (ya, xa, yb - ya, xb - xa)
    anchor = ref.gray(shaken[0][ya:yb, xa:xb])
    n = 21
    for w0 in range(0, len(shaken), n):
        shifts, _, pixels = ref.stabilize(shaken[w0:w0 + n], rect, 8, anchor)
        got = np.stack([shifts["dy"], shifts["dx"]], 1)
        assert np.array_equal(got, -jitter[w0:w0 + n]), "window at frame %d" % w0
        assert np.array_equal(pixels, still[w0:w0 + n, ya:yb, xa:xb])
        assert (shifts["sad"] < shifts["sad_unshifted"])[np.any(got != 0, axis=1)].all()
        if reanchor:
            anchor = ref.gray(pixels[-1])


@pytest.mark.parametrize("chroma", ["444", "420"])
def test_restatement_recovers_the_jitter_after_the_yuv_round_trip(chroma):
    """the clips the GPU tests write as .y4m files (stabilize_ref.yuv_planes) and read back as BGR: first window"""
    from swiftwatcher_amd.io_y4m import yuv_rect_to_bgr
    shaken, still, jitter = ref.shaken_clip()
    H, W = ref.CLIP["frame_hw"]
    s = 0 if chroma == "444" else 1

    def back(frame):
        return yuv_rect_to_bgr(*ref.yuv_planes(frame, chroma), 0, H, 0, W, sx=s, sy=s)
    (ya, yb, xa, xb), _ = _margin_and_search()
    got_shaken = np.stack([back(f) for f in shaken[:21]])
    got_still = np.stack([back(f) for f in still[:21]])
    shifts, _, pixels = ref.stabilize(got_shaken, (ya, xa, yb - ya, xb - xa), 8, ref.gray(got_shaken[0][ya:yb, xa:xb]))
    assert np.array_equal(np.stack([shifts["dy"], shifts["dx"]], 1), -jitter[:21])
    assert np.array_equal(pixels, got_still[:, ya:yb, xa:xb])


# ------------------------------------------------------------------ 3. StabilizingReader over the restatement
def _reader(frames, **kw):
    from swiftwatcher_amd.io_frames import ArrayReader
    from swiftwatcher_amd.stabilize import StabilizingReader
    backend = ref.RefBackend()
    return StabilizingReader(ArrayReader(list(frames)), ref.CLIP["crop_region"], backend=backend, **kw), backend


@pytest.mark.parametrize("reanchor", [0, 1, 2])
def test_reader_hands_out_the_still_clip(reanchor):
    from swiftwatcher_amd.io_frames import ArrayReader
    from swiftwatcher_amd.io_roi_stream import RoiFrame
    shaken, still, jitter = ref.shaken_clip()
    total, n = len(shaken), 21
    reader, backend = _reader(shaken, search=8, reanchor=reanchor)
    plain = ArrayReader(list(still))
    (ya, yb, xa, xb), _ = _margin_and_search()
    (x0, y0), (x1, y1) = ref.CLIP["crop_region"]
    assert reader.total_frames == total and reader.fps == plain.fps
    assert reader.read_frame(0, increment=False) is reader.reader.frames[0]          # the unshifted first frame
    windows = 0
    while reader.next_frame_number <= total:
        frames, numbers, stamps = reader.get_n_frames(n)
        want_frames, want_numbers, want_stamps = plain.get_n_frames(n)
        windows += 1
        assert numbers == want_numbers and stamps == want_stamps
        for fr, wf, num in zip(frames, want_frames, numbers):
            assert isinstance(fr, RoiFrame) and fr.origin == (ya, xa) and fr.shape == (110, 160, 3) and fr.block is None
            assert np.array_equal(fr[ya:yb, xa:xb], wf[ya:yb, xa:xb]), "frame %d" % num
            assert np.array_equal(fr[y0:y1, x0:x1], wf[y0:y1, x0:x1])
            if num < 0:
                assert not fr.roi.any()
    assert windows == 3 and backend.calls == 3
    # numbers 0 .. total: the frame one past the end is the last one again (read_errors), then nulls
    assert numbers[:11] == list(range(42, 53)) and numbers[11:] == [-1] * 10
    assert (reader.frames_read, reader.read_errors) == (plain.frames_read, plain.read_errors) == (total, 1)
    assert sorted(reader.shifts) == list(range(total + 1))
    for k in range(total + 1):
        jy, jx = jitter[min(k, total - 1)]
        dy, dx, sad, sad0 = reader.shifts[k]
        assert (dy, dx) == (-jy, -jx) and sad <= sad0
    assert reader.windows == 3


def test_reader_anchor_replacement():
    shaken, still, _ = ref.shaken_clip()
    (ya, yb, xa, xb), _ = _margin_and_search()
    first = ref.gray(still[0][ya:yb, xa:xb])
    fixed, _ = _reader(shaken, reanchor=0)
    moving, _ = _reader(shaken, reanchor=1)
    every2, _ = _reader(shaken, reanchor=2)
    for r in (fixed, moving, every2):
        r.get_n_frames(21)
    assert np.array_equal(fixed.anchor, first) and np.array_equal(every2.anchor, first)
    assert np.array_equal(moving.anchor, ref.gray(still[20][ya:yb, xa:xb]))
    every2.get_n_frames(21)
    assert np.array_equal(every2.anchor, ref.gray(still[41][ya:yb, xa:xb]))


def test_reader_clips_the_search_rectangle_to_the_picture():
    from swiftwatcher_amd.stabilize import search_rect
    margin, search = search_rect((110, 160), [(30, 20), (126, 84)], 8)
    assert margin == (8, 96, 18, 138) and search == (0, 104, 10, 146)
    margin, search = search_rect((110, 160), [(30, 20), (126, 84)], 16)
    assert search == (0, 110, 2, 154)
    margin, search = search_rect((90, 130), [(30, 20), (126, 84)], 16)
    assert margin == (8, 90, 18, 130) and search == (0, 90, 2, 130)


def test_reader_value_errors(tmp_path):
    from swiftwatcher_amd import io_roi_stream
    from swiftwatcher_amd.io_frames import ArrayReader
    from swiftwatcher_amd.stabilize import StabilizingReader, search_range
    shaken, _, _ = ref.shaken_clip()
    crop = ref.CLIP["crop_region"]
    with pytest.raises(ValueError, match="search"):
        StabilizingReader(ArrayReader(list(shaken[:3])), crop, search=17, backend=ref.RefBackend())
    with pytest.raises(ValueError, match="reanchor"):
        StabilizingReader(ArrayReader(list(shaken[:3])), crop, reanchor=-1, backend=ref.RefBackend())
    path = str(tmp_path / "clip.roi")
    io_roi_stream.write_roi_stream(path, list(shaken[:3]), crop)
    roi_reader = io_roi_stream.RoiStreamReader(path, prefetch=False)
    try:
        with pytest.raises(ValueError, match="ROI stream"):
            StabilizingReader(roi_reader, crop, backend=ref.RefBackend())
    finally:
        roi_reader.close()
    r = StabilizingReader(ArrayReader(list(shaken[:3])), crop, backend=ref.RefBackend())
    assert not hasattr(r, "ahead") and not hasattr(r, "set_region")                  # ArrayReader neither reads ahead nor takes a region
    assert [search_range(v) for v in (None, False, 0, True, 1, 16)] == [0, 0, 0, 8, 1, 16]
    with pytest.raises(ValueError):
        search_range(17)


def _y4m_pipe(tmp_path, frames):
    """a Y4MStreamReader over the bytes of a mono .y4m written by hand (no conversion needed on the host)"""
    from swiftwatcher_amd.io_y4m import Y4MStreamReader
    H, W = frames.shape[1:3]
    path = tmp_path / "pipe.y4m"
    with open(path, "wb") as fh:
        fh.write(b"YUV4MPEG2 W%d H%d F30:1 Ip Cmono\n" % (W, H))
        for f in frames:
            fh.write(b"FRAME\n" + ref.gray(f).tobytes())
    return Y4MStreamReader(open(path, "rb"), ahead=0)


def test_stream_reader_is_asked_for_the_grown_rectangle(tmp_path):
    from swiftwatcher_amd.stabilize import StabilizingReader
    shaken, _, _ = ref.shaken_clip()
    crop = ref.CLIP["crop_region"]
    inner = _y4m_pipe(tmp_path, shaken[:4])
    try:
        r = StabilizingReader(inner, crop, search=8, backend=ref.RefBackend())
        assert inner.min_seg_size == (40, 40) and inner._rect == (0, 104, 10, 146)
        r.set_region(crop, (24, 24))                                                 # the counting loop's call: accepted as it is
        assert inner.min_seg_size == (40, 40)
        with pytest.raises(ValueError, match="one crop region"):
            r.set_region([(31, 20), (127, 84)], (24, 24))
        r.ahead = 3
        assert inner.ahead == 3 and r.ahead == 3
    finally:
        inner.close()
    inner = _y4m_pipe(tmp_path, shaken[:4])
    try:
        inner.set_region(crop, (24, 24))
        inner.get_n_frames(2)                                                        # the smaller rectangle is fixed now
        with pytest.raises(ValueError, match="already fixed"):
            StabilizingReader(inner, crop, search=8, backend=ref.RefBackend())
    finally:
        inner.close()


def test_reader_recovers_the_jitter_at_the_clis_regions():
    """the clip as the CLI test on the GPU counts it: written as 8-bit 4:2:0, the crop region from --corners on its first frame"""
    from swiftwatcher_amd import image_filtering as img
    from swiftwatcher_amd.io_frames import ArrayReader
    from swiftwatcher_amd.stabilize import StabilizingReader
    shaken, still, jitter = ref.shaken_clip()
    total = len(shaken)
    got_shaken = ref.yuv420_round_trip(shaken)
    crop, _, _ = img.generate_regions(got_shaken[0], ref.CORNERS)
    (x0, y0), (x1, y1) = crop
    assert 0 <= x0 < x1 <= 160 and 0 <= y0 < y1 <= 110 and (x1 - x0, y1 - y0) != (96, 64)
    reader = StabilizingReader(ArrayReader(list(got_shaken)), crop, search=8, backend=ref.RefBackend())
    while reader.next_frame_number <= total:
        reader.get_n_frames(21)
    assert [reader.shifts[k][:2] for k in range(total)] == [(-jy, -jx) for jy, jx in jitter]


# ------------------------------------------------------------------ 4. the CLI
def test_cli_option_parsing(capsys):
    from swiftwatcher_amd.__main__ import plan
    base = ["clip.y4m", "--corners", "1,2,3,4"]
    assert plan(base)[0].stabilize == 0
    assert plan(base + ["--stabilize"])[0].stabilize == 8
    assert plan(base + ["--stabilize", "12"])[0].stabilize == 12
    assert plan(["--stabilize", "--corners", "1,2,3,4", "clip.y4m"])[0].stabilize == 8
    for bad in ("0", "17", "x"):
        with pytest.raises(SystemExit) as exc:
            plan(base + ["--stabilize", bad])
        assert exc.value.code == 2
    capsys.readouterr()


def test_csv_and_summary(tmp_path):
    from swiftwatcher_amd.stabilize import CSV_COLUMNS, summary, write_csv
    shifts = {2: (0, 0, 5, 5), 0: (0, 0, 0, 0), 1: (-3, 2, 40, 900), 3: (1, -5, 7, 90)}
    path = tmp_path / "stabilization.csv"
    write_csv(str(path), shifts)
    with open(path, newline="") as fh:
        rows = list(csv.reader(fh))
    assert tuple(rows[0]) == CSV_COLUMNS == ("frame_number", "dy", "dx", "sad", "sad_unshifted")
    assert len(rows) == 1 + len(shifts)
    assert [[int(x) for x in r] for r in rows[1:]] == [[k] + list(shifts[k]) for k in sorted(shifts)]
    assert summary(shifts, 8) == {"search": 8, "moved_frames": 2, "max_shift": 5}
    assert summary({}, 4) == {"search": 4, "moved_frames": 0, "max_shift": 0}
