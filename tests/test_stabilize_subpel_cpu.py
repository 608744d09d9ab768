"""The quarter-pixel stage of stabilization without a GPU: the filter and the numpy restatement of swk_stabilize_subpel_u8
(tests/stabilize_subpel_ref.py) on designed planes, the sub-pixel shaken scene that the GPU tests count (the restatement alone must
recover its jitter to a quarter pixel and leave the segment stage less than integer shifts do), stabilize.StabilizingReader with the
restatement injected in place of the GPU calls, and the pipeline's and the CLI's option, CSV columns and JSON entries."""
import csv
import os
import re

import numpy as np
import pytest

import stabilize_ref as ref1
import stabilize_subpel_ref as ref
from swiftwatcher_amd._lib import STABILIZE_SUBPEL_TILE, SUBSHIFT_DTYPE          # (the binding's side of what the restatement states)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _smooth_texture(seed, H, W):
    """(H, W, 3) uint8, all channels equal, smooth at the scale of a few pixels"""
    rng = np.random.default_rng(seed)
    a = ref1._smooth(rng.uniform(0, 1, size=(H, W)), 5)
    a = np.rint((a - a.min()) / (a.max() - a.min()) * 255).astype(np.uint8)
    return np.repeat(a[:, :, None], 3, 2)


# ------------------------------------------------------------------ 1. the filter
def test_filter_rows_sum_to_128_and_phase_0_is_the_identity():
    assert (ref.T.sum(axis=1) == 128).all() and ref.T.shape == (4, 4)
    assert np.array_equal(ref.T[3], ref.T[1][::-1]) and np.array_equal(ref.T[2], ref.T[2][::-1])
    rng = np.random.default_rng(1)
    for k in range(4):
        plane = rng.integers(0, 256, size=(23, 31), dtype=np.uint8)
        rect = (3, 4, 15, 20)
        for Qy, Qx in ((0, 0), (4, -8), (-12, 16)):
            assert np.array_equal(ref.resample(plane, rect, Qy, Qx), plane[3 + Qy // 4:18 + Qy // 4, 4 + Qx // 4:24 + Qx // 4])
    # phase 0 reads no neighbour: a rectangle that touches every edge of the plane
    assert np.array_equal(ref.resample(plane, (0, 0, 23, 31), 0, 0), plane)


def test_step_plane_reaches_the_clamp_and_v_stays_in_its_bound():
    plane = ref.step_plane(40, 50)[..., 0]
    rect = (5, 6, 28, 36)
    lo = hi = False
    worst = 0
    for Qy in range(-6, 7):
        for Qx in range(-6, 7):
            v = ref.resample_unclamped(plane, rect, Qy, Qx)
            worst = max(worst, int(np.abs(v).max()))
            r = (v + 8192) >> 14
            lo, hi = lo or bool((r < 0).any()), hi or bool((r > 255).any())
            out = ref.resample(plane, rect, Qy, Qx)
            assert out.dtype == np.uint8 and np.array_equal(out, np.clip(r, 0, 255))
    assert lo and hi
    assert 255 * 16384 < worst <= ref.V_BOUND < 1 << 23
    # the bound is that of the taps on pixels of 0..255: positive taps sum to at most 144, negative ones to -16 (phase 2), and the
    # plane that is 255 exactly where the product of the two taps is positive attains it
    assert max(int(t[t > 0].sum()) for t in ref.T) == 144 and min(int(t[t < 0].sum()) for t in ref.T) == -16
    sign = np.where(ref.T[2] > 0, 1, -1)
    extreme = np.where(np.outer(sign, sign) > 0, 255, 0)
    assert int(ref.resample_unclamped(extreme, (1, 1, 1, 1), 2, 2)[0, 0]) == ref.V_BOUND
    assert int(ref.resample_unclamped(255 - extreme, (1, 1, 1, 1), 2, 2)[0, 0]) == -2 * 144 * 16 * 255
    rng = np.random.default_rng(2)
    noise = rng.integers(0, 2, size=(40, 50)) * 255
    assert max(int(np.abs(ref.resample_unclamped(noise, rect, Qy, Qx)).max()) for Qy in (1, 2, 3) for Qx in (1, 2, 3)) <= ref.V_BOUND


# ------------------------------------------------------------------ 2. the restatement on designed planes
@pytest.mark.parametrize("Q", [(0, 0), (4, -8), (5, -6), (-3, 2), (1, 1), (-7, 7), (2, 0), (0, -9)])
def test_resampled_texture_is_matched_back_with_score_zero(Q):
    """the anchor is the texture resampled at (Qy, Qx) by the defined filter: that candidate scores 0 and is chosen"""
    frame = _smooth_texture(3, 70, 80)
    y0, x0, Ho, Wo, S = 12, 14, 40, 48, 3
    rect = (y0, x0, Ho, Wo)
    anchor = ref.resample(frame[..., 0], rect, *Q)
    recs, (table, sub), pixels = ref.stabilize_subpel(frame[None], rect, S, anchor)
    r = recs[0]
    assert (int(r["qy_total"]), int(r["qx_total"]), int(r["sad"])) == (Q[0], Q[1], 0)
    assert abs(4 * int(r["dy"]) - Q[0]) <= 2 and abs(4 * int(r["dx"]) - Q[1]) <= 2
    assert int(r["sad_int"]) == int(table[0, int(r["dy"]) + S, int(r["dx"]) + S]) == int(sub[0, 2, 2])
    assert int(r["sad_unshifted"]) == int(table[0, S, S])
    assert np.array_equal(pixels[0], np.repeat(anchor[:, :, None], 3, 2))
    if Q[0] % 4 == 0 and Q[1] % 4 == 0:                # a whole number of pixels: stage 1 finds it, stage 2 stays, the pixels are a copy
        assert (int(r["dy"]), int(r["dx"])) == (Q[0] // 4, Q[1] // 4) and int(r["sad_int"]) == 0
        assert np.array_equal(pixels[0], frame[y0 + Q[0] // 4:y0 + Q[0] // 4 + Ho, x0 + Q[1] // 4:x0 + Q[1] // 4 + Wo])
        assert np.array_equal(pixels[0], ref1.stabilize(frame[None], rect, S, anchor)[2][0])
    else:
        assert int(r["sad_int"]) > 0


def test_flat_frame_gives_no_shift():
    frame = np.full((1, 40, 50, 3), 90, np.uint8)
    anchor = np.full((20, 30), 120, np.uint8)
    recs, (_, sub), pixels = ref.stabilize_subpel(frame, (10, 10, 20, 30), 8, anchor)
    r = recs[0]
    assert (int(r["dy"]), int(r["dx"]), int(r["qy_total"]), int(r["qx_total"])) == (0, 0, 0, 0)
    assert len(np.unique(sub[0])) == 1 and int(r["sad"]) == int(r["sad_int"]) == int(r["sad_unshifted"]) == 20 * 30 * 30
    assert (pixels == 90).all()
    # the rule's order on a hand-made table around (dy, dx) = (1, -1): equal scores -> the smallest Qy^2 + Qx^2, then Qy, then Qx
    t = np.full((5, 5), 7, np.uint64)
    assert ref.choose(t, 1, -1) == (2, -2)
    assert ref.choose(t, 0, 0) == (0, 0)
    t[2, 2] = 9
    assert ref.choose(t, 0, 0) == (-1, 0)                # norm 1: (-1, 0), (0, -1), (0, 1), (1, 0)
    t[1, 2] = 9
    assert ref.choose(t, 0, 0) == (0, -1)
    t[:] = ref.EXCLUDED
    t[2, 2], t[4, 4] = 5, 5
    assert ref.choose(t, 0, 0) == (0, 0)


def test_null_frames_are_not_matched():
    frames = np.stack([_smooth_texture(4, 40, 50), np.zeros((40, 50, 3), np.uint8)])
    rect = (8, 9, 20, 24)
    anchor = ref.resample(frames[0][..., 0], rect, 3, -5)
    recs, _, pixels = ref.stabilize_subpel(frames, rect, 4, anchor)
    assert (int(recs[0]["qy_total"]), int(recs[0]["qx_total"]), int(recs[0]["sad"])) == (3, -5, 0)
    r = recs[1]
    assert (int(r["dy"]), int(r["dx"]), int(r["qy_total"]), int(r["qx_total"])) == (0, 0, 0, 0)
    assert int(r["sad"]) == int(r["sad_int"]) == int(r["sad_unshifted"]) == int(anchor.astype(np.int64).sum())
    assert not pixels[1].any()


LOW = {0: {-2, -1, 1, 2}, 1: {-2, -1}, 2: set()}           # q excluded on an axis whose rectangle lies so far from the top / left edge
HIGH = {0: {-2, -1, 1, 2}, 1: {1, 2}, 2: set()}            # ... from the bottom / right edge


@pytest.mark.parametrize("gap", [0, 1, 2])
@pytest.mark.parametrize("edge", ["top", "bottom", "left", "right"])
def test_exactly_the_footprint_rule_excludes(edge, gap):
    """the frame shows the anchor where the rectangle lies, so stage 1's winner is (0, 0) and the 25 candidates are q itself"""
    Hs, Ws, Ho, Wo, S = 40, 50, 20, 24, 2
    y0 = gap if edge == "top" else Hs - Ho - gap if edge == "bottom" else 9
    x0 = gap if edge == "left" else Ws - Wo - gap if edge == "right" else 11
    frame = _smooth_texture(5, Hs, Ws)
    rect = (y0, x0, Ho, Wo)
    anchor = ref1.gray(frame[y0:y0 + Ho, x0:x0 + Wo])
    recs, (_, sub), _ = ref.stabilize_subpel(frame[None], rect, S, anchor)
    assert (int(recs[0]["dy"]), int(recs[0]["dx"]), int(recs[0]["qy_total"]), int(recs[0]["qx_total"]), int(recs[0]["sad"])) == (0, 0, 0, 0, 0)
    bad_y = LOW[gap] if edge == "top" else HIGH[gap] if edge == "bottom" else set()
    bad_x = LOW[gap] if edge == "left" else HIGH[gap] if edge == "right" else set()
    want = np.array([[qy in bad_y or qx in bad_x for qx in range(-2, 3)] for qy in range(-2, 3)])
    assert np.array_equal(sub[0] == ref.EXCLUDED, want)
    assert sub[0, 2, 2] != ref.EXCLUDED


def test_exclusions_around_a_winner_at_the_edge():
    """the rectangle 1 px below the top edge and the scene 1 px further up: stage 1 wins at dy = -1, the last row inside; of the
    quarter-pixel candidates only qy = 0 keeps its rectangle inside, and q = (0, 0) stays"""
    Hs, Ws, Ho, Wo = 40, 50, 20, 24
    frame = _smooth_texture(6, Hs, Ws)
    anchor = ref1.gray(frame[0:Ho, 11:11 + Wo])
    recs, (_, sub), pixels = ref.stabilize_subpel(frame[None], (1, 11, Ho, Wo), 2, anchor)
    assert (int(recs[0]["dy"]), int(recs[0]["dx"]), int(recs[0]["qy_total"]), int(recs[0]["qx_total"])) == (-1, 0, -4, 0)
    assert np.array_equal(sub[0] == ref.EXCLUDED, np.array([[qy != 0] * 5 for qy in range(-2, 3)]))
    assert np.array_equal(pixels[0], frame[0:Ho, 11:11 + Wo])


def test_kernel_tile_constants_are_the_bindings():
    """the GPU tests name their shapes from _lib.STABILIZE_SUBPEL_TILE: it must be the score kernel's tile"""
    with open(os.path.join(ROOT, "swiftwatcher_amd", "csrc", "stabilize.hip")) as fh:
        m = re.search(r"constexpr int kSubRows = (\d+), kSubCols = (\d+)", fh.read())
    assert (int(m.group(1)), int(m.group(2))) == tuple(STABILIZE_SUBPEL_TILE)
    assert SUBSHIFT_DTYPE == ref.SUBSHIFT_DTYPE and SUBSHIFT_DTYPE.itemsize == 40


# ------------------------------------------------------------------ 3. the rendered scene
S = 5
CROP = ref.CLIP["crop_region"]


def _rects(grow):
    from swiftwatcher_amd.stabilize import search_rect
    return search_rect(ref.CLIP["frame_hw"], CROP, grow)


def _stabilized_clip(subpel):
    """the restatement on the whole clip against the first frame's grey: (records or shifts, pixels)"""
    shaken, _, _ = ref.subpel_clip()
    (ya, yb, xa, xb), (sa, sb, ta, tb) = _rects(S + 2)
    src = shaken[:, sa:sb, ta:tb]
    rect = (ya - sa, xa - ta, yb - ya, xb - xa)
    anchor = ref1.gray(shaken[0][ya:yb, xa:xb])
    if subpel:
        recs, _, pixels = ref.stabilize_subpel(src, rect, S, anchor)
    else:
        recs, _, pixels = ref1.stabilize(src, rect, S, anchor)
    return recs, pixels, anchor


def test_scene_is_what_it_says():
    shaken, still, jitter = ref.subpel_clip()
    assert shaken.shape == still.shape == (52, 110, 160, 3) and 0.35 <= ref.SIGMA <= 0.6
    assert (jitter[0] == 0).all() and np.abs(jitter).max() == ref.JITTER_Q and len({tuple(j % 4) for j in jitter}) >= 12
    assert np.array_equal(shaken[0], still[0])
    moved = [k for k in range(52) if jitter[k].any()]
    assert all(not np.array_equal(shaken[k], still[k]) for k in moved)
    # a frame at a whole number of pixels is the still frame moved (same noise field aside): the scene moves, not the camera's grid
    _, _, jit_int = ref.subpel_clip(total=8, noise=0.0, integer_jitter=True)
    sh_int, st_int, _ = ref.subpel_clip(total=8, noise=0.0, integer_jitter=True)
    for k in range(1, 8):
        jy, jx = jit_int[k] // 4
        assert np.array_equal(sh_int[k][10:100, 10:150], st_int[k][10 + jy:100 + jy, 10 + jx:150 + jx])


def test_restatement_recovers_the_jitter_to_a_quarter_pixel():
    _, _, jitter = ref.subpel_clip()
    recs, _, _ = _stabilized_clip(True)
    Q = np.stack([recs["qy_total"], recs["qx_total"]], 1).astype(np.int64)
    err = np.abs(Q + jitter)
    exact = int((err.sum(axis=1) == 0).sum())
    print("frames whose quarter-pixel jitter is recovered exactly: %d of %d; largest error %d quarter pixels" % (exact, len(Q), err.max()))
    assert err.max() <= 1                                # the condition: within a quarter pixel per axis, every frame
    assert exact >= 52                                   # observed: 52 of 52
    assert (np.abs(4 * recs["dy"].astype(np.int64) + jitter[:, 0]) <= 2).all() and (np.abs(4 * recs["dx"].astype(np.int64) + jitter[:, 1]) <= 2).all()
    assert (recs["sad"] <= recs["sad_int"]).all() and (recs["sad_int"] <= recs["sad_unshifted"]).all()


def test_quarter_pixel_stage_leaves_fewer_pixels_above_the_threshold():
    """|anchor - stabilized grey| > 15, the segment stage's threshold on the sparse term, over the bird-free frames"""
    _, pix2, anchor = _stabilized_clip(True)
    _, pix1, _ = _stabilized_clip(False)
    a = anchor.astype(np.int64)
    n = ref.BIRD_FREE
    over1 = int((np.abs(a - ref1.gray(pix1[:n]).astype(np.int64)) > 15).sum())
    over2 = int((np.abs(a - ref1.gray(pix2[:n]).astype(np.int64)) > 15).sum())
    print("pixels above 15 over %d bird-free frames: integer stage %d, quarter-pixel stage %d" % (n, over1, over2))
    assert over2 < over1 and over1 > 100


def _pasted(subpel):
    """full frames with the stabilized rectangles (StabilizingReader over the restatement, as the counting loop reads) at their
    unshifted place, and the reader"""
    from swiftwatcher_amd.io_frames import ArrayReader
    from swiftwatcher_amd.stabilize import StabilizingReader
    shaken, _, _ = ref.subpel_clip()
    total = len(shaken)
    reader = StabilizingReader(ArrayReader(list(shaken)), CROP, S, backend=ref.RefSubpelBackend(), subpel=subpel)
    out = np.array(shaken)
    while reader.next_frame_number <= total:
        frames, numbers, _ = reader.get_n_frames(21)
        for fr, num in zip(frames, numbers):
            if 0 <= num < total:
                (ya, xa), (h, w) = fr.origin, fr.roi.shape[:2]
                out[num, ya:ya + h, xa:xa + w] = fr.roi
    return out, reader


def test_segment_stage_finds_fewer_segments_after_the_quarter_pixel_stage():
    from oracle.pipeline_ref import oracle_frames
    _, still, _ = ref.subpel_clip()
    counts = [sum(len(info["segments"]) for info in oracle_frames(clip, CROP)) for clip in (_pasted(False)[0], _pasted(True)[0], still)]
    print("segments of the oracle's segment stage: integer stage %d, quarter-pixel stage %d, still twin %d" % tuple(counts))
    assert counts[1] < counts[0]


# ------------------------------------------------------------------ 4. StabilizingReader over the restatement
def test_reader_without_subpel_makes_todays_calls():
    """subpel=False with the backend that has both methods: stabilize alone is called, with the arguments and the bytes that the
    reader over stabilize_ref.RefBackend (which has no other method) gets"""
    from swiftwatcher_amd.io_frames import ArrayReader
    from swiftwatcher_amd.stabilize import StabilizingReader
    shaken, _, _ = ref.subpel_clip()
    total = len(shaken)
    old_backend, new_backend = ref1.RefBackend(), ref.RefSubpelBackend()
    old = StabilizingReader(ArrayReader(list(shaken)), CROP, S, backend=old_backend)
    new = StabilizingReader(ArrayReader(list(shaken)), CROP, S, backend=new_backend, subpel=False)
    while old.next_frame_number <= total:
        f_old, n_old, s_old = old.get_n_frames(21)
        f_new, n_new, s_new = new.get_n_frames(21)
        assert n_old == n_new and s_old == s_new
        for a, b in zip(f_old, f_new):
            assert a.origin == b.origin and np.array_equal(a.roi, b.roi)
    assert (old_backend.calls, new_backend.calls, new_backend.subpel_calls) == (3, 3, 0)
    assert old.shifts == new.shifts and new.subshifts == {} and not new.subpel and new.grow == S
    (ya, yb, xa, xb), (sa, sb, ta, tb) = _rects(S)
    assert new_backend.rects == [((sb - sa, tb - ta), (ya - sa, xa - ta, yb - ya, xb - xa))] * 3


@pytest.mark.parametrize("reanchor", [0, 1, 2])
def test_reader_with_subpel(reanchor):
    from swiftwatcher_amd.io_frames import ArrayReader
    from swiftwatcher_amd.stabilize import StabilizingReader
    shaken, _, jitter = ref.subpel_clip()
    total = len(shaken)
    backend = ref.RefSubpelBackend()
    reader = StabilizingReader(ArrayReader(list(shaken)), CROP, S, backend=backend, subpel=True, reanchor=reanchor)
    assert reader.subpel and reader.grow == S + 2
    (ya, yb, xa, xb), (sa, sb, ta, tb) = _rects(S + 2)
    assert (sa, sb, ta, tb) == (ya - 7, yb + 7, xa - 7, xb + 7)
    rect = (ya - sa, xa - ta, yb - ya, xb - xa)
    anchor = ref1.gray(shaken[0][ya:yb, xa:xb])
    windows = 0
    while reader.next_frame_number <= total:
        assert np.array_equal(reader.anchor, anchor) or windows == 0
        frames, numbers, _ = reader.get_n_frames(21)
        real = [k for k, num in enumerate(numbers) if num >= 0]
        src = np.stack([shaken[min(numbers[k], total - 1)][sa:sb, ta:tb] if numbers[k] >= 0 else np.zeros((sb - sa, tb - ta, 3), np.uint8)
                        for k in range(21)])
        recs, _, pixels = ref.stabilize_subpel(src, rect, S, anchor)
        for k in range(21):
            assert frames[k].origin == (ya, xa) and np.array_equal(frames[k].roi, pixels[k])
        for k in real:
            r = recs[k]
            assert reader.shifts[numbers[k]] == (int(r["dy"]), int(r["dx"]), int(r["sad_int"]), int(r["sad_unshifted"]))
            assert reader.subshifts[numbers[k]] == (int(r["qy_total"]), int(r["qx_total"]), int(r["sad"]))
        windows += 1
        if reanchor and windows % reanchor == 0:         # the rule: the grey of the newest stabilized frame, as handed out
            anchor = ref1.gray(pixels[real[-1]])
    assert windows == 3 and (backend.calls, backend.subpel_calls) == (0, 3)
    assert backend.rects == [((sb - sa, tb - ta), rect)] * 3
    assert sorted(reader.subshifts) == sorted(reader.shifts) == list(range(total + 1))
    for k in range(total):
        assert max(abs(reader.subshifts[k][0] + jitter[k][0]), abs(reader.subshifts[k][1] + jitter[k][1])) <= 1, "frame %d" % k


def test_reader_with_subpel_clips_at_the_picture_and_refuses_a_roi_stream(tmp_path):
    from swiftwatcher_amd import io_roi_stream
    from swiftwatcher_amd.io_frames import ArrayReader
    from swiftwatcher_amd.stabilize import StabilizingReader
    shaken, _, _ = ref.subpel_clip()
    backend = ref.RefSubpelBackend()
    reader = StabilizingReader(ArrayReader(list(shaken[:5])), CROP, 16, backend=backend, subpel=True)
    reader.get_n_frames(21)
    # the margin rectangle (8, 96, 18, 138) grown by 18 and clipped to 110 x 160
    assert backend.rects == [((110, 156), (8, 18, 88, 120))] and reader.grow == 18
    path = str(tmp_path / "clip.roi")
    io_roi_stream.write_roi_stream(path, list(shaken[:3]), CROP)
    roi_reader = io_roi_stream.RoiStreamReader(path, prefetch=False)
    try:
        with pytest.raises(ValueError, match="ROI stream"):
            StabilizingReader(roi_reader, CROP, backend=backend, subpel=True)
    finally:
        roi_reader.close()


def test_stream_reader_is_asked_for_the_footprints_margin(tmp_path):
    from swiftwatcher_amd.io_y4m import Y4MStreamReader
    from swiftwatcher_amd.stabilize import StabilizingReader
    shaken, _, _ = ref.subpel_clip()
    path = tmp_path / "pipe.y4m"
    with open(path, "wb") as fh:
        fh.write(b"YUV4MPEG2 W160 H110 F30:1 Ip Cmono\n")
        for f in shaken[:4]:
            fh.write(b"FRAME\n" + ref1.gray(f).tobytes())
    for subpel, grown, held in ((False, 24 + 2 * 8, (0, 104, 10, 146)), (True, 24 + 2 * 10, (0, 106, 8, 148))):
        inner = Y4MStreamReader(open(path, "rb"), ahead=0)
        try:
            StabilizingReader(inner, CROP, search=8, backend=ref.RefSubpelBackend(), subpel=subpel)
            assert inner.min_seg_size == (grown, grown) and inner._rect == held
        finally:
            inner.close()


# ------------------------------------------------------------------ 5. the pipeline and the CLI
def test_pipeline_refuses_subpel_without_stabilize():
    from swiftwatcher_amd import pipeline
    shaken, _, _ = ref.subpel_clip()
    mask = np.full((64, 96), 255, np.uint8)
    with pytest.raises(ValueError, match="stabilize_subpel"):
        pipeline.count_swifts(list(shaken[:3]), CROP, mask, stabilize_subpel=True)
    with pytest.raises(ValueError, match="stabilize_subpel"):
        pipeline.count_swifts(list(shaken[:3]), CROP, mask, stabilize=0, stabilize_subpel=True)
    with pytest.raises(ValueError, match="stabilize_subpel"):
        pipeline.count_swifts_videos([shaken[:3]], regions=[(CROP, mask)], stabilize_subpel=True)
    from swiftwatcher_amd.io_frames import ArrayReader
    wrapped = pipeline._stabilized(ArrayReader(list(shaken[:3])), CROP, True, (24, 24), 0, None, True)
    assert wrapped.subpel and wrapped.search == 8 and wrapped.grow == 10
    assert not pipeline._stabilized(ArrayReader(list(shaken[:3])), CROP, 4, (24, 24), 0, None).subpel


def test_cli_option_parsing(capsys):
    from swiftwatcher_amd.__main__ import plan
    base = ["clip.y4m", "--corners", "1,2,3,4"]
    assert plan(base)[0].stabilize_subpel is False
    assert plan(base + ["--stabilize"])[0].stabilize_subpel is False
    args = plan(base + ["--stabilize", "--stabilize-subpel"])[0]
    assert args.stabilize == 8 and args.stabilize_subpel is True
    args = plan(["--stabilize-subpel", "--stabilize", "12"] + base)[0]
    assert args.stabilize == 12 and args.stabilize_subpel is True
    with pytest.raises(SystemExit) as exc:
        plan(base + ["--stabilize-subpel"])
    assert exc.value.code == 2
    assert "--stabilize-subpel needs --stabilize" in capsys.readouterr().err


def test_csv_and_summary(tmp_path):
    from swiftwatcher_amd.stabilize import CSV_COLUMNS, CSV_SUBPEL_COLUMNS, quarter_text, summary, write_csv
    shifts = {2: (0, 0, 5, 5), 0: (0, 0, 0, 0), 1: (-3, 2, 40, 900), 3: (1, -5, 7, 90)}
    sub = {2: (1, 0, 4), 0: (0, 0, 0), 1: (-12, 8, 40), 3: (5, -22, 6)}
    off, on = tmp_path / "off.csv", tmp_path / "on.csv"
    write_csv(str(off), shifts)
    write_csv(str(on), shifts, sub)
    with open(off, newline="") as fh:
        rows_off = list(csv.reader(fh))
    with open(on, newline="") as fh:
        rows_on = list(csv.reader(fh))
    assert tuple(rows_off[0]) == CSV_COLUMNS == ("frame_number", "dy", "dx", "sad", "sad_unshifted")
    assert tuple(rows_on[0]) == CSV_COLUMNS + CSV_SUBPEL_COLUMNS == CSV_COLUMNS + ("shift_y", "shift_x", "sad_subpel")
    assert [r[:5] for r in rows_on] == rows_off
    assert [r[5:] for r in rows_on[1:]] == [["0.00", "0.00", "0"], ["-3.00", "2.00", "40"], ["0.25", "0.00", "4"], ["1.25", "-5.50", "6"]]
    assert [quarter_text(q) for q in (-1, -3, -4, -5, 0, 3, 66)] == ["-0.25", "-0.75", "-1.00", "-1.25", "0.00", "0.75", "16.50"]
    assert summary(shifts, 8) == {"search": 8, "moved_frames": 2, "max_shift": 5}
    assert summary(shifts, 8, sub) == {"search": 8, "moved_frames": 2, "max_shift": 5, "subpel": True, "fractional_frames": 2}
    assert list(summary(shifts, 8, sub))[:3] == list(summary(shifts, 8))
    assert summary({}, 4, {}) == {"search": 4, "moved_frames": 0, "max_shift": 0, "subpel": True, "fractional_frames": 0}


def test_cli_outputs_on_and_off(tmp_path, capsys, monkeypatch):
    """main(argv) with the source opened as decoded frames and the GPU calls replaced by the restatement's backend: stabilization.csv
    and the JSON line with and without --stabilize-subpel (the counting loop itself is stubbed: this is about what the CLI writes)"""
    import json
    from swiftwatcher_amd import __main__ as cli
    from swiftwatcher_amd import io_y4m, pipeline, stabilize
    from swiftwatcher_amd.io_frames import ArrayReader
    shaken, _, jitter = ref.subpel_clip()
    clip = shaken[:12]
    path = str(tmp_path / "clip.y4m")
    monkeypatch.setattr(io_y4m, "open_y4m", lambda source, start=0, end=0: ArrayReader(list(clip)))
    init = stabilize.StabilizingReader.__init__
    made = []

    def with_backend(self, *a, **k):
        k["backend"] = ref.RefSubpelBackend()
        made.append(k.get("subpel", False))
        init(self, *a, **k)

    def read_all(reader, crop_region=None, roi_mask=None, **kw):
        while reader.next_frame_number <= reader.total_frames:
            reader.get_n_frames(21)
        return 0, []

    monkeypatch.setattr(stabilize.StabilizingReader, "__init__", with_backend)
    monkeypatch.setattr(pipeline, "count_swifts", read_all)
    corners = "%d,%d,%d,%d" % (ref1.CORNERS[0] + ref1.CORNERS[1])
    lines, tables = {}, {}
    for name, extra in (("off", []), ("on", ["--stabilize-subpel"])):
        out = tmp_path / name
        assert cli.main([path, "--corners", corners, "--stabilize", "5", "--out", str(out)] + extra) == 0
        lines[name] = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
        with open(out / "stabilization.csv", newline="") as fh:
            tables[name] = list(csv.reader(fh))
    assert made == [False, True]
    assert lines["off"]["stabilize"].keys() == {"search", "moved_frames", "max_shift"}
    assert lines["on"]["stabilize"].keys() == {"search", "moved_frames", "max_shift", "subpel", "fractional_frames"}
    assert lines["on"]["stabilize"]["subpel"] is True and lines["on"]["stabilize"]["search"] == 5
    assert tables["off"][0] == ["frame_number", "dy", "dx", "sad", "sad_unshifted"]
    assert tables["on"][0] == tables["off"][0] + ["shift_y", "shift_x", "sad_subpel"]
    rows = tables["on"][1:]
    assert [int(r[0]) for r in rows] == list(range(13))
    got = np.array([[float(r[5]), float(r[6])] for r in rows[:12]]) * 4
    assert np.abs(got + jitter[:12]).max() <= 1
    assert lines["on"]["stabilize"]["fractional_frames"] == sum(1 for r in rows if float(r[5]) % 1 or float(r[6]) % 1) > 6
    assert all(int(r[7]) <= int(r[3]) for r in rows)
