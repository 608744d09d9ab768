"""swk_batch_run / swk_batch_run_groups with the bilateral diameter and sigmas of swk_params (csrc/filters.hip, k_filter_fused<GEOM, R>,
R = 1..4; csrc/swk_api.hip, run_batch): every radius against the CPU oracle with the same overrides and against the stage functions
on the GPU, bit for bit on every pixel and every region record; groups; parameters that must not leak between calls; the refusals that
stay; the counting loop with params.

Scenes.  The larger ROIs are helpers.roi_stack windows with dark blobs placed on all four borders of every frame (birds that touch the
borders: the filter's BORDER_REFLECT_101 and the opening's edge handling decide pixels there).  The ROIs of 4 x 4, 5 x 7 and 4 x 130
pixels cannot use the reference's lambda = 0.01: with so few pixels the IALM's first shrinkage threshold (lambda ||X||_F / 1.25) lies
below the pixel values, the sparse term starts positive and the sparse image (clip(-E)) stays all zero whatever the frames hold --
pure random pixels included -- so the filter would see nothing.  They are random pixels that keep their place from frame to frame, with
dark blocks in some frames, run at a larger lambda (swk_params.lmbda, the oracle's lmbda) for which the oracle leaves a region at every
parameter set; seeds and lambdas were fixed from the oracle alone.  Every case asserts on the oracle's output that the scene exercises
the filter (a region somewhere, a bilateral image that differs from d = 7's, at most 255 components per frame)."""
import functools

import numpy as np
import pytest

from helpers import STAGES, check_against_lone, lone_run, orc_seg_tuples, roi_stack, seg_tuples

pytestmark = pytest.mark.gpu

# (bil_d, bil_sigma_color, bil_sigma_space): radius 1, 2, 4, 4, 1, 2 (from sigma), 3 (from sigma: another table than d = 7), 4 (from sigma)
BIL = [(3, 15.0, 1.0), (5, 15.0, 1.0), (9, 15.0, 1.0), (9, 40.0, 3.0), (2, 15.0, 1.0), (0, 15.0, 1.0), (0, 15.0, 2.0), (-1, 25.0, 2.5)]
BIL_IDS = ["d3", "d5", "d9", "d9_s40_3", "d2", "d0_ss1", "d0_ss2", "dneg_ss2.5"]

# tiny scenes: (seed, lmbda, drop, every, lo, hi, noise, block h, block w) per (H, W, n)
TINY = {(4, 4, 21): (0, 0.2, 150.0, 4, 150, 151, 0.5, 3, 3), (4, 4, 5): (21, 0.15, 230.0, 5, 230, 235, 1.5, 3, 3),
        (5, 7, 21): (9, 0.1, 120.0, 7, 100, 120, 3.0, 4, 4), (5, 7, 5): (5, 0.15, 150.0, 5, 150, 170, 1.5, 4, 3),
        (4, 130, 21): (1, 0.05, 90.0, 3, 150, 230, 1.5, 4, 5), (4, 130, 5): (1, 0.05, 90.0, 3, 150, 230, 1.5, 4, 5)}
# bordered scenes: (roi_stack seed, windows) per (H, W): 47 x 94 is no multiple of the 32 x 64 tile in either direction, 67 x 95 is
# wider than one tile with an odd width (rows start on every byte alignment)
LARGE = {(47, 94): (3100, 2), (67, 95): (3200, 1)}
SHAPES = [(47, 94), (67, 95), (4, 4), (5, 7), (4, 130)]
SHAPE_IDS = ["%dx%d" % s for s in SHAPES]


@pytest.fixture(scope="module")
def orc():
    from oracle import reference_path
    return reference_path


@pytest.fixture(scope="module")
def ctx():
    from swiftwatcher_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def _tiny_scene(n, H, W, seed, drop, every, lo, hi, noise, bh, bw):
    """random pixels that stay put from frame to frame + noise; every `every`-th frame holds a dark bh x bw block"""
    rng = np.random.default_rng(seed)
    base = rng.integers(lo, hi, size=(1, H, W, 1)).astype(np.float64)
    f = base + rng.normal(0.0, noise, size=(n, H, W, 3))
    for t in range(0, n, every):
        h, w = min(H, bh), min(W, bw)
        r, c = int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1))
        f[t, r:r + h, c:c + w] -= drop
    return np.clip(np.rint(f), 0, 255).astype(np.uint8)


def _bordered(roi, seed):
    """a dark 5 x 8 blob on each of the four borders of every frame, at a new place every frame"""
    rng = np.random.default_rng(seed)
    F, H, W = roi.shape[:3]
    f = roi.astype(np.float64)
    for t in range(F):
        a, b, c, d = (int(rng.integers(0, m - 8)) for m in (W, W, H, H))
        f[t, 0:5, a:a + 8] -= 70.0
        f[t, H - 5:H, b:b + 8] -= 70.0
        f[t, c:c + 8, 0:5] -= 70.0
        f[t, d:d + 8, W - 5:W] -= 70.0
    return np.clip(np.rint(f), 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def _scene(H, W, n):
    """(frames (nwin * n, H, W, 3), nwin, overrides beside the bilateral ones: oracle keywords = swk_params fields)"""
    if (H, W) in LARGE:
        seed, nwin = LARGE[(H, W)]
        return _bordered(roi_stack(seed + n, nwin, H, W, n=n), seed), nwin, {}
    seed, lmbda = TINY[(H, W, n)][:2]
    return _tiny_scene(n, H, W, seed, *TINY[(H, W, n)][2:]), 1, dict(lmbda=lmbda)


def _overrides(bil, fma):
    return dict(bil_d=bil[0], bil_sigma_color=bil[1], bil_sigma_space=bil[2], bil_fma=bool(fma))


def _params(over):
    from swiftwatcher_amd import _lib
    return _lib.default_params(**{k: int(v) if k == "bil_fma" else v for k, v in over.items()})


@functools.lru_cache(maxsize=None)
def _oracle_windows(H, W, n, bil, fma):
    """the oracle on every window of the scene, with the overrides (bil None: the scene at d = 7)"""
    from oracle import reference_path as orc
    roi, nwin, extra = _scene(H, W, n)
    over = dict(extra, **(_overrides(bil, fma) if bil is not None else {}))
    return [orc.window(np.ascontiguousarray(roi[w * n:(w + 1) * n]), **over) for w in range(nwin)]


def _assert_scene_exercises_the_filter(H, W, n, bil, fma):
    from oracle import reference_path as orc
    refs, d7 = _oracle_windows(H, W, n, bil, fma), _oracle_windows(H, W, n, None, 0)
    counts = [len(s) for ref in refs for s in ref["segments"]]
    assert max(counts) >= 1, "no frame has a region"
    assert max(int(ref["labels"].max()) for ref in refs) <= 255 and max(counts) <= 255
    for ref in refs:                    # u8 labels wrap above 255 components: count them on the opened image itself
        for img in ref["opened"]:
            assert orc.ccl_u8(img)[0] <= 255
    assert any(not np.array_equal(a["bilateral"], b["bilateral"]) for a, b in zip(refs, d7)), "the bilateral image equals d = 7's"


def _assert_equals_oracle(res, refs, n, what=""):
    for w, ref in enumerate(refs):
        for key in STAGES:
            assert np.array_equal(res[key][w * n:(w + 1) * n], ref[key]), "%s window %d: stage %s differs from the oracle" % (what, w, key)
        assert int(res["iters"][w]) == int(ref["iters"]), (what, w)
        for i in range(n):
            assert int(res["nseg"][w * n + i]) == len(ref["segments"][i]), (what, w, i)
            assert seg_tuples(res, w * n + i) == orc_seg_tuples(ref["segments"][i]), "%s window %d frame %d" % (what, w, i)


# ------------------------------------------------------------------ 1 + 2. every radius against the CPU oracle
@pytest.mark.parametrize("fma", [0, 1], ids=["mul_add", "fma"])
@pytest.mark.parametrize("bil", BIL, ids=BIL_IDS)
@pytest.mark.parametrize("n", [21, 5])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_batch_run_against_the_oracle(ctx, shape, n, bil, fma):
    H, W = shape
    _assert_scene_exercises_the_filter(H, W, n, bil, fma)
    roi, nwin, extra = _scene(H, W, n)
    res = ctx.batch_run(roi, nwin, n, params=_params(dict(extra, **_overrides(bil, fma))))
    _assert_equals_oracle(res, _oracle_windows(H, W, n, bil, fma), n)


def test_birds_touch_all_four_borders():
    """on the oracle's output alone: the bordered scenes leave regions on the first and last row and column, at radius 1 and 4"""
    for H, W in LARGE:
        for bil in (BIL[0], BIL[2]):
            lab = np.concatenate([ref["labels"] for ref in _oracle_windows(H, W, 21, bil, 0)])
            assert lab[:, 0].any() and lab[:, -1].any() and lab[:, :, 0].any() and lab[:, :, -1].any(), (H, W, bil)


# ------------------------------------------------------------------ 3. against the stage functions on the GPU
@pytest.mark.parametrize("fma", [0, 1], ids=["mul_add", "fma"])
@pytest.mark.parametrize("bil", BIL, ids=BIL_IDS)
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_batch_run_against_the_stage_functions(ctx, shape, bil, fma):
    H, W = shape
    roi, nwin, extra = _scene(H, W, 21)
    res = ctx.batch_run(roi, nwin, 21, params=_params(dict(extra, **_overrides(bil, fma))))
    assert res["rpca"].any()
    blur = ctx.bilateral_u8(res["rpca"], d=bil[0], sigma_color=bil[1], sigma_space=bil[2], use_fma=bool(fma))
    assert np.array_equal(res["bilateral"], blur)
    thr = ctx.thresh_tozero_u8(blur, 15)
    assert np.array_equal(res["thresh"], thr)
    assert np.array_equal(res["opened"], ctx.grey_open3x3_u8(thr))


# ------------------------------------------------------------------ 4. groups
@pytest.mark.parametrize("device_frames", [False, True], ids=["host_frames", "device_frames"])
@pytest.mark.parametrize("bil", [BIL[0], BIL[5], BIL[7]], ids=["radius1", "radius2", "radius4"])
def test_groups_take_the_radius(ctx, orc, bil, device_frames):
    """three geometries in one call (the per-frame-geometry instantiations): every group equals its lone run and the oracle"""
    n = 21
    rois = [_bordered(roi_stack(3300, 2, 40, 70), 3300), _bordered(roi_stack(3310, 1, 107, 214), 3310), roi_stack(3320, 1, 4, 9)]
    specs = [dict(frames=r, nwin=r.shape[0] // n, n=n) for r in rois]
    if device_frames:
        import torch
        specs = [dict(s, frames=torch.from_numpy(s["frames"]).cuda()) for s in specs]
    over = _overrides(bil, 0)
    got = ctx.batch_run_groups(specs, params=_params(over))
    assert len(got) == 3
    regions = 0
    for g, (spec, roi, res) in enumerate(zip(specs, rois, got)):
        check_against_lone(g, res, lone_run(ctx, spec, params=_params(over)), ae=False)
        refs = [orc.window(np.ascontiguousarray(roi[w * n:(w + 1) * n]), **over) for w in range(spec["nwin"])]
        _assert_equals_oracle(res, refs, n, "group %d" % g)
        regions += int(res["nseg"].sum())
    assert regions > 0
    assert not np.array_equal(got[1]["bilateral"], ctx.batch_run(rois[1], 1, n)["bilateral"])


# ------------------------------------------------------------------ 5. parameters do not leak between calls
def test_parameters_do_not_leak_between_calls(ctx, orc):
    n = 21
    roi, nwin, _ = _scene(67, 95, n)
    ref = orc.window(roi)
    runs = []
    for bil in (BIL[7], None, BIL[0], None):
        res = ctx.batch_run(roi, nwin, n, params=_params(_overrides(bil, 0)) if bil else None)
        if bil is None:
            runs.append(res)
        else:
            _assert_equals_oracle(res, _oracle_windows(67, 95, n, bil, 0), n)
    for key in STAGES + ("iters", "nseg", "segs"):
        assert np.array_equal(runs[0][key], runs[1][key]), key
    _assert_equals_oracle(runs[0], [ref], n, "defaults")


# ------------------------------------------------------------------ 6. refusals that stay
def test_refusals_that_stay(ctx, orc):
    from swiftwatcher_amd import _lib
    n = 5
    roi, nwin, _ = _scene(47, 94, n)
    with pytest.raises(_lib.SwkError):          # radius 5
        ctx.batch_run(roi, nwin, n, params=_lib.default_params(bil_d=11))
    with pytest.raises(_lib.SwkError):          # radius 6 from sigma_space
        ctx.batch_run(roi, nwin, n, params=_lib.default_params(bil_d=0, bil_sigma_color=15.0, bil_sigma_space=4.0))
    with pytest.raises(_lib.SwkError):          # only the (3, 3) opening exists
        ctx.batch_run(roi, nwin, n, params=_lib.default_params(open_kh=5))
    with pytest.raises(_lib.SwkError):
        ctx.batch_run_groups([dict(frames=roi, nwin=nwin, n=n), dict(frames=roi_stack(1, 1, 30, 40, n=n), nwin=1, n=n)],
                             params=_lib.default_params(bil_d=11))
    # the context still works, at a radius that is served and at the defaults
    _assert_equals_oracle(ctx.batch_run(roi, nwin, n, params=_params(_overrides(BIL[2], 0))), _oracle_windows(47, 94, n, BIL[2], 0), n)
    _assert_equals_oracle(ctx.batch_run(roi, nwin, n), _oracle_windows(47, 94, n, None, 0), n)


# ------------------------------------------------------------------ 7. the counting loop
@pytest.mark.parametrize("windows_per_call", [1, 2])
def test_counting_loop_with_params(orc, monkeypatch, windows_per_call):
    """pipeline.count_swifts(params=default_params(bil_d=5)) over 2 full windows + one padded with null frames: the segments the
    tracker is handed equal the oracle's at bil_d = 5, window by window as oracle.pipeline_ref.oracle_frames reads them"""
    from swiftwatcher_amd import _lib, pipeline, synthetic
    from swiftwatcher_amd.io_frames import ArrayReader
    crop_region = [(30, 20), (30 + 96, 20 + 64)]
    (x0, y0), (x1, y1) = crop_region
    total, n = 52, 21
    clip = synthetic.full_frames(4343, total, crop_region, frame_hw=(110, 160), birds=4, bird_len=(8, 12), bird_wid=(3, 5))[::-1].copy()
    roi_mask = np.zeros((64, 96), np.uint8)
    roi_mask[32:, 10:86] = 255
    seen = {}

    class Spy(pipeline.SegmentTracker):
        def set_current_frame(self, frame):
            if frame.frame_number >= 0:
                seen[frame.frame_number] = [(s.label, tuple(s.bbox), tuple(s.centroid), s.area) for s in frame.segments]
            super().set_current_frame(frame)

    monkeypatch.setattr(pipeline, "SegmentTracker", Spy)
    count, events = pipeline.count_swifts(list(clip), crop_region, roi_mask, params=_lib.default_params(bil_d=5),
                                          windows_per_call=windows_per_call)
    reader = ArrayReader(list(clip))
    processed, expected, differs = 0, {}, False
    while processed < reader.total_frames:
        frames, numbers, _ = reader.get_n_frames(n)
        roi = np.ascontiguousarray(np.stack([f[y0:y1, x0:x1] for f in frames][::-1]))          # queue order: newest first
        ref, ref7 = orc.window(roi, bil_d=5), orc.window(roi)
        differs = differs or not np.array_equal(ref["bilateral"], ref7["bilateral"])
        for pos in range(n - 1, -1, -1):
            k = n - 1 - pos
            if numbers[k] >= 0:
                expected[numbers[k]] = [(s["label"], tuple(s["bbox"]), tuple(s["centroid"]), s["area"]) for s in ref["segments"][pos]]
                processed += 1
    # (the reader serves the frame one past the end once, as a copy of the last one, before the null frames: it is a real frame too)
    assert differs and set(range(total)) <= set(expected)
    assert sum(len(v) for v in expected.values()) > 50
    assert sorted(seen) == sorted(expected)
    for k in sorted(expected):
        assert seen[k] == expected[k], "frame %d" % k
