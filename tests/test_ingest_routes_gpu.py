"""Frame ingest of swk_batch_run / swk_batch_run_groups at every route (swk_api.hip: host_stage_plan / host_stage_copy; filters.hip:
k_gray4, k_gray4g, k_gray; groups.hip: k_gray_groups).  One scene (helpers.SCENES) is embedded in many views (helpers.View): host
buffers that force each of the four staging routes, device buffers read in place, every residue mod 4 of the first ROI byte and of
the row stride.  For every view
  * the gray plane equals the numpy statement of BGR2GRAY on the scene (every byte outside the ROI is noise: a read outside shows),
  * every other product equals the run of the dense, contiguous scene on the same context, bit for bit,
  * swk_last_host_stage reports the route the view is named after.
The dense runs of the two scenes large enough for a LAPACK-independent oracle are held to the CPU oracle, all six stages and the
region records.  tests/test_ingest_scenes_cpu.py checks the scenes, views and tables themselves."""
import ctypes

import numpy as np
import pytest

from helpers import (ANCHORED, ROUTE_2D, ROUTE_DENSE, ROUTE_DEVICE, ROUTE_ROWS, ROUTE_WHOLE, SCENES, STAGES, View, alignment_views,
                     check_against_lone, gray_kernel, group_views, orc_seg_tuples, residue_table, route_views, scene, scene_gray,
                     seg_tuples)

pytestmark = pytest.mark.gpu

LATER = tuple(s for s in STAGES if s != "gray")


@pytest.fixture(scope="module")
def orc():
    from oracle import reference_path
    return reference_path


@pytest.fixture(scope="module")
def ctx():
    from swiftwatcher_amd import _lib
    c = _lib.Context(0)
    c._dense_runs = {}
    yield c
    c.close()


def _params(gray_mode):
    from swiftwatcher_amd import _lib
    return _lib.default_params(gray_mode=gray_mode)


def dense_run(ctx, name, gray_mode=0, ae=False):
    """the run of the dense, contiguous scene (host frames, host outputs), once per context"""
    key = (name, gray_mode, ae)
    if key not in ctx._dense_runs:
        _, nwin, n, _, _, _ = SCENES[name]
        res = ctx.batch_run(scene(name), nwin, n, params=_params(gray_mode), want_A=ae, want_E=ae)
        assert ctx.last_host_stage() == [ROUTE_DENSE]
        assert np.array_equal(res["gray"], scene_gray(name, gray_mode)), "%s: dense gray differs from numpy" % name
        if name in ANCHORED:          # (the smaller scenes hold regions in the oracle's output: test_ingest_scenes_cpu.py)
            assert int(res["nseg"].sum()) >= 1, name
        ctx._dense_runs[key] = res
    return ctx._dense_runs[key]


def run_view(ctx, view, ae=False):
    buf = view.buffer()
    if view.device:
        frames, alloc = view.device_array(buf)
        assert alloc.data_ptr() % 4 == 0 and frames.data_ptr() % 4 == view.base % 4
    else:
        frames = view.host_array(buf)
    res = ctx.batch_run(frames, view.nwin, view.n, crop=view.crop, reverse_frames=view.reverse, params=_params(view.gray_mode),
                        want_A=ae, want_E=ae)
    return res, ctx.last_host_stage()


def check_view(ctx, view, res, kinds, ae=False):
    assert kinds == [view.route], "%s took route %s" % (view.id, kinds)
    gray = scene_gray(view.scene, view.gray_mode)
    bad = np.argwhere(res["gray"] != gray)
    assert not len(bad), "%s: gray differs from numpy at %d pixels, first (frame, row, column) %s" % (view.id, len(bad), bad[0])
    ref = dense_run(ctx, view.scene, view.gray_mode, ae)
    for key in LATER:
        assert np.array_equal(res[key], ref[key]), "%s: stage %s differs from the dense run" % (view.id, key)
    for key in ("iters", "nseg", "segs") + (("A", "E") if ae else ()):
        assert np.array_equal(res[key], ref[key]), "%s: %s differs from the dense run" % (view.id, key)


# ------------------------------------------------------------------ 0. the dense runs against the CPU oracle
@pytest.mark.parametrize("name", ANCHORED)
def test_dense_run_matches_the_oracle(ctx, orc, name):
    res = dense_run(ctx, name)
    ref = orc.window(scene(name))
    for key in STAGES:
        assert np.array_equal(res[key], ref[key]), "%s: stage %s vs oracle" % (name, key)
    assert int(res["iters"][0]) == ref["iters"]
    for f in range(SCENES[name][2]):
        assert seg_tuples(res, f) == orc_seg_tuples(ref["segments"][f]), (name, f)


# ------------------------------------------------------------------ 1. every scene through every staging route
@pytest.mark.parametrize("view", route_views(), ids=lambda v: v.id)
def test_staging_route(ctx, view):
    res, kinds = run_view(ctx, view)
    check_view(ctx, view, res, kinds)


def test_all_four_routes_were_reported(ctx):
    seen = set()
    for label in ("scene", "margin_all_sides", "tall_frames", "small_roi_large_frame"):
        view = next(v for v in route_views() if v.scene == "bgr33x75n5" and v.label == label)
        seen.add(run_view(ctx, view)[1][0])
    assert seen == {ROUTE_DENSE, ROUTE_WHOLE, ROUTE_ROWS, ROUTE_2D}


@pytest.mark.parametrize("view", [v for v in route_views() if v.scene == "bgr33x75n21" and v.label in
                                  ("margin_all_sides", "reversed", "tall_frames", "row_stride_off_pixels_1", "frame_stride_off_rows")] +
                         [View("bgr33x75n21", ROUTE_DEVICE, "ae_misaligned", x0=1, y0=1, right=2, below=1, row_pad=1, base=3, device=True)],
                         ids=lambda v: v.id)
def test_low_rank_and_sparse_factors_do_not_depend_on_the_route(ctx, view):
    """A and E of a view are those of the dense scene bit for bit: the same kernels on the same gray plane"""
    res, kinds = run_view(ctx, view, ae=True)
    check_view(ctx, view, res, kinds, ae=True)


# ------------------------------------------------------------------ 2. alignment: first ROI byte and row stride, each residue mod 4
def test_residue_table_covers_every_kernel():
    first, stride, q15 = residue_table(alignment_views())
    for kernel in ("k_gray4", "k_gray4g", "k_gray"):
        assert first[kernel] == {0, 1, 2, 3} and stride[kernel] == {0, 1, 2, 3} and q15.get(kernel), kernel


@pytest.mark.parametrize("view", alignment_views(), ids=lambda v: v.id)
def test_alignment(ctx, view):
    res, kinds = run_view(ctx, view)
    check_view(ctx, view, res, kinds)


def test_device_views_of_the_other_scenes(ctx):
    """device frames read in place, reversed and with every kind of padding at once, for the scenes the alignment table leaves out"""
    for i, name in enumerate(k for k in SCENES if k not in ("bgr60x120n21", "bgr33x75n5", "gray60x120n21")):
        view = View(name, ROUTE_DEVICE, "padded", x0=1 + i % 3, y0=2, right=3, below=2, row_pad=1 + i % 3, frame_pad=5, base=1 + i % 3,
                    reverse=bool(i % 2), device=True)
        res, kinds = run_view(ctx, view)
        check_view(ctx, view, res, kinds)


# ------------------------------------------------------------------ 3. one groups call with every route in it
def _check_groups(ctx, views, got, kinds):
    assert kinds == [v.route for v in views], kinds
    for g, (view, res) in enumerate(zip(views, got)):
        assert np.array_equal(res["gray"], scene_gray(view.scene)), "group %d (%s): gray differs from numpy" % (g, view.id)
        check_against_lone(g, res, dense_run(ctx, view.scene), ae=False)


def test_groups_call_with_every_route(ctx):
    views = group_views()
    keep = []
    specs = [v.group_spec(keep) for v in views]
    got = ctx.batch_run_groups(specs)
    _check_groups(ctx, views, got, ctx.last_host_stage())
    assert ctx.last_host_stage() == [0, 1, 2, 3, -1, 1, 3]
    back = ctx.batch_run_groups(specs[::-1])
    _check_groups(ctx, views[::-1], back, ctx.last_host_stage())
    for a, b in zip(got, back[::-1]):
        check_against_lone(0, a, b, ae=False)
        assert np.array_equal(a["gray"], b["gray"])


def test_groups_call_factors_within_summation_order(ctx):
    """A / E of every group against the dense lone run (another summation order beside other groups: helpers.ATOL_AE)"""
    views = group_views()
    keep = []
    got = ctx.batch_run_groups([v.group_spec(keep) for v in views], want_A=True, want_E=True)
    for g, (view, res) in enumerate(zip(views, got)):
        check_against_lone(g, res, dense_run(ctx, view.scene, ae=True), ae=True)


# ------------------------------------------------------------------ 4. refusals that stay refusals
def test_refused_inputs_leave_the_context_usable(ctx):
    from swiftwatcher_amd import _lib
    name = "bgr33x75n5"
    _, nwin, n, H, W, _ = SCENES[name]
    before = dense_run(ctx, name)
    two = np.ascontiguousarray(scene(name)[..., :2])
    thin = np.ascontiguousarray(scene(name)[:, :3])
    for frames in (two, thin):
        inp, out, _res = ctx._group_io(frames, nwin, n, None, False, 255, STAGES, False, False)
        rc = _lib.load().swk_batch_run(ctx._h, ctypes.byref(inp), ctypes.byref(_lib.default_params()), ctypes.byref(out))
        assert rc == -1, "expected SWK_ERR_ARG, got %d" % rc
        with pytest.raises(_lib.SwkError):
            ctx.batch_run(frames, nwin, n)
    again = ctx.batch_run(scene(name), nwin, n)
    for key in STAGES + ("iters", "nseg", "segs"):
        assert np.array_equal(again[key], before[key]), key
    assert gray_kernel(name) == "k_gray4g"
