"""Conditions on the INPUTS of tests/test_ingest_routes_gpu.py and tests/test_output_placement_gpu.py (helpers.py: scenes, views,
tables), checked without a GPU: a scene without regions, a view that does not hold its scene, constant padding or a table that misses
a residue would let those tests pass without testing anything.  A case that fails here is mended, not dropped from its table."""
import functools

import numpy as np
import pytest

import helpers
from helpers import (ALIGN_SCENES, ANCHOR_ELEMS, ANCHORED, ROUTE_2D, ROUTE_DENSE, ROUTE_ROWS, ROUTE_WHOLE, SCENES, alignment_views,
                     gray_kernel, group_views, residue_table, route_views, scene)

ALL_VIEWS = route_views() + alignment_views() + group_views()


@functools.lru_cache(maxsize=None)
def _oracle(name):
    """orc.window per window of a scene, once"""
    from oracle import reference_path as orc
    _, nwin, n, _, _, ch = SCENES[name]
    s = scene(name)
    if ch == 1:          # the single-channel scene is the gray of its BGR twin: the same later stages
        return _oracle([k for k, v in SCENES.items() if v[:5] == SCENES[name][:5] and v[5] == 3][0])
    return [orc.window(np.ascontiguousarray(s[w * n:(w + 1) * n])) for w in range(nwin)]


@pytest.mark.parametrize("name", list(SCENES))
def test_every_scene_leaves_regions(name):
    for ref in _oracle(name):
        per_frame = [len(s) for s in ref["segments"]]
        assert sum(per_frame) >= 1, "scene %s: the oracle finds no region in any frame" % name
        assert max(per_frame) <= 255


def test_anchored_scenes():
    """the two scenes whose dense runs are held to the oracle: large enough for the oracle to be LAPACK-independent, at most 255
    components per frame (the u8 labels would wrap), regions in several frames, and at least 3 regions somewhere (the record-cap test)"""
    assert ANCHORED == ("bgr60x120n21", "bgr67x101n21")
    for name in ANCHORED:
        _, _, n, H, W, _ = SCENES[name]
        assert n * H * W >= ANCHOR_ELEMS
        ref = _oracle(name)[0]
        assert all(int(lab.max()) == len(s) <= 255 for lab, s in zip(ref["labels"], ref["segments"]))
        assert sum(1 for s in ref["segments"] if s) >= 3
    assert max(len(s) for s in _oracle("bgr67x101n21")[0]["segments"]) >= 3
    assert max(len(s) for ref in _oracle("bgr36x52n21w2") for s in ref["segments"]) >= 2          # (the other record-cap scene)


def test_plane_sizes_of_the_output_scenes():
    """67x101x21 is not a whole number of dwords (the gray plane takes the library's padded buffer), 60x120x21 is"""
    sizes = {k: v[1] * v[2] * v[3] * v[4] for k, v in SCENES.items()}
    assert sizes["bgr67x101n21"] % 4 == 3 and sizes["bgr60x120n21"] % 4 == 0 and sizes["bgr33x75n5"] % 2 == 1


def test_scene_widths_reach_every_gray_kernel():
    assert sorted({SCENES[k][4] % 4 for k in SCENES if SCENES[k][5] == 3}) == [0, 1, 2, 3]
    assert [gray_kernel(k) for k in ALIGN_SCENES] == ["k_gray4", "k_gray4g", "k_gray"]


@pytest.mark.parametrize("view", ALL_VIEWS, ids=lambda v: v.id)
def test_view_embeds_its_scene_in_noise(view):
    buf = view.buffer()
    arr = view.host_array(buf)
    roi = arr[:, view.y0:view.y0 + view.Hc, view.x0:view.x0 + view.Wc]
    assert np.array_equal(roi[::-1] if view.reverse else roi, scene(view.scene))
    mask = view.roi_mask()
    assert int(mask.sum()) == view.roi_bytes
    outside = buf[~mask]
    if view.route == ROUTE_DENSE or view.label.startswith("dense"):          # the scene itself: nothing around it but the buffer's ends
        assert outside.size == view.base + 8 and len(np.unique(outside)) > 1
    else:
        assert outside.size >= view.F * view.Hc and len(np.unique(outside)) > 64, "bytes outside the ROI are (nearly) constant"
    # margins, row padding and frame padding, where the view has them, each hold noise of their own
    if view.x0:
        assert len(np.unique(arr[:, :, :view.x0])) > 16
    if view.y0:
        assert len(np.unique(arr[:, :view.y0])) > 16
    # the crop lies inside a frame and the frames do not overlap
    assert view.x0 + view.Wc <= view.Wf and view.y0 + view.Hc <= view.Hf and view.rs >= view.Wf * view.ch and view.fs >= view.Hf * view.rs
    assert view.base + (view.F - 1) * view.fs + view.Hf * view.rs <= view.nbytes


def test_every_host_view_is_named_after_the_route_the_rule_gives():
    for v in ALL_VIEWS:
        if not v.device:
            assert v.rule_route() == v.route, v.id


def test_route_table_covers_every_route_for_every_scene():
    for name in SCENES:
        labels = {(v.route, v.label) for v in route_views() if v.scene == name}
        assert {r for r, _ in labels} == {ROUTE_DENSE, ROUTE_WHOLE, ROUTE_ROWS, ROUTE_2D}
        assert sum(1 for r, _ in labels if r == ROUTE_WHOLE) >= 6 and sum(1 for r, _ in labels if r == ROUTE_ROWS) >= 2
        if SCENES[name][5] == 3:
            assert {v.rs % 3 for v in route_views() if v.scene == name} == {0, 1, 2}
    assert any(v.fs % v.rs for v in route_views())
    for route in (ROUTE_WHOLE, ROUTE_ROWS, ROUTE_2D):
        assert any(v.reverse for v in route_views() if v.route == route)


def test_the_factor_two_views_sit_on_the_rule_and_just_beyond():
    for name in SCENES:
        by = {v.label: v for v in route_views() if v.scene == name}
        for on, beyond, route in (("factor2_exact", "factor2_one_more_row", ROUTE_2D),
                                  ("factor2_exact_full_rows", "factor2_one_more_full_row", ROUTE_ROWS)):
            a, b = by[on], by[beyond]
            assert a.F * a.fs == 2 * a.roi_bytes and a.route == ROUTE_WHOLE
            assert b.F * b.fs == 2 * b.roi_bytes + b.F * b.rs and b.route == route          # one more row per frame
            assert (a.x0, a.y0, a.rs) == (b.x0, b.y0, b.rs) and b.Hf == a.Hf + 1
            # ... and nothing but the factor-2 clause refuses the view beyond
            assert b.rs % b.ch == 0 and b.fs % b.rs == 0 and b.rs >= (b.x0 + b.Wc) * b.ch and b.fs >= (b.y0 + b.Hc) * b.rs


def test_residue_table_covers_every_kernel():
    first, stride, q15 = residue_table(alignment_views())
    for kernel in ("k_gray4", "k_gray4g", "k_gray"):
        assert first[kernel] == {0, 1, 2, 3}, kernel
        assert stride[kernel] == {0, 1, 2, 3}, kernel
        assert q15.get(kernel), "no misaligned Q15 view for %s" % kernel
    # both families separately: host views on the whole-buffer route, device views read in place
    for dev in (False, True):
        f, s, _ = residue_table([v for v in alignment_views() if v.device == dev])
        assert all(f[k] == {0, 1, 2, 3} and s[k] == {0, 1, 2, 3} for k in f) and len(f) == 3
    # a row stride that is not a multiple of 4 makes the rows of one launch alternate between the aligned and the byte-wise branch
    assert any(v.row_residues() == {0, 1, 2, 3} for v in alignment_views())
    assert all(not v.device and v.route == ROUTE_WHOLE or v.device for v in alignment_views())


def test_group_views_differ_in_geometry():
    views = group_views()
    assert [v.route for v in views] == [0, 1, 2, 3, -1, 1, 3]
    assert len({v.n for v in views}) == 1
    assert len({(v.Hc, v.Wc, v.x0, v.y0) for v in views}) == len(views)
    assert views[4].device and views[4].first_roi_residue() != 0 and views[5].reverse and views[6].ch == 1


def test_guarded_buffer_notices_a_stray_byte():
    g = helpers.Guarded(10, device=False, shift=3)
    assert g.ptr % 4 == 3 and g.read().tolist() == [helpers.Guarded.SENTINEL] * 10
    for at in (g.lead - 1, g.lead + 10):
        g2 = helpers.Guarded(10, device=False, shift=3)
        g2.buf[at] = 0
        with pytest.raises(AssertionError):
            g2.read()
