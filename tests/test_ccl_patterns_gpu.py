"""The labeller (csrc/ccl.hip) on structured frames and on both sides of its run cap.

Stage level: swk_ccl_u8 (k_ccl_frame<VEC, false>, int32 labels) over every pattern family of tests/ccl_patterns.py -- single frames
and batches that put per-pixel-path frames between run-path ones -- at all four (connectivity, order) pairs, bit for bit against the
CPU oracle; the multi-kernel path on frames too large for one workgroup; swk_regionprops_u8 on the u8-cast labels, seg_cap below the
live label count included.  tests/test_ccl_patterns_cpu.py holds the oracle to scipy and numpy on the same frames.

Batch level: k_ccl_frame<VEC, true[, GEOM]> (u8 labels + region records) reads the pipeline's opened image (handed frames of the
test's choosing it runs in tests/test_ccl_props_planes_gpu.py, through swk_debug_ccl_frame_props; the GEOM instantiation only here).
The windows of ccl_patterns.SCENES are built so that the OPENED frames have the wanted structure; every case asserts that
structure -- run counts, component counts, which branch of the kernel the frame takes -- on the CPU oracle's output before the GPU
result is looked at, then compares all six stage planes, nseg and every region record with the oracle, and the labels / records
with swk_ccl_u8 / swk_regionprops_u8 run on the call's own opened frames."""
import functools

import numpy as np
import pytest

import ccl_patterns as cp
from helpers import STAGES, check_against_lone, lone_run, orc_seg_tuples, roi_stack, seg_tuples

pytestmark = pytest.mark.gpu

PAIRS = [(8, 1), (8, 0), (4, 0), (4, 1)]
PAIR_IDS = ["8way_block", "8way_raster", "4way_raster", "4way_block"]
FAMILIES = cp.small_families()
LARGE_SHAPES = [(800, 808), (799, 811)]


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


def _records(segs):
    return [(int(s["label"]), int(s["r0"]), int(s["c0"]), int(s["r1"]), int(s["c1"]), int(s["area"]), int(s["sum_r"]), int(s["sum_c"]))
            for s in segs]


# ------------------------------------------------------------------ stage level: swk_ccl_u8
@pytest.mark.parametrize("conn,order", PAIRS, ids=PAIR_IDS)
@pytest.mark.parametrize("case", FAMILIES, ids=lambda c: c.name)
def test_ccl_single_frames(ctx, orc, case, conn, order):
    assert cp.frame_kernel_takes(*case.img.shape)
    n, lab = ctx.ccl_u8(case.img, conn, order)
    nref, ref = orc.ccl_u8(case.img, conn, order)
    want = case.comps8 if conn == 8 else case.comps4
    assert nref == want or want is None
    assert n == nref
    np.testing.assert_array_equal(lab, ref)


@pytest.mark.parametrize("conn,order", PAIRS, ids=PAIR_IDS)
@pytest.mark.parametrize("shape", cp.K_RUN_SHAPES, ids=["P0mod4", "P2mod4", "Podd"])
def test_ccl_batches_mix_run_path_and_per_pixel_frames(ctx, orc, shape, conn, order):
    """one call, same-shape frames: a 1025-run frame between two sparse ones, 1023 / 1024 / 1025 runs, checkerboards, an empty and a
    full frame -- every frame indexes its own slice of the parents and its own component count"""
    mix = cp.batch_mix(*shape)
    runs = [cp.count_runs(c.img) for c in mix]
    assert runs[0] <= cp.RUN_CAP < runs[1] and runs[2] <= cp.RUN_CAP
    ims = np.stack([c.img for c in mix])
    nc, lab = ctx.ccl_u8(ims, conn, order)
    for i, c in enumerate(mix):
        nref, ref = orc.ccl_u8(c.img, conn, order)
        assert nc[i] == nref, c.name
        np.testing.assert_array_equal(lab[i], ref, err_msg=c.name)
    # the same frames in the opposite order: no frame's labels depend on its neighbours'
    nc2, lab2 = ctx.ccl_u8(ims[::-1].copy(), conn, order)
    assert np.array_equal(nc2[::-1], nc) and np.array_equal(lab2[::-1], lab)


@pytest.mark.parametrize("conn,order", PAIRS, ids=PAIR_IDS)
@pytest.mark.parametrize("shape", LARGE_SHAPES, ids=["800x808", "799x811"])
def test_ccl_multi_kernel_path(ctx, orc, shape, conn, order):
    assert not cp.frame_kernel_takes(*shape)
    for case in cp.large_families(*shape):
        n, lab = ctx.ccl_u8(case.img, conn, order)
        nref, ref = orc.ccl_u8(case.img, conn, order)
        assert n == nref, case.name
        np.testing.assert_array_equal(lab, ref, err_msg=case.name)


@pytest.fixture()
def forced(ctx):
    """the context with the multi-kernel labeller forced for every frame size (swk_debug_force_ccl_multi_kernel), for one test"""
    ctx.force_ccl_multi_kernel(True)
    yield ctx
    ctx.force_ccl_multi_kernel(False)


@pytest.mark.parametrize("conn,order", PAIRS, ids=PAIR_IDS)
@pytest.mark.parametrize("case", FAMILIES, ids=lambda c: c.name)
def test_ccl_single_frames_multi_kernel_forced(forced, orc, case, conn, order):
    """the pattern families through k_ccl_init / union / flatten / wordprefix / label, which otherwise only meets frames too large
    for one workgroup"""
    n, lab = forced.ccl_u8(case.img, conn, order)
    nref, ref = orc.ccl_u8(case.img, conn, order)
    want = case.comps8 if conn == 8 else case.comps4
    assert nref == want or want is None
    assert n == nref
    np.testing.assert_array_equal(lab, ref)


# ------------------------------------------------------------------ stage level: swk_regionprops_u8
def _check_regionprops(ctx, orc, lab8, name):
    want = orc_seg_tuples(orc.regionprops_u8(lab8))
    segs, n = ctx.regionprops_u8(lab8)
    assert n == len(want), name
    assert _records(segs) == want, name
    if len(want) > 1:          # seg_cap below the live label count: nseg reports all, the records are the first seg_cap by ascending label
        for cap in sorted({1, len(want) // 2, len(want) - 1}):
            segs, n = ctx.regionprops_u8(lab8, seg_cap=cap)
            assert n == len(want) and len(segs) == cap, (name, cap)
            assert _records(segs) == want[:cap], (name, cap)
    return len(want)


@pytest.mark.parametrize("case", FAMILIES, ids=lambda c: c.name)
def test_regionprops_on_the_oracle_labels(ctx, orc, case):
    for conn, order in [(8, 1), (4, 0)]:
        n, lab = orc.ccl_u8(case.img, conn, order)
        live = _check_regionprops(ctx, orc, orc.labels_to_u8(lab), (case.name, conn))
        assert live == min(n, 255)


def test_regionprops_with_more_than_255_and_511_components(ctx, orc):
    """the frames whose labels wrap once and more than once, as one batch, and the large frames"""
    by = {c.name: c for c in FAMILIES}
    labs, counts = [], []
    for name, conn in [("checkerboard2_64x96", 4), ("k1025_isolated_64x96", 8), ("checkerboard1_64x96", 4), ("k1023_trunk_64x96", 8)]:
        n, lab = orc.ccl_u8(by[name].img, conn, 0)
        labs.append(orc.labels_to_u8(lab))
        counts.append(n)
    assert counts[0] > 511 and counts[1] > 4 * 256 and counts[2] > 255 and counts[3] == 1
    for cap in (255, 100):
        segs, nseg = ctx.regionprops_u8(np.stack(labs), seg_cap=cap)
        for i, lab8 in enumerate(labs):
            want = orc_seg_tuples(orc.regionprops_u8(lab8))
            assert nseg[i] == len(want) == min(counts[i], 255)
            assert _records(segs[i, :min(nseg[i], cap)]) == want[:cap]
    for shape in LARGE_SHAPES:
        for case in cp.large_families(*shape):
            n, lab = orc.ccl_u8(case.img, 4, 0)
            _check_regionprops(ctx, orc, orc.labels_to_u8(lab), case.name)


# ------------------------------------------------------------------ batch level: the fused kernel with records
@functools.lru_cache(maxsize=None)
def _roi(name):
    return cp.block_scene(**cp.SCENES[name])


@functools.lru_cache(maxsize=None)
def _oracle(name, conn=8, order=1):
    from oracle import reference_path as orc
    return orc.window(_roi(name), connectivity=conn, label_order=order)


def _regimes(name, conn=8, order=1):
    """[(frame, runs, components)] of the oracle's non-empty opened frames"""
    from oracle import reference_path as orc
    out = [(f,) + cp.frame_regime(orc, img, conn, order) for f, img in enumerate(_oracle(name, conn, order)["opened"]) if img.any()]
    assert out, "%s: every opened frame is empty" % name
    return out


def _params(conn, order):
    from swiftwatcher_amd import _lib
    return _lib.default_params(connectivity=conn, label_order=order)


def _check_call(ctx, orc, res, ref, cap=255, conn=8, order=1, what=""):
    """one window of a batch call against the oracle's window, and against the stage functions on the call's own opened frames"""
    n = ref["opened"].shape[0]
    for key in STAGES:
        assert np.array_equal(res[key], ref[key]), "%s: stage %s differs from the oracle" % (what, key)
    assert int(res["iters"][0]) == int(ref["iters"]), what
    nc, lab32 = ctx.ccl_u8(res["opened"], conn, order)
    assert np.array_equal(res["labels"], orc.labels_to_u8(lab32)), "%s: labels differ from swk_ccl_u8 on the opened frames" % what
    segs, nseg = ctx.regionprops_u8(res["labels"], seg_cap=cap)
    assert np.array_equal(res["nseg"], nseg), what
    for f in range(n):
        want = orc_seg_tuples(ref["segments"][f])
        assert int(nc[f]) == orc.ccl_u8(ref["opened"][f], conn, order)[0], (what, f)
        assert int(res["nseg"][f]) == len(want) == min(int(nc[f]), 255), (what, f)
        got = seg_tuples(res, f)
        assert len(got) == min(len(want), cap), (what, f)
        assert got == want[:cap], "%s frame %d: records differ from the oracle" % (what, f)
        assert got == _records(segs[f, :min(nseg[f], cap)]), "%s frame %d: records differ from swk_regionprops_u8" % (what, f)
        # label k and label 256 + k united: box of the union, area and coordinate sums added; label 256 gone
        assert got == cp.merged_records(lab32[f])[:cap], "%s frame %d: records differ from the recount of the int32 labels" % (what, f)


@pytest.mark.parametrize("cap", [255, 17])
def test_batch_fallback_with_records(ctx, orc, cap):
    """Case a: the per-pixel branch (nruns > cap) of k_ccl_frame<4, true>.  Oracle: 1785-1890 runs and 595-630 components on every
    patterned frame, so the labels wrap more than twice and every frame has 255 records."""
    regimes = _regimes("dense_212x424")
    assert all(r > cp.RUN_CAP and c > 511 for _, r, c in regimes) and len(regimes) >= 3
    assert (212 * 424) % 4 == 0
    res = ctx.batch_run(_roi("dense_212x424"), 1, 21, seg_cap=cap)
    _check_call(ctx, orc, res, _oracle("dense_212x424"), cap, what="dense_212x424 cap %d" % cap)


def test_batch_run_path_with_wrap(ctx, orc):
    """Case b: the by_runs branch with labels above 255.  Oracle: 858-897 runs (at most the cap) and 286-299 components on every
    patterned frame: records 1 .. n - 256 are unions of two regions, the others single regions, label 256 has none."""
    regimes = _regimes("wrap_212x424")
    assert all(r <= cp.RUN_CAP and 257 <= c <= 341 for _, r, c in regimes) and len(regimes) >= 3
    ref = _oracle("wrap_212x424")
    for f, _, c in regimes:          # the oracle's own records are the united ones
        assert orc_seg_tuples(ref["segments"][f]) == cp.merged_records(orc.ccl_u8(ref["opened"][f])[1])
    res = ctx.batch_run(_roi("wrap_212x424"), 1, 21)
    _check_call(ctx, orc, res, ref, what="wrap_212x424")
    for f, _, c in regimes:
        lab32 = ctx.ccl_u8(res["opened"][f])[1]
        for k in (1, c - 256):
            rr, cc = np.nonzero((lab32 == k) | (lab32 == k + 256))
            assert (lab32 == k + 256).any()
            assert seg_tuples(res, f)[k - 1] == (k, rr.min(), cc.min(), rr.max() + 1, cc.max() + 1, rr.size, rr.sum(), cc.sum())


def test_batch_either_side_of_the_run_cap(ctx, orc):
    """Case c: one window whose patterned frames have, on the oracle, 1023, 1024, 1025, 900, 1026 and 1200 runs (341, 341, 341, 300,
    342, 400 components; frames 0, 4, 8, 12, 16, 20): the last frames the run path takes, the first the per-pixel path takes,
    side by side in one launch."""
    regimes = _regimes("cap_212x424")
    assert [r for _, r, _ in regimes] == [1023, 1024, 1025, 900, 1026, 1200]
    assert [c for _, _, c in regimes] == [341, 341, 341, 300, 342, 400]
    assert any(900 <= r <= cp.RUN_CAP for _, r, _ in regimes) and any(cp.RUN_CAP < r <= 1200 for _, r, _ in regimes)
    res = ctx.batch_run(_roi("cap_212x424"), 1, 21)
    _check_call(ctx, orc, res, _oracle("cap_212x424"), what="cap_212x424")


def test_batch_either_side_of_the_run_cap_multi_kernel_forced(forced, orc):
    """case c's window with launch_ccl + launch_regionprops in the batch call: 341 / 342 / 400 components a frame, so the u8 labels
    wrap and k_props unites label k with label 256 + k"""
    res = forced.batch_run(_roi("cap_212x424"), 1, 21)
    forced.force_ccl_multi_kernel(False)          # (_check_call's own swk_ccl_u8 takes the one-workgroup kernel: two routes, one result)
    _check_call(forced, orc, res, _oracle("cap_212x424"), what="cap_212x424 forced")


@pytest.mark.parametrize("name,residue,fallback", [("dense_212x424", 0, True), ("dense_211x422", 2, True), ("dense_211x423", 1, True),
                                                   ("sparse_64x96", 0, False), ("sparse_63x94", 2, False), ("sparse_67x95", 1, False)])
def test_batch_all_three_load_widths(ctx, orc, name, residue, fallback):
    """Case d: P = 0 mod 4, 2 mod 4 and odd select k_ccl_frame<4>, <2> and <1>.  The 211 x 422 and 211 x 423 ROIs hold more than 1024
    runs on every patterned frame (the per-pixel branch at every width).  63 x 94 and 67 x 95 cannot: 342 blocks of 3 x 3 would
    cover half of such an ROI, and the RPCA returns an empty frame for so dense a foreground; there the run path is asserted
    (about a hundred blocks, 297-342 runs)."""
    s = cp.SCENES[name]
    assert (s["H"] * s["W"]) % 4 == residue
    regimes = _regimes(name)
    if fallback:
        assert all(r > cp.RUN_CAP and c > 511 for _, r, c in regimes) and len(regimes) >= 3
    else:
        assert all(100 < r <= cp.RUN_CAP and c >= 30 for _, r, c in regimes) and len(regimes) >= 3
    res = ctx.batch_run(_roi(name), 1, 21)
    _check_call(ctx, orc, res, _oracle(name), what=name)


@pytest.mark.parametrize("conn,order", [(4, 1), (4, 0), (8, 0)], ids=["4way", "4way_raster", "8way_raster"])
def test_batch_fallback_parameter_variants(ctx, orc, conn, order):
    """Case e: connectivity = 4 and label_order = SWK_ORDER_RASTER on case a's window (the per-pixel branch, 255 records)."""
    regimes = _regimes("dense_212x424", conn, order)
    assert all(r > cp.RUN_CAP and c > 511 for _, r, c in regimes) and len(regimes) >= 3
    res = ctx.batch_run(_roi("dense_212x424"), 1, 21, params=_params(conn, order))
    _check_call(ctx, orc, res, _oracle("dense_212x424", conn, order), conn=conn, order=order, what="dense_212x424 %d/%d" % (conn, order))


@pytest.mark.parametrize("dense,sparse,tiny", [("dense_212x424", "sparse_64x96", (4, 9)), ("dense_211x422", "sparse_63x94", (4, 9)),
                                               ("dense_211x423", "sparse_67x95", (5, 7))], ids=["P0mod4", "P2mod4", "Podd"])
def test_batch_groups_with_a_fallback_frame(ctx, orc, dense, sparse, tiny):
    """Case f: one swk_batch_run_groups call = one k_ccl_frame<VEC, true, true> launch over a group whose patterned frames take the
    per-pixel branch, a run-path group of another geometry (its records cut at seg_cap 40, below its component count) and a tiny
    group.  VEC is the widest load that every group's pixel count allows (swk_api.hip, run_batch): the three parametrisations hold
    pixel counts that are all multiples of 4, all even with one 2 mod 4, and odd ones.  Every group equals its lone run and the
    oracle."""
    assert all(r > cp.RUN_CAP and c > 511 for _, r, c in _regimes(dense))
    assert all(r <= cp.RUN_CAP and c > 40 for _, r, c in _regimes(sparse))
    n = 21
    tiny_roi = roi_stack(3320, 1, tiny[0], tiny[1])
    rois = [_roi(dense), _roi(sparse), tiny_roi]
    specs = [dict(frames=rois[0], nwin=1, n=n), dict(frames=rois[1], nwin=1, n=n, seg_cap=40), dict(frames=rois[2], nwin=1, n=n)]
    got = ctx.batch_run_groups(specs)
    assert len(got) == 3
    refs = [_oracle(dense), _oracle(sparse), orc.window(tiny_roi)]
    for g, (spec, res, ref) in enumerate(zip(specs, got, refs)):
        check_against_lone(g, res, lone_run(ctx, spec), ae=False)
        _check_call(ctx, orc, res, ref, cap=spec.get("seg_cap", 255), what="group %d" % g)
