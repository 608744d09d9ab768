"""The yardsticks of tests/test_ccl_patterns_gpu.py, checked on the CPU before they are trusted on frames they have never been
compared on: over every pattern family of tests/ccl_patterns.py the C oracle's labeller equals scipy.ndimage.label (4- and 8-way, its
2x2-block order the same partition ranked by first block), the counts the patterns have by construction hold, and the oracle's
region records of the u8-cast labels equal a plain numpy recount.  Then the demonstrations that the checks can fail: a wrong rule in
a numpy restatement is caught by the family / the scene that aims at it."""
import functools

import numpy as np
import pytest

import ccl_patterns as cp
from helpers import orc_seg_tuples


@pytest.fixture(scope="module")
def orc():
    from oracle import reference_path
    return reference_path


FAMILIES = cp.small_families()
LARGE = cp.large_families(160, 203)          # the tiling itself, at a size that keeps scipy quick (the GPU file tiles to 800 x 808)


@functools.lru_cache(maxsize=None)
def _oracle_window(name):
    from oracle import reference_path as orc
    return orc.window(cp.block_scene(**cp.SCENES[name]))


def test_names_are_unique_and_values_vary():
    names = [c.name for c in FAMILIES + LARGE]
    assert len(set(names)) == len(names)
    for c in FAMILIES:
        vals = np.unique(c.img[c.img != 0])
        assert c.img.dtype == np.uint8 and (vals.size > 1 or np.count_nonzero(c.img) <= 2), c.name


@pytest.mark.parametrize("case", FAMILIES + LARGE, ids=lambda c: c.name)
def test_oracle_equals_scipy_and_counts_hold(orc, case):
    counts = cp.assert_oracle_matches_scipy(orc, case.img)
    runs = cp.count_runs(case.img)
    # the run count by two routes: the flattened-bitmap rule and a per-row difference
    fg = np.pad(case.img != 0, ((0, 0), (1, 0)))
    assert runs == int(np.count_nonzero(fg[:, 1:] & ~fg[:, :-1]))
    if case.runs is not None:
        assert runs == case.runs
    if case.comps4 is not None:
        assert counts[4] == case.comps4
    if case.comps8 is not None:
        assert counts[8] == case.comps8


@pytest.mark.parametrize("case", FAMILIES, ids=lambda c: c.name)
def test_oracle_regionprops_equal_a_numpy_recount(orc, case):
    for conn, order in [(8, 1), (4, 0)]:
        lab = orc.ccl_u8(case.img, conn, order)[1]
        lab8 = orc.labels_to_u8(lab)
        got = orc_seg_tuples(orc.regionprops_u8(lab8))
        assert got == cp.numpy_regionprops(lab8)
        assert got == cp.merged_records(lab)          # label k and label k + 256 j united, multiples of 256 gone


def test_families_reach_what_they_aim_at():
    """the regimes the GPU file relies on, from the patterns alone"""
    by = {c.name: c for c in FAMILIES}
    # row-wrap pairs inside one bitmap word and across two
    straddles = [s for W in cp.ROW_WRAP_WIDTHS for s in cp.row_wrap_straddles(W)]
    assert any(straddles) and not all(straddles)
    # exactly k runs at the three pixel-count residues
    assert sorted((H * W) % 4 for H, W in cp.K_RUN_SHAPES) == [0, 1, 2]
    for H, W in cp.K_RUN_SHAPES:
        for k in cp.K_RUNS:
            for kind in ("isolated", "trunk"):
                assert cp.count_runs(by["k%d_%s_%dx%d" % (k, kind, H, W)].img) == k
    # both sides of the run cap among the chains and the checkerboards
    assert cp.count_runs(by["checkerboard1_212x424"].img) > cp.RUN_CAP and cp.count_runs(by["serpentine_212x424"].img) <= cp.RUN_CAP
    # more than 255 and more than 511 components (the u8 wrap of the records)
    assert by["k1025_isolated_64x96"].comps8 > 4 * 256 and by["checkerboard2_64x96"].comps4 > 511
    # the extreme shapes fit the one-workgroup kernel, on both sides of the cap, with runs that start beyond column 32767 / row 16383
    for H, W in cp.EXTREME_SHAPES:
        assert cp.frame_kernel_takes(H, W), (H, W, cp.frame_lds_bytes(H, W))
        assert cp.count_runs(by["extreme_%dx%d_runs" % (H, W)].img) <= cp.RUN_CAP < cp.count_runs(by["extreme_%dx%d_dense" % (H, W)].img)
        rr, cc = np.nonzero(cp.run_starts_flat(by["extreme_%dx%d_runs" % (H, W)].img))
        assert rr.max() == H - 1 and (cc.max() > 32767 or rr.max() > 16383)
    # the frames of the multi-kernel tests are beyond it; the workload ROIs are not
    assert not cp.frame_kernel_takes(800, 808) and not cp.frame_kernel_takes(799, 811)
    assert cp.frame_kernel_takes(212, 424) and cp.frame_kernel_takes(425, 850)


def test_u_shape_roots_differ_between_the_numbering_rules(orc):
    """the U is label 2 in raster order (the lone pixel comes first) and label 1 in 2x2-block order"""
    img = cp.u_shape().img
    raster, block = orc.ccl_u8(img, 8, 0)[1], orc.ccl_u8(img, 8, 1)[1]
    assert raster[0, 4] == 1 and raster[1, 0] == 2 and block[0, 4] == 2 and block[1, 0] == 1


def test_batch_mix_has_both_paths_side_by_side():
    for H, W in cp.K_RUN_SHAPES:
        runs = [cp.count_runs(c.img) for c in cp.batch_mix(H, W)]
        assert runs[1] == 1025 and runs[0] <= cp.RUN_CAP and runs[2] <= cp.RUN_CAP
        assert {1023, 1024, 1025} <= set(runs) and 0 in runs


# ------------------------------------------------------------------ the pipeline scenes: regimes on the oracle's output
def test_scene_regimes(orc):
    """what tests/test_ccl_patterns_gpu.py claims per scene, asserted once here as well so that a GPU-less machine sees it"""
    def regimes(name):
        return [cp.frame_regime(orc, f) for f in _oracle_window(name)["opened"] if f.any()]
    dense = regimes("dense_212x424")
    assert dense and all(r > cp.RUN_CAP and c > 511 for r, c in dense)
    wrap = regimes("wrap_212x424")
    assert wrap and all(r <= cp.RUN_CAP and 257 <= c <= 341 for r, c in wrap)
    assert [r for r, _ in regimes("cap_212x424")] == [1023, 1024, 1025, 900, 1026, 1200]


# ------------------------------------------------------------------ each check can fail
def test_dropping_the_column0_term_is_caught_by_the_row_wrap_family():
    """Run starts without the `col0` term (a set bit starts a run only when the bit before it in the FLATTENED bitmap is clear) merge
    (r, W - 1) with (r + 1, 0): the row-wrap family's run count by construction rejects that rule at every width, and accepts
    the right one."""
    for W in cp.ROW_WRAP_WIDTHS:
        case = cp.row_wrap(W)
        assert cp.count_runs(case.img, col0=True) == case.runs
        assert cp.count_runs(case.img, col0=False) == case.runs // 2 != case.runs
    # the families without a run that starts in column 0 right after a set last column cannot tell the rules apart
    blind = cp.staircase(9, 9, False)
    assert cp.count_runs(blind.img, col0=False) == blind.runs


def test_counting_label_256_as_label_1_is_caught_by_the_run_path_wrap_scene(orc):
    """Region records with label 256 counted as label 1 (instead of vanishing with the u8 cast) differ from the oracle's records
    on every patterned frame of the wrap scene (286-299 components on at most 1024 runs); the right rule -- label k united with
    label 256 + k, label 256 gone -- equals them.  On a frame with at most 255 components the two rules agree, so only a scene
    that wraps can tell."""
    ref = _oracle_window("wrap_212x424")
    seen = 0
    for f, opened in enumerate(ref["opened"]):
        if not opened.any():
            continue
        n, lab = orc.ccl_u8(opened)
        assert 257 <= n <= 341 and cp.count_runs(opened) <= cp.RUN_CAP
        want = orc_seg_tuples(ref["segments"][f])
        assert len(want) == 255
        assert cp.merged_records(lab) == want
        wrong = cp.numpy_regionprops(np.where(lab == 256, 1, lab % 256))
        assert wrong != want and [w for w in wrong if w[0] != 1] == [w for w in want if w[0] != 1]
        # records of the united labels: the box is the union's, the sums add up
        for k in (1, n - 256):
            a, b = lab == k, lab == k + 256
            rec = want[k - 1]
            assert rec[0] == k and rec[5] == int(a.sum() + b.sum())
            rr, cc = np.nonzero(a | b)
            assert rec[1:5] == (rr.min(), cc.min(), rr.max() + 1, cc.max() + 1) and rec[6:] == (rr.sum(), cc.sum())
        seen += 1
    assert seen >= 3
    sparse = _oracle_window("sparse_64x96")
    for f, opened in enumerate(sparse["opened"]):
        n, lab = orc.ccl_u8(opened)
        assert n <= 255
        assert cp.numpy_regionprops(np.where(lab == 256, 1, lab % 256)) == orc_seg_tuples(sparse["segments"][f])
