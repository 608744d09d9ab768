"""tests/ialm_trajectory_cases.py checked on the host, before any kernel is judged by it (tests/test_ialm_trajectory_gpu.py): the
restated loop is the oracle's at the end and at truncations, the float64 Gram route -- the CPU stand-in for the kernels -- stays
within 1e-6 of the SVD route at every k (so the GPU bound of 1e-5 leaves a correct Gram route a tenfold margin on these windows),
no stopping test of any case is decided within 1 % of tol, and the bytes of the sparse image that a perturbation below 1e-5 can
change are at most 2e-4 of a window, outside of which the stand-in's image is the oracle's."""
import numpy as np
import pytest

import ialm_trajectory_cases as tc
from oracle import reference_path as orc

NAMES = sorted(tc.CASES)


@pytest.mark.parametrize("name", NAMES)
def test_trajectory_is_the_oracles(name):
    """Same K as the case list says and as ialm_defined finds, its A and E within 1e-9 at the end and at two truncations"""
    case, tr = tc.CASES[name], tc.reference(name)
    X = tc.matrix(name)
    K = len(tr)
    assert X.shape == (case.Hc * case.Wc, case.n) and X.dtype == np.uint8
    assert K == case.K
    assert int((~X.any(axis=0)).sum()) == case.null and not X[:, :case.null].any()          # the null frames lead the queue
    if case.dup is not None:
        assert np.array_equal(X[:, case.dup], X[:, case.dup + 1]) and X[:, case.dup].any()
    A, E, k = orc.ialm_defined(X, return_iters=True)
    assert k == K
    assert np.abs(A - tr[-1].A).max() <= 1e-9 and np.abs(E - tr[-1].E).max() <= 1e-9
    for km in (3, K // 2):
        A, E, k = orc.ialm_defined(X, maxiter=km, return_iters=True)
        assert k == km
        assert np.abs(A - tr[km - 1].A).max() <= 1e-9 and np.abs(E - tr[km - 1].E).max() <= 1e-9
    assert tc.ks_to_test(name) == list(range(1, K + 2))


@pytest.mark.parametrize("name", NAMES)
def test_gram_route_standin_stays_within_1e6(name):
    tr, st = tc.reference(name), tc.standin(name)
    assert len(st) == len(tr)
    errs = [(float(np.abs(a.A - b.A).max()), float(np.abs(a.E - b.E).max())) for a, b in zip(tr, st)]
    kA, kE = int(np.argmax([e[0] for e in errs])), int(np.argmax([e[1] for e in errs]))
    print("%s: stand-in max |A - A_k| %.2e at k = %d, max |E - E_k| %.2e at k = %d" % (name, errs[kA][0], kA + 1, errs[kE][1], kE + 1))
    for k, (eA, eE) in enumerate(errs, 1):
        assert eA <= tc.ATOL_STANDIN and eE <= tc.ATOL_STANDIN, (name, k, eA, eE)
    d = tc.CASES[name].dup
    if d is not None:          # the copies of a duplicated frame: equal to rounding on both routes, to the bit on neither
        oracle = max(max(tc.copies_differ(it.A, d), tc.copies_differ(it.E, d)) for it in tr)
        gram = max(max(tc.copies_differ(it.A, d), tc.copies_differ(it.E, d)) for it in st)
        print("%s: the copies differ by %.2e on the SVD route, %.2e on the Gram route" % (name, oracle, gram))
        assert 0.0 < oracle <= 1e-9 and gram <= tc.ATOL_COPIES
    # the stopping ratios agree far inside the margin that the next test proves
    assert max(abs(a.ratio / b.ratio - 1.0) for a, b in zip(tr, st)) < 1e-6


@pytest.mark.parametrize("name", NAMES)
def test_no_stopping_test_is_near_tol(name):
    tr = tc.reference(name)
    margins = [abs(it.ratio / 1e-3 - 1.0) for it in tr]
    k = int(np.argmin(margins))
    print("%s: smallest margin %.3e at k = %d (ratio %.4e)" % (name, margins[k], k + 1, tr[k].ratio))
    assert min(margins) > tc.RATIO_MARGIN
    assert all(it.ratio >= 1e-3 for it in tr[:-1]) and tr[-1].ratio < 1e-3


@pytest.mark.parametrize("name", NAMES)
def test_boundary_mask_is_small_and_the_standin_image_is_the_oracles_outside_it(name):
    tr, st = tc.reference(name), tc.standin(name)
    worst, differing = 0.0, 0
    for k, (a, b) in enumerate(zip(tr, st), 1):
        mask = tc.boundary_mask(a.E, tc.BAND)
        worst = max(worst, float(mask.mean()))
        assert mask.mean() <= tc.MASK_CAP, (name, k, int(mask.sum()))
        want, got = orc.rpca_epilogue(a.E), orc.rpca_epilogue(b.E)
        differing += int((want != got).sum())
        assert np.array_equal(want[~mask], got[~mask]), (name, k)
        assert np.array_equal(want, tc.sparse_u8(a.E))
    print("%s: largest masked share %.2e, %d differing pixels without the mask" % (name, worst, differing))


def test_boundary_mask_marks_what_can_change():
    """Elements a perturbation below the band can carry across a byte boundary, and no others"""
    E = -np.array([0.0, 0.5, 1.0 - 4e-6, 1.0, 1.0 + 4e-6, 1.0 + 2e-5, 254.999999, 255.0 + 4e-6, 256.0, 300.0, -3.0, 4e-6, 17.3])
    want = np.array([0, 0, 1, 1, 1, 0, 1, 1, 0, 0, 0, 0, 0], bool)
    assert np.array_equal(tc.boundary_mask(E, 1e-5), want)
    rng = np.random.default_rng(5)
    E = -rng.uniform(-3.0, 260.0, 200000)
    d = rng.uniform(-1e-5, 1e-5, E.size)
    changed = tc.sparse_u8(E) != tc.sparse_u8(E + d)
    assert not (changed & ~tc.boundary_mask(E, 1e-5)).any()
