"""tests/ialm_first_step_cases.py checked on the host, so that tests/test_ialm_first_step_gpu.py cannot silently test nothing: the
256-bit reference proves itself on every case, the two float64 stand-ins (LAPACK's eigh of K for the Gram route, its SVD of the window
for the refined route) have the constants the case module writes down, a refinement that returned the standard B would miss the
refined tolerance tenfold on every ill-conditioned case, and the checker fails what it must fail: a transposed unsymmetrised W and a
B from a K with one pixel dropped."""
import numpy as np
import pytest

import ialm_first_step_cases as fc
from ialm_first_step_cases import EPS


@pytest.mark.parametrize("case", fc.PROOF_CASES, ids=fc.case_id)
def test_reference_proves_itself(case):
    """max |I - W K W| and max |W - W^T| below 2^-150 in the reference's own arithmetic (asserted where W is formed), on the frames
    that are not null; the window is what the case says it is: its start, its clipping, the exactness of M_1 and K."""
    ref = fc.reference(case)
    assert ref.proof < 2.0 ** -150 and ref.steps >= 1
    print("%s: %d steps, proof %.1e, cond %.1f, 1/mu_0 %.1f" % (case.name, ref.steps, ref.proof, ref.cond, ref.inv_mu))
    assert ref.x.shape == (case.n, case.P) and (case.P >= 2 * case.n or case.name.startswith("square"))
    if case.lmbda == fc.LMBDA:
        assert ref.clipped, "the first shrinkage of this window must clip at lmbda = 0.01"
    else:
        assert not ref.clipped
    assert int(ref.live.sum()) == case.n - (case.kind == "null")
    # K is the Gram matrix of the float64 M_1 (of X): symmetric, and its float64 image agrees with a float64 product
    kf = fc.k_float(ref)
    a = ref.x.astype(np.float64) if ref.integer else ref.M
    np.testing.assert_allclose(kf, a @ a.T, rtol=1e-12)
    assert all(ref.K[i, j] == ref.K[j, i] for i in range(case.n) for j in range(i))


def _constants(case):
    ref = fc.reference(case)
    cg = fc.err(fc.standin_eigh(ref), ref) / (EPS * ref.cond ** 2 * ref.inv_mu)
    cr = fc.err(fc.standin_svd(ref), ref) / (EPS * ref.cond * ref.inv_mu)
    return cg, cr


def test_standins_have_the_constants_written_down():
    """C_GRAM and C_REF are the maxima of err / (eps cond^2 / mu_0) and err / (eps cond / mu_0) of the two stand-ins over the whole
    case list, rounded up to two digits: no case exceeds them, and the largest is within a tenth of them (they were not padded)."""
    cs = [_constants(case) for case in fc.CASES]
    for case, (cg, cr) in zip(fc.CASES, cs):
        print("%-36s C_gram %.4f  C_ref %.4f" % (case.name, cg, cr))
    cg, cr = max(c[0] for c in cs), max(c[1] for c in cs)
    print("maxima: C_gram %.4f  C_ref %.4f" % (cg, cr))
    assert 0.9 * fc.C_GRAM <= cg <= fc.C_GRAM
    assert 0.9 * fc.C_REF <= cr <= fc.C_REF


@pytest.mark.parametrize("case", fc.ILL_CONDITIONED, ids=fc.case_id)
def test_standard_route_would_fail_the_refined_bound(case):
    """On an ill-conditioned window the Gram route in float64 misses the refined route's tolerance by 10x or more, while the SVD
    stand-in meets it: a refinement that handed the standard B back would not pass."""
    ref = fc.reference(case)
    assert ref.cond > 1000
    e_gram, e_svd = fc.err(fc.standin_eigh(ref), ref), fc.err(fc.standin_svd(ref), ref)
    print("%s: eigh %.2e, svd %.2e, refined bound %.2e" % (case.name, e_gram, e_svd, fc.bound_ref(ref)))
    assert e_gram >= 10 * fc.bound_ref(ref)
    assert e_gram <= fc.bound_std(ref) and e_svd <= fc.bound_ref(ref)


CAN_FAIL = [fc.FRAME_CASES[(17, "int")], fc.FRAME_CASES[(33, "f64")], fc.FRAME_CASES[(48, "clip")]]


@pytest.mark.parametrize("case", CAN_FAIL, ids=fc.case_id)
def test_checker_fails_a_transposed_unsymmetrised_w(case):
    """W = R^-1 polar(R) formed the way k_ialm_refine_start forms it (float64 restatement: forward substitution, scaled coupled
    Newton-Schulz, the product not symmetrised) meets the refined bound; the same W read transposed misses it, although W - W^T is
    rounding noise next to W: the forward error of U, eps cond, then meets R instead of the orthonormal Q."""
    ref = fc.reference(case)
    b, bt = fc.standin_refine_route(ref)
    e, et = fc.err(b, ref), fc.err(bt, ref)
    print("%s: as used %.2e, transposed %.2e, bound %.2e, max |W - W^T| mu_0 = %.2e" % (case.name, e, et, fc.bound_ref(ref), np.abs(b - bt).max()))
    assert e <= fc.bound_ref(ref)
    assert et > fc.bound_ref(ref)


@pytest.mark.parametrize("case", CAN_FAIL[:2], ids=fc.case_id)
def test_checker_fails_a_dropped_pixel(case):
    """B from the 256-bit K^(-1/2) of a K that lacks the window's last pixel fails both bounds (the kernel's last partial chunk)"""
    ref = fc.reference(case)
    a = ref.x.astype(np.float64) if ref.integer else ref.M
    shift = 0 if ref.integer else fc.M_SHIFT
    last = fc._exact_int(a[:, -1], shift)
    k_less = ref.K - np.outer(last, last)
    w, _, _ = fc.invsqrt_fixed(k_less, ref.kshift)
    b_less = fc._b_exact(w, ref.c1, ref.inv_mu)
    b64 = np.array([[int(v) / fc.ONE for v in row] for row in b_less], np.float64)
    e = fc.err(b64, ref)
    e_right = fc.err(np.array([[int(v) / fc.ONE for v in row] for row in ref.B], np.float64), ref)
    print("%s: one pixel dropped %.2e, the exact B rounded %.2e, bounds %.2e / %.2e" % (case.name, e, e_right, fc.bound_ref(ref), fc.bound_std(ref)))
    assert e_right <= fc.bound_ref(ref)
    assert e > fc.bound_std(ref) and e > fc.bound_ref(ref)


def test_rank_deficient_definition_and_estimate():
    """The float64 statement of the project's definition gives the null frame weight 0 and agrees with the 256-bit reference of the
    remaining frames within the standard bound; the flag's estimate from eigvalsh is usable (cond(K) <= 1e7) on the windows the flag
    test uses."""
    for st in ("int", "clip"):
        ref = fc.reference(fc.GIVEUP_CASES[("null", st)])
        b = fc.definition_f64(ref)
        dead = int(np.flatnonzero(~ref.live)[0])          # (LAPACK leaves the null direction mixed in at 1e-15; the kernels mask it exactly)
        assert abs(b[dead, dead] - 1.0) < 1e-12 and np.abs(np.delete(b[dead], dead)).max() < 1e-12
        assert fc.err(b, ref) <= fc.bound_std(ref)
    for case in fc.FLAG_CASES:
        _, est, cond_k = fc.cond_estimate(fc.reference(case))
        assert cond_k <= 1e7 and est > 0
