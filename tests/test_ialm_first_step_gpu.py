"""The first step of the IALM on the GPU (swk_debug_ialm_first_step: the chain's start, then ialm_first_step -- the slab sum, the
small-matrix step of k = 0 in k_ialm_small or k_ialm_small_wide, and k_ialm_refine_start) against the 256-bit reference of
tests/ialm_first_step_cases.py, window by window, in grey levels of A_1:

  err(B_std) <= 8 C_GRAM eps cond^2 / mu_0          the matrix the small-matrix step leaves, under both solvers
  err(B_fin) <= 8 C_REF eps cond / mu_0             where the window was refined (refine == 2)

and the states: which windows are flagged (the estimate and its threshold), refined, given up (null frame, repeated frame: B_fin is
B_std bit for bit and holds the project's definition) or over the work cap; windows in a batch equal their lone results.

Every window enters as 8-bit pixels: from the integer start (lmbda = 4), from the f64 start pass of a window that clips nothing
(lmbda = 4, integer start off: the refinement forms its double-double Gram matrix from the pixels) and from the f64 start pass of a
window whose first shrinkage clips (lmbda = 0.01)."""
import time

import numpy as np
import pytest

import ialm_first_step_cases as fc

pytestmark = pytest.mark.gpu

METHODS = [0, 1]
METHOD_IDS = ["newton_schulz", "jacobi"]
ALWAYS = 1e-30          # swk_set_start_refine: every window with a finite estimate is flagged


@pytest.fixture(scope="module")
def ctx():
    from swiftwatcher_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def _call(ctx, x, lmbda, integer, method, tau):
    ctx.set_ialm_variant(0)
    ctx.set_integer_start(1 if integer else 0)
    ctx.set_eig_method(method)
    ctx.set_start_refine(tau)
    return ctx.debug_ialm_first_step(x, lmbda)


def _run(ctx, case, method, tau):
    """One lone window through the first step; the start is the one the reference assumed (start choice, mu_0 and the dual norm
    to the bit: M_1 is a function of them)."""
    ref = fc.reference(case)
    res = _call(ctx, ref.x[None], case.lmbda, case.integer, method, tau)
    assert int(res["int_gram"][0]) == int(case.integer), case.name
    assert float(res["mu_0"][0]) == ref.mu and float(res["dual_norm"][0]) == ref.dual, case.name
    return ref, res


def _hold(what, e, bound):
    print("%s: err %.3e, bound %.3e (%.3f of it)" % (what, e, bound, e / bound))
    assert e <= bound, "%s: err %.3e over the bound %.3e" % (what, e, bound)


def _check_refined_and_not(ctx, case, method):
    """tau = 1e-30: the window is refined and both matrices hold their bounds; refinement off: B_fin is B_std, bit for bit the
    matrix of the refined run's small-matrix step."""
    ref, res = _run(ctx, case, method, ALWAYS)
    cs, cr = fc.EPS * ref.cond ** 2 * ref.inv_mu, fc.EPS * ref.cond * ref.inv_mu
    assert int(res["refine"][0]) == 2, "%s: refine = %d" % (case.name, res["refine"][0])
    e_std, e_fin = fc.err(res["B_std"][0], ref), fc.err(res["B_fin"][0], ref)
    print("%s: cond %.1f, 1/mu_0 %.1f, solver steps %d, C of B_std %.4f, C of B_fin %.4f (read transposed: %.4f)"
          % (case.name, ref.cond, ref.inv_mu, res["sweeps"][0], e_std / cs, e_fin / cr, fc.err(res["B_fin"][0].T, ref) / cr))
    _hold(case.name + " B_std", e_std, fc.bound_std(ref))
    _hold(case.name + " B_fin", e_fin, fc.bound_ref(ref))
    assert (res["sweeps"][0] >= 100) == (method == 1)
    _, off = _run(ctx, case, method, 0.0)
    assert int(off["refine"][0]) == 0
    assert np.array_equal(off["B_fin"], off["B_std"]) and np.array_equal(off["B_std"], res["B_std"])
    return res


@pytest.mark.parametrize("n", fc.FRAMES)
@pytest.mark.parametrize("start", fc.STARTS)
@pytest.mark.parametrize("method", METHODS, ids=METHOD_IDS)
def test_every_frame_count(ctx, method, start, n):
    """sigma = 0.6 at every frame count around the block counts 1..4 (thread layouts 256 / 512 / 1024, the double buffer up to 48
    frames, plain = (n == 1)), from each start."""
    case = fc.FRAME_CASES[(n, start)]
    if start == "clip":
        assert fc.reference(case).clipped          # the host's M_1, before the GPU is read
    _check_refined_and_not(ctx, case, method)


@pytest.mark.parametrize("n", sorted(fc.SQUARE_CASES))
@pytest.mark.parametrize("method", METHODS, ids=METHOD_IDS)
def test_from_pixels_with_one_pixel_more_than_frames(ctx, method, n):
    """P = n + 1: the double-double Gram matrix from the pixels is one or two partial chunks"""
    _check_refined_and_not(ctx, fc.SQUARE_CASES[n], method)


@pytest.mark.parametrize("key", sorted(fc.TABLE_CASES), ids=str)
def test_scenes_of_the_table(ctx, key):
    _check_refined_and_not(ctx, fc.TABLE_CASES[key], 0)


@pytest.mark.parametrize("key", sorted(fc.SIGMA_CASES), ids=str)
@pytest.mark.parametrize("method", METHODS, ids=METHOD_IDS)
def test_other_noise_levels_and_the_default_threshold(ctx, method, key):
    """sigma = 8, 2 and 0.3: B_std holds its bound; with the default tau = 1e-5 the flag is the host's statement of it."""
    case = fc.SIGMA_CASES[key]
    ref, res = _run(ctx, case, method, 1e-5)
    _hold(case.name + " B_std", fc.err(res["B_std"][0], ref), fc.bound_std(ref))
    _, est, cond_k = fc.cond_estimate(ref)
    assert cond_k <= 1e7 and abs(est / 1e-5 - 1.0) > 0.01, "%s: the estimate %.3e is too close to the threshold to be a case" % (case.name, est)
    print("%s: estimate %.3e, refine %d" % (case.name, est, res["refine"][0]))
    if est > 1e-5:
        assert int(res["refine"][0]) == 2
        _hold(case.name + " B_fin", fc.err(res["B_fin"][0], ref), fc.bound_ref(ref))
    else:
        assert int(res["refine"][0]) == 0 and np.array_equal(res["B_fin"], res["B_std"])


@pytest.mark.parametrize("case", fc.FLAG_CASES, ids=fc.case_id)
@pytest.mark.parametrize("method", METHODS, ids=METHOD_IDS)
def test_flag_fires_at_its_estimate(ctx, method, case):
    """tau 1 % below the exact estimate 1.1e-16 ||G_1||_F sum 1 / lambda_i / mu_0 flags the window, 1 % above does not; the
    returned cond_sum is the exact one within 1e-5 (float64 eigvalsh: below 1e-7 for cond(K) <= 1e7, asserted)."""
    ref = fc.reference(case)
    cond_sum, est, cond_k = fc.cond_estimate(ref)
    assert cond_k <= 1e7
    _, lo = _run(ctx, case, method, 0.99 * est)
    _, hi = _run(ctx, case, method, 1.01 * est)
    print("%s: cond_sum %.6e (exact %.6e), estimate %.3e" % (case.name, lo["cond_sum"][0], cond_sum, est))
    assert int(lo["refine"][0]) >= 1 and int(hi["refine"][0]) == 0
    for r in (lo, hi):
        assert abs(float(r["cond_sum"][0]) / cond_sum - 1.0) <= 1e-5


@pytest.mark.parametrize("key", sorted(fc.GIVEUP_CASES), ids=lambda k: "%s_%s" % k)
@pytest.mark.parametrize("method", METHODS, ids=METHOD_IDS)
def test_rank_deficient_windows_are_given_up(ctx, method, key):
    """A null frame and a repeated last frame: flagged, given up (refine == 3), B_fin is B_std bit for bit, and B_std holds the
    project's definition -- directions below 1e-13 lambda_max carry weight 0 -- within the standard bound at the conditioning of the
    live part: against the 256-bit reference of the remaining frames (null frame), against the float64 statement (repeated frame)."""
    case = fc.GIVEUP_CASES[key]
    ref, res = _run(ctx, case, method, ALWAYS)
    assert int(res["refine"][0]) == 3, "%s: refine = %d" % (case.name, res["refine"][0])
    assert np.array_equal(res["B_fin"], res["B_std"])
    B = res["B_std"][0]
    if case.kind == "null":
        dead = int(np.flatnonzero(~ref.live)[0])
        assert B[dead, dead] == 1.0 and not np.delete(B[dead], dead).any() and not np.delete(B[:, dead], dead).any()
        _hold(case.name + " B_std", fc.err(B, ref), fc.bound_std(ref))
        assert (res["sweeps"][0] >= 100) == (method == 1)          # a dead direction is masked: Newton-Schulz still solves it
    else:
        _hold(case.name + " B_std", fc.err_vs(B, fc.to_fixed(fc.definition_f64(ref)), ref.M), fc.bound_std(ref))
        assert res["sweeps"][0] >= 100          # ||Z||_F^2 >= 1e11 (or no convergence) hands a singular matrix to Jacobi


def test_work_cap_of_the_gram_matrix_from_the_pixels(ctx):
    """64 frames from the f64 start are 2080 pairs, 3 rounds per pixel: 133,333 pixels stay under 400,000 pixel x pair rounds and are
    refined within the bound, 133,334 go over (refine == 4, B_fin is B_std)."""
    x = fc.window(fc.CAP_OVER)
    over = _call(ctx, x[None], fc.CAP_OVER.lmbda, False, 0, ALWAYS)
    assert int(over["int_gram"][0]) == 0 and int(over["refine"][0]) == 4
    assert np.array_equal(over["B_fin"], over["B_std"])
    t = time.perf_counter()
    ref, under = _run(ctx, fc.CAP_UNDER, 0, ALWAYS)
    print("under the cap: %.2f s for the call" % (time.perf_counter() - t))
    assert int(under["refine"][0]) == 2
    _hold("cap B_std", fc.err(under["B_std"][0], ref), fc.bound_std(ref))
    _hold("cap B_fin", fc.err(under["B_fin"][0], ref), fc.bound_ref(ref))


def _between(refs, flagged):
    """A threshold between the estimates of the windows that are to be flagged and those that are not, a factor 2 from either"""
    est = [fc.cond_estimate(r)[1] for r in refs]
    lo = max(e for e, f in zip(est, flagged) if not f)
    hi = min(e for e, f in zip(est, flagged) if f)
    assert hi > 4 * lo, est
    return float(np.sqrt(lo * hi))


@pytest.mark.parametrize("start", sorted(fc.BATCH_CASES))
@pytest.mark.parametrize("method", METHODS, ids=METHOD_IDS)
def test_windows_of_a_batch_equal_their_lone_results(ctx, method, start):
    """Refined, unflagged, null frame, repeated frame, refined in one call: states as expected, and every window's results are those
    of the window run alone -- bit for bit from the integer start (K is exact whatever the slab count); from the pixels B_fin of the
    refined windows bit for bit (their K comes from the pixels), the rest through the states and the bound, since the f64 start pass
    sums a lone window's slabs in another order."""
    batch = fc.BATCH_CASES[start]
    refs = [fc.reference(c) for c in batch]
    want = [2, 0, 3, 3, 2]
    tau = _between(refs, [w != 0 for w in want])
    x = np.stack([r.x for r in refs])
    both = _call(ctx, x, batch[0].lmbda, batch[0].integer, method, tau)
    assert [int(v) for v in both["refine"]] == want
    for w, (case, ref) in enumerate(zip(batch, refs)):
        _, alone = _run(ctx, case, method, tau)
        assert int(alone["refine"][0]) == want[w], case.name
        assert int(both["int_gram"][w]) == int(case.integer)
        for key in ("dual_norm", "mu_0", "thr_0", "dnorm"):
            assert both[key][w] == alone[key][0], (case.name, key)
        if case.integer:
            for key in ("B_std", "B_fin", "cond_sum", "sweeps"):
                assert np.array_equal(both[key][w], alone[key][0]), (case.name, key)
        elif want[w] == 2:
            assert np.array_equal(both["B_fin"][w], alone["B_fin"][0]), case.name
        if want[w] != 2:
            assert np.array_equal(both["B_fin"][w], both["B_std"][w]), case.name
        if case.kind == "plain":
            _hold(case.name + " B_std in the batch", fc.err(both["B_std"][w], ref), fc.bound_std(ref))
            if want[w] == 2:
                _hold(case.name + " B_fin in the batch", fc.err(both["B_fin"][w], ref), fc.bound_ref(ref))


@pytest.mark.parametrize("n", fc.WIDE_FRAMES)
def test_long_windows(ctx, n):
    """65, 100 and 128 frames go through k_ialm_small_wide (Jacobi in global memory) and hold the standard bound; the plan switches
    the refinement off above 64 frames."""
    case = fc.WIDE_CASES[n]
    ref, res = _run(ctx, case, 0, ALWAYS)
    assert int(res["refine"][0]) == 0 and np.array_equal(res["B_fin"], res["B_std"]) and res["sweeps"][0] >= 100
    _hold(case.name + " B_std", fc.err(res["B_std"][0], ref), fc.bound_std(ref))
