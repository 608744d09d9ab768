"""The IALM on the GPU at EVERY iteration count against the oracle's iterates (tests/ialm_trajectory_cases.py; the reference and the
windows are proven on the host by tests/test_ialm_trajectory_cpu.py).  maxiter = k stops a run after exactly k iterations, so each
truncation is a full, legal run through entry points the library already has:

  swk_ialm(..., maxiter=k)            A_k and E_k of the float64 passes (A/Y-state MFMA pass, LDS pass, the plain f64 kernels of long
                                      windows) under both small-matrix solvers, within 1e-5 of the oracle's iterate k -- the bound the
                                      suite holds the final result to -- plus the iteration count, exact zeros in null frames, the two
                                      copies of a duplicated frame within 1e-6 of each other, the stopping norm, the solver's step count
  swk_batch_run, params.maxiter = k   the M-state pass's uint8 sparse image of iteration k: the oracle's wherever a perturbation of
                                      E_k below 1e-5 cannot change the byte, and the same bytes under every variant and speculation
  eight windows in one batch          stopping by tol and by the cap in the same iteration

What runs only from iteration 2 on -- the passes' mode switch, the warm-started Newton-Schulz tables, the dead directions once Y is no
longer the scaled X, the store-and-norm bookkeeping, k_ialm_small_wide after its first call -- is held here iterate by iterate, not
by the final result alone.  The last test needs no GPU: it feeds the same assertions deliberately wrong trajectories."""
import functools
import time

import numpy as np
import pytest

import ialm_trajectory_cases as tc

gpu = pytest.mark.gpu

ROUTES = [(2, 0), (2, 1), (1, 0), (1, 1), (6, 1)]
ROUTE_IDS = ["mfma_pass+newton_schulz", "mfma_pass+jacobi", "lds_pass+newton_schulz", "lds_pass+jacobi", "plain_f64+wide_jacobi"]
UP_TO_64 = ("plain21", "null21", "short5", "full64", "dup", "n37")
LONG_ROUTE = ("plain21", "full64", "wide70", "wide65")
AE_PARAMS = [pytest.param(r, name, id="%s-%s" % (rid, name)) for r, rid in zip(ROUTES, ROUTE_IDS)
             for name in (LONG_ROUTE if r[0] == 6 else UP_TO_64)]


@pytest.fixture(scope="module")
def contexts():
    """One context per (pass variant, solver), made when first asked for"""
    from swiftwatcher_amd import _lib
    made = {}

    def get(variant, method):
        if (variant, method) not in made:
            c = made[(variant, method)] = _lib.Context(0)
            c.set_ialm_variant(variant)
            c.set_eig_method(method)
        return made[(variant, method)]
    yield get
    for c in made.values():
        c.close()


# ------------------------------------------------------------------ a. A_k, E_k and the norm at every truncation
@gpu
@pytest.mark.parametrize("route,name", AE_PARAMS)
def test_every_truncation_of_the_f64_passes(contexts, route, name):
    variant, method = route
    ctx = contexts(variant, method)
    x = tc.planes(name)
    K = tc.steps(name)
    newton_schulz = variant != 6 and method == 0
    t0 = time.perf_counter()
    worst_a = worst_e = 0.0
    steps, at_K = [], None
    for k in tc.ks_to_test(name):
        A, E, iters = ctx.ialm(x, maxiter=k)
        ratio, err_bound = ctx.last_stopping_norms()
        assert len(ratio) == 1
        eA, eE = tc.check_iterate(name, k, A, E, iters, float(ratio[0]), float(err_bound[0]))
        worst_a, worst_e = max(worst_a, eA), max(worst_e, eE)
        sweeps = ctx.last_eig_sweeps
        steps.append(sweeps)
        if newton_schulz and name in tc.FULL_RANK:
            assert sweeps < 100, "%s k=%d: the warm-started Newton-Schulz solve handed over to Jacobi (%d)" % (name, k, sweeps)
        if not newton_schulz:
            assert sweeps >= 100
        if k == K:
            at_K = (A, E)
        if k == K + 1:          # the cap above the stopping iteration changes nothing
            assert np.array_equal(A, at_K[0]) and np.array_equal(E, at_K[1]), "%s: maxiter K + 1 is not maxiter K bit for bit" % name
    print("TRAJ a %s %s: K %d, max |A - A_k| %.2e, max |E - E_k| %.2e, solver steps %d..%d, %.2f s"
          % (ROUTE_IDS[ROUTES.index(route)], name, K, worst_a, worst_e, min(steps), max(steps), time.perf_counter() - t0))


# ------------------------------------------------------------------ b. the M-state image at every truncation
MSTATE_VARIANTS = (0, 4, 5)
SPECULATIONS = (None, (0.0, 0.0), (16.0, 0.0))          # (sparse, norm) factors; None: the library's defaults


@functools.lru_cache(maxsize=None)
def _expected_images(name):
    """Per k = 1..K: (the oracle's uint8 image of E_k as (n, Hc, Wc), the elements a perturbation below 1e-5 can change)"""
    from oracle import reference_path as orc
    case = tc.CASES[name]
    out = []
    for it in tc.reference(name):
        img = orc.rpca_epilogue(it.E).T.reshape(case.n, case.Hc, case.Wc)
        mask = tc.boundary_mask(it.E, tc.BAND).T.reshape(case.n, case.Hc, case.Wc)
        assert mask.mean() <= tc.MASK_CAP
        out.append((img, mask))
    return out


def _mstate_context(variant, spec):
    from swiftwatcher_amd import _lib
    c = _lib.Context(0)
    c.set_ialm_variant(variant)
    if spec is not None:
        c.set_sparse_speculation(spec[0])
        c.set_norm_speculation(spec[1])
    return c


@gpu
@pytest.mark.parametrize("name", UP_TO_64)
def test_mstate_image_at_every_truncation(name):
    """A truncated run often stops right after a pass whose sparse-image stores were switched off: the guess failed and the window
    runs again.  The library then keeps its guesses off for the next 64 batches, so a context whose guess failed is replaced by a
    fresh one: every k meets the speculation it is listed with."""
    from swiftwatcher_amd import _lib
    case = tc.CASES[name]
    frames = tc.frames(name)
    K = tc.steps(name)
    want = _expected_images(name)
    ks = tc.ks_to_test(name)
    first = {}
    redone = masked = fresh = 0
    t0 = time.perf_counter()
    for variant in MSTATE_VARIANTS:
        for spec in SPECULATIONS:
            ctx = _mstate_context(variant, spec)
            for k in ks:
                p = _lib.default_params()
                p.maxiter = k
                before = ctx.redo_windows
                res = ctx.batch_run(frames, 1, case.n, params=p, stages=("rpca",))
                again = ctx.redo_windows - before
                assert 0 <= again <= 1, "%d windows ran again in a call of one" % again
                assert spec != (0.0, 0.0) or again == 0
                redone += again
                assert int(res["iters"][0]) == min(k, K), (name, variant, spec, k, int(res["iters"][0]))
                img, mask = want[min(k, K) - 1]
                bad = (res["rpca"] != img) & ~mask
                assert not bad.any(), "%s variant %d speculation %s k=%d: %d bytes differ outside the mask" % (name, variant, spec, k, int(bad.sum()))
                masked += int((res["rpca"] != img).sum())
                if case.dup is not None:          # the two copies of the duplicated frame: the same bytes
                    d = case.dup
                    assert np.array_equal(res["rpca"][d][~(mask[d] | mask[d + 1])], res["rpca"][d + 1][~(mask[d] | mask[d + 1])])
                    assert not res["rpca"][:case.null].any()
                if k in first:
                    assert np.array_equal(res["rpca"], first[k]), "%s variant %d speculation %s k=%d: not the bytes of the first route" % (name, variant, spec, k)
                else:
                    first[k] = res["rpca"]
                if again:
                    ctx.close()
                    ctx = _mstate_context(variant, spec)
                    fresh += 1
            ctx.close()
    assert np.array_equal(first[K + 1], first[K])
    print("TRAJ b %s: K %d, %d calls, %d reruns (%d fresh contexts), %d bytes inside the mask differ from the oracle's, %.2f s"
          % (name, K, len(ks) * 9, redone, fresh, masked, time.perf_counter() - t0))


# ------------------------------------------------------------------ c. mixed stopping in one batch
@gpu
def test_windows_that_stop_by_tol_and_by_the_cap_in_one_batch():
    """Eight windows of two kinds that stop after 23 and 22 iterations alternately, in one call with maxiter = 21 (every window capped),
    22 (half stop by tol in the iteration that caps the others) and 23 (none capped): per window the iteration count and the image
    of the oracle run with that cap, and the same bytes from a second call."""
    from oracle import reference_path as orc
    from swiftwatcher_amd import _lib, synthetic
    n, Hc, Wc, nwin = 21, 64, 96, 8
    kinds = (dict(birds=3, noise=2.0, bird_len=(8, 14), bird_wid=(3, 6)), dict(birds=12, noise=6.0, bird_len=(20, 30), bird_wid=(10, 14)))
    roi = np.concatenate([synthetic.roi_window(4100 + 7 * w, n, Hc, Wc, **kinds[w % 2]) for w in range(nwin)])
    gray = np.stack([orc.bgr2gray(f) for f in roi])
    trs = [tc.trajectory(gray[w * n:(w + 1) * n].reshape(n, -1).T) for w in range(nwin)]
    assert [len(tr) for tr in trs] == [23, 22] * 4
    for w in (0, 1):          # the restated loop is the oracle's on both kinds of window, at the cap that splits them
        ref = orc.window(np.ascontiguousarray(roi[w * n:(w + 1) * n]), maxiter=22)
        assert ref["iters"] == 22
        np.testing.assert_array_equal(ref["rpca"], orc.rpca_epilogue(trs[w][21].E).T.reshape(n, Hc, Wc))
    ctx = _lib.Context(0)
    t0 = time.perf_counter()
    for cap in (21, 22, 23):
        p = _lib.default_params()
        p.maxiter = cap
        res = ctx.batch_run(gray, nwin, n, params=p, stages=("rpca",))
        again = ctx.batch_run(gray, nwin, n, params=p, stages=("rpca",))
        assert res["rpca"].tobytes() == again["rpca"].tobytes() and res["iters"].tobytes() == again["iters"].tobytes()
        for w in range(nwin):
            k = min(cap, len(trs[w]))
            assert int(res["iters"][w]) == k, (cap, w, int(res["iters"][w]))
            np.testing.assert_array_equal(res["rpca"][w * n:(w + 1) * n], orc.rpca_epilogue(trs[w][k - 1].E).T.reshape(n, Hc, Wc),
                                          err_msg="maxiter %d window %d" % (cap, w))
    print("TRAJ c: %.2f s on the GPU side" % (time.perf_counter() - t0))
    ctx.close()


# ------------------------------------------------------------------ d. the assertions reject a wrong trajectory (no GPU)
def _first_rejected(name, tr):
    """The first k at which the assertions of (a) fail the trajectory tr, or None"""
    for k, it in enumerate(tr, 1):
        try:
            tc.check_iterate(name, k, it.A, it.E, min(k, len(tr)), it.ratio)
        except AssertionError:
            return k
    return None


def test_per_iterate_bound_rejects_wrong_trajectories():
    """The assertions of (a), fed on the host.  The float64 Gram-route stand-in passes them at every k, the stopping norm's derived
    bound included.  Two wrong stand-ins do not: one that applies mu <- 1.5 mu one iteration late at k = 3 only (rejected at k = 4, the
    first iterate that runs on the wrong mu), and one that keeps the dead-direction weight -1/mu from iteration 2 on (rejected at k = 2
    on the window with a duplicated frame; on a window of full rank there is no dead direction and it IS the stand-in).

    The final-iterate check alone -- same K, A and E within 1e-5 -- rejects both as well on these windows: measured on the host, the late
    mu leaves the last iterate 26 to 47 grey levels off (plain21 47, short5 41, full64 26) and the kept weight 23 (dup).  A wrong step is
    not forgiven here: an error in one early iterate grows until the loop stops.  What the per-iterate bound adds is the k and the
    route at which a kernel first goes wrong, and the code that no final result ever reaches when the loop runs to its end."""
    for name in ("plain21", "dup"):
        assert _first_rejected(name, tc.standin(name)) is None
    late = tc.mutant_trajectory(tc.matrix("plain21"), "mu_late")
    assert np.array_equal(late[2].A, tc.standin("plain21")[2].A)          # iterates 1..3 are untouched
    assert _first_rejected("plain21", late) == 4
    kept = tc.mutant_trajectory(tc.matrix("dup"), "dead_weight")
    assert _first_rejected("dup", kept) == 2
    assert not tc.check_final_only("plain21", late) and not tc.check_final_only("dup", kept)
    same = tc.mutant_trajectory(tc.matrix("plain21"), "dead_weight")
    assert all(np.array_equal(a.A, b.A) for a, b in zip(same, tc.standin("plain21")))
