"""No result depends on what the context ran before it.

One protocol for every case (tests/history_cases.py): `fresh` is the victim call on a new Context, `after` the same call on a
Context that first ran a sequence of valid, larger calls -- the dirtiers -- that leave the most in the device buffers the victim
uses.  after == fresh byte for byte in every output (stage images, iteration counts, region and shape records, A and E as raw
float64 bytes, shift tables, review planes, network inputs, skip counts), and fresh meets the assertion its host reference already
has in the suite: ialm_trajectory_cases.check_iterate at the final K, the masked image comparison of test_ialm_trajectory_gpu.py,
equality with the CPU oracle or the numpy restatement for the integer kernels.  No tolerance is new.

Stale contents are what real calls leave: no poison fill, no debug hook, no write into a slot from outside.
tests/test_history_independence_cpu.py shows from the geometry alone that the dirtiers' footprints cover the victims' padding, and
that history_cases.SLOTS names a case in here for every slot of the library."""
import functools
import gc
import os
import subprocess
import sys

import numpy as np
import pytest

import frame_chunks as fc
import history_cases as hc
import ialm_trajectory_cases as tc
from helpers import STAGES, orc_seg_tuples, roi_stack, seg_tuples

pytestmark = pytest.mark.gpu

ROOT = hc.ROOT
RESULT_KEYS = STAGES + ("iters", "nseg", "segs")


@pytest.fixture(scope="module")
def orc():
    from oracle import reference_path
    return reference_path


# ------------------------------------------------------------------ the protocol
def _on_new_context(setup, calls):
    """runs the calls on one new Context (setup first); the last call's result"""
    from swiftwatcher_amd import _lib
    c = _lib.Context(0)
    try:
        if setup is not None:
            setup(c)
        out = None
        for call in calls:
            out = call(c)
        return out
    finally:
        c.close()


def pair(victim, dirtiers, what, setup=None):
    """fresh and after of one victim; returns fresh for the comparison with the host reference"""
    fresh = _on_new_context(setup, [victim])
    after = _on_new_context(setup, list(dirtiers) + [victim])
    hc.assert_same(fresh, after, what)
    return fresh


def _pick(res, keys=RESULT_KEYS + ("A", "E")):
    return {k: res[k] for k in keys if k in res}


# ------------------------------------------------------------------ dirtiers
def d_batch(d, ae, **kw):
    def run(c):
        c.batch_run(hc.dirtier_frames(d), d.nwin, d.n, want_A=ae, want_E=ae, **kw)
    return run


def d_ialm(d):
    """swk_ialm takes one window: the dirtier's first"""
    def run(c):
        c.ialm(hc.dirtier_frames(d)[:d.n].reshape(d.n, -1))
    return run


def d_dense_scene(c):
    """255 region records on every patterned frame, labels that wrap, every stage plane of 21 x 212 x 424 written"""
    c.batch_run(hc.scene_roi("dense_212x424"), 1, 21)


def ialm_sequence(dirt, last_with_factors):
    """d64 alone, or d64 and then d70 (another route: the plain f64 kernels and k_ialm_small_wide); each with A and E wanted and
    not wanted, the kind the victim runs last"""
    order = (False, True) if last_with_factors else (True, False)
    seq = [d_batch(hc.D64, ae) for ae in order]
    if last_with_factors:
        seq.append(d_ialm(hc.D64))
    if dirt == "d64_then_d70":
        seq += [d_batch(hc.D70, ae) for ae in order]
        if last_with_factors:
            seq.append(d_ialm(hc.D70))
    return seq


DIRT = ["d64", "d64_then_d70"]


def d_unrelated(c):
    """another family's leftovers for the stand-alone calls: a batch with factors, a conversion of large frames, the forced labeller"""
    d_batch(hc.D64, True)(c)
    c.bgr_to_yuv420(_bright_bgr(30, 70, 130))
    c.force_ccl_multi_kernel(True)
    c.ccl_u8(_busy_masks(24, 70, 130))
    c.force_ccl_multi_kernel(False)
    c.grey_open_u8(_bright_planes(40, 70, 130), (5, 5))


@functools.lru_cache(maxsize=None)
def _bright_planes(count, H, W):
    """planes of blobs near 255 on a bright noisy ground: every stage of the filter leaves large values everywhere"""
    rng = np.random.default_rng(count * 100003 + H * 1009 + W)
    r, c = np.indices((H, W))
    out = rng.integers(120, 256, size=(count, H, W)).astype(np.uint8)
    for k in range(count):
        out[k][((r // 5 + c // 7 + k) % 3) == 0] = 255
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _bright_bgr(count, H, W):
    out = np.random.default_rng(count + H + W).integers(100, 256, size=(count, H, W, 3), dtype=np.uint8)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _busy_masks(count, H, W):
    """isolated pixels on a lattice of period 2, shifted per frame: (H / 2) (W / 2) > 255 components under either connectivity"""
    out = np.zeros((count, H, W), np.uint8)
    for k in range(count):
        out[k, (k % 2)::2, ((k // 2) % 2)::2] = 255
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _busy_labels(count, H, W):
    """u8 label planes that hold every label 1..255, scattered over the whole plane"""
    rng = np.random.default_rng(H * W + count)
    out = rng.integers(1, 256, size=(count, H, W)).astype(np.uint8)
    out.setflags(write=False)
    return out


# ------------------------------------------------------------------ family 1: the IALM on every route
@functools.lru_cache(maxsize=None)
def _expected_image(name):
    """the oracle's u8 image of E_K and the elements a perturbation of E below 1e-5 can change (test_ialm_trajectory_gpu.py)"""
    case = tc.CASES[name]
    it = tc.reference(name)[-1]
    from oracle import reference_path as orc
    img = orc.rpca_epilogue(it.E).T.reshape(case.n, case.Hc, case.Wc)
    mask = tc.boundary_mask(it.E, tc.BAND).T.reshape(case.n, case.Hc, case.Wc)
    assert mask.mean() <= tc.MASK_CAP
    return img, mask


def _check_mstate_image(name, res, what):
    case, K = tc.CASES[name], tc.steps(name)
    assert int(res["iters"][0]) == K, (what, int(res["iters"][0]), K)
    img, mask = _expected_image(name)
    bad = (res["rpca"] != img) & ~mask
    assert not bad.any(), "%s: %d bytes differ from the oracle's outside the mask" % (what, int(bad.sum()))
    assert not res["rpca"][:case.null].any(), "%s: a null frame's sparse image is not 0" % what
    if case.dup is not None:
        d = case.dup
        free = ~(mask[d] | mask[d + 1])
        assert np.array_equal(res["rpca"][d][free], res["rpca"][d + 1][free]), what


def _mstate_victim(name):
    frames = tc.frames(name)

    def run(c):
        return _pick(c.batch_run(frames, 1, frames.shape[0], stages=("rpca",)))
    return run


@pytest.mark.parametrize("dirt", DIRT)
@pytest.mark.parametrize("name", hc.TRAJECTORY_VICTIMS)
def test_mstate_window_after_ialm_dirtiers(name, dirt):
    """The default route of swk_batch_run (pass variants 0 = 4 and 5): M lies in the A
    slot, binary16 U in the Y slot, neither is cleared, and planes n .. fpad - 1 of both hold what the dirtiers left."""
    for variant in (0, 4, 5):
        what = "%s variant %d after %s" % (name, variant, dirt)
        fresh = pair(_mstate_victim(name), ialm_sequence(dirt, False), what, setup=lambda c, v=variant: c.set_ialm_variant(v))
        _check_mstate_image(name, fresh, what)


def _check_scene(orc, name, res, what, cap=255, **overrides):
    """one window against the CPU oracle: the six stages, the iteration count, every region record (test_ccl_patterns_gpu.py)"""
    ref = hc.scene_oracle(name, **overrides)
    for key in STAGES:
        assert np.array_equal(res[key], ref[key]), "%s: stage %s differs from the oracle" % (what, key)
    assert int(res["iters"][0]) == int(ref["iters"]), what
    for f in range(ref["opened"].shape[0]):
        want = orc_seg_tuples(ref["segments"][f])
        assert int(res["nseg"][f]) == len(want), (what, f)
        assert seg_tuples(res, f)[:cap] == want[:cap], "%s frame %d: records differ from the oracle" % (what, f)


def _scene_victim(name, params=None, **kw):
    def run(c):
        return _pick(c.batch_run(hc.scene_roi(name), 1, 21, params=params, **kw))
    return run


@pytest.mark.parametrize("mode", ["stages", "factors"])
@pytest.mark.parametrize("name", hc.SCENE_VICTIMS)
def test_batch_scene_after_ialm_dirtiers(orc, name, mode):
    """ROIs of 63 x 94 (2 mod 16) and 67 x 95 (odd) pixels: every plane of A / Y / E has padded columns, the labeller reads bytes, and
    every stage after the IALM runs on buffers the dense scene and d64 filled.  With A and E asked for: the host staging of
    (pixels, frames) too."""
    ae = mode == "factors"
    seq = [d_dense_scene] + ialm_sequence("d64_then_d70", ae)
    what = "%s %s" % (name, mode)
    fresh = pair(_scene_victim(name, want_A=ae, want_E=ae), seq, what)
    _check_scene(orc, name, fresh, what)
    if ae:
        last = hc.scene_trajectory(name)[-1]
        eA, eE = float(np.abs(fresh["A"][0] - last.A).max()), float(np.abs(fresh["E"][0] - last.E).max())
        print("HISTORY %s: max |A - A_K| %.2e, max |E - E_K| %.2e" % (what, eA, eE))
        assert eA <= tc.ATOL_AE and eE <= tc.ATOL_AE, (what, eA, eE)


ROUTES = [(2, 0), (2, 1), (1, 0), (1, 1), (6, 1)]
ROUTE_IDS = ["mfma_pass+newton_schulz", "mfma_pass+jacobi", "lds_pass+newton_schulz", "lds_pass+jacobi", "plain_f64+wide_jacobi"]


def _route_setup(variant, method, more=None):
    def setup(c):
        c.set_ialm_variant(variant)
        c.set_eig_method(method)
        if more is not None:
            more(c)
    return setup


def _factor_victim(name):
    x, K = tc.planes(name), tc.steps(name)

    def run(c):
        A, E, iters = c.ialm(x, maxiter=K)
        ratio, err_bound = c.last_stopping_norms()
        return dict(A=A, E=E, iters=np.array([iters], np.int32), ratio=np.asarray(ratio, np.float64), err_bound=np.asarray(err_bound, np.float64))
    return run


def _check_factors(name, res):
    """check_iterate at the final K: the iteration count, A_K and E_K within 1e-5, exact zeros in null frames (the dirtiers have
    none), the copies of a duplicated frame, the stopping norm within its derived bound"""
    return tc.check_iterate(name, tc.steps(name), res["A"], res["E"], int(res["iters"][0]), float(res["ratio"][0]), float(res["err_bound"][0]))


@pytest.mark.parametrize("dirt", DIRT)
@pytest.mark.parametrize("route", ROUTES, ids=ROUTE_IDS)
def test_ialm_factors_after_ialm_dirtiers(route, dirt):
    """swk_ialm with A and E under the A/Y-state MFMA pass and the LDS pass, each under Newton-Schulz and Jacobi, and under variant 6
    (the plain f64 kernels, wide70 and plain21).  The A/Y-state route clears A always and Y where fpad != n; E when it is asked for."""
    variant, method = route
    for name in (hc.WIDE_VICTIMS if variant == 6 else hc.TRAJECTORY_VICTIMS):
        what = "%s %s after %s" % (ROUTE_IDS[ROUTES.index(route)], name, dirt)
        fresh = pair(_factor_victim(name), ialm_sequence(dirt, True), what, setup=_route_setup(variant, method))
        _check_factors(name, fresh)


@pytest.mark.parametrize("kind", ["mstate", "mfma_pass", "lds_pass", "plain_f64"])
def test_all_zero_window_after_ialm_dirtiers(kind):
    """A window of null frames alone stops before its first pass: "defined as zeros, zero iterations"
    (test_gpu_parity.py::test_ialm_vs_oracle_and_null_frames).  Nothing writes its sparse image, A or E: they are what the
    clearings of ialm_start left, in buffers that hold the dirtiers' images and factors."""
    zeros = np.zeros((21, 64, 96), np.uint8)
    if kind == "mstate":
        def victim(c):
            return _pick(c.batch_run(zeros, 1, 21))
        fresh = pair(victim, ialm_sequence("d64_then_d70", False), "all-zero window, M-state route")
        assert int(fresh["iters"][0]) == 0 and not fresh["nseg"].any()
        for key in STAGES:
            assert not fresh[key].any(), key
        return

    def victim(c):
        A, E, iters = c.ialm(zeros.reshape(21, -1))
        return dict(A=A, E=E, iters=np.array([iters], np.int32))
    variant = {"mfma_pass": 2, "lds_pass": 1, "plain_f64": 6}[kind]
    fresh = pair(victim, ialm_sequence("d64_then_d70", True), "all-zero window, " + kind, setup=_route_setup(variant, 0))
    assert int(fresh["iters"][0]) == 0 and not fresh["A"].any() and not fresh["E"].any()


@pytest.mark.parametrize("kind", ["mstate", "factors"])
def test_f64_start_and_forced_refinement_after_ialm_dirtiers(kind):
    """integer start off (k_ialm_stats and the f64 start pass instead of k_gram_u8) and the accurate first iteration forced for every
    window (ialm_refine.hip works in the B-matrix and Gram slots the dirtiers filled)"""
    def more(c):
        c.set_integer_start(0)
        c.set_start_refine(1e-12)
    for name in ("plain21", "n37", "dup"):
        what = "%s %s, f64 start, refinement forced" % (kind, name)
        if kind == "mstate":
            fresh = pair(_mstate_victim(name), ialm_sequence("d64_then_d70", False), what, setup=more)
            _check_mstate_image(name, fresh, what)
        else:
            fresh = pair(_factor_victim(name), ialm_sequence("d64_then_d70", True), what, setup=_route_setup(2, 0, more))
            _check_factors(name, fresh)


# ------------------------------------------------------------------ family 2: switch state
def _truncated(name, k):
    from swiftwatcher_amd import _lib
    frames = tc.frames(name)
    p = _lib.default_params()
    p.maxiter = k

    def run(c):
        return _pick(c.batch_run(frames, 1, frames.shape[0], params=p, stages=("rpca",)))
    return run


def test_backoff_after_a_failed_guess():
    """A run stopped by maxiter right after a pass whose sparse-image stores were switched off: the guess failed, the window runs
    again and the context keeps its guesses off for the next 64 batches.  Those 64 calls -- 63 of the victim and, in their middle,
    the truncated call again, which now cannot fail a guess -- and the two after them, when the guess is back, give the bytes of a
    fresh context; the truncated call then fails its guess again.  The rerun slots were filled before by d64 stopped at maxiter 2
    (three larger windows run again), and the 64 victim calls that follow it are held to the fresh bytes as well."""
    from swiftwatcher_amd import _lib
    name = "plain21"
    victim = _mstate_victim(name)
    fresh = _on_new_context(None, [victim])
    _check_mstate_image(name, fresh, "plain21 on a fresh context")
    # the first cap at which a fresh context's guess fails
    k_fail = None
    for k in range(1, tc.steps(name)):
        c = _lib.Context(0)
        fresh_trunc = _truncated(name, k)(c)
        failed = c.redo_windows
        c.close()
        if failed:
            k_fail = k
            break
    assert k_fail is not None, "no truncation of plain21 fails a guess: the case tests nothing"
    p = _lib.default_params()
    p.maxiter = 2
    c = _lib.Context(0)
    try:
        c.batch_run(hc.dirtier_frames(hc.D64), hc.D64.nwin, hc.D64.n, params=p)
        # d64's own guess fails where a truncated run's does: the context is backing off already.  64 victim calls bring the guesses back.
        for i in range(1, 65):
            hc.assert_same(fresh, victim(c), "call %d after d64 stopped at maxiter 2" % i)
        first = c.redo_windows
        got = _truncated(name, k_fail)(c)
        assert c.redo_windows == first + 1, "the truncated call's guess did not fail on this context"
        hc.assert_same(fresh_trunc, got, "the truncated call after d64")
        redo = c.redo_windows
        for i in range(1, 65):          # the 64 batches of the backoff
            if i == 32:
                hc.assert_same(fresh_trunc, _truncated(name, k_fail)(c), "backoff call %d (truncated)" % i)
                assert c.redo_windows == redo, "a guess was made during the backoff"
            else:
                hc.assert_same(fresh, victim(c), "backoff call %d" % i)
        for i in (65, 66):              # the guess is back
            hc.assert_same(fresh, victim(c), "call %d after the failed guess" % i)
        redo = c.redo_windows
        hc.assert_same(fresh_trunc, _truncated(name, k_fail)(c), "the truncated call once the guess is back")
        assert c.redo_windows == redo + 1, "the guess did not come back after 64 batches"
    finally:
        c.close()


def test_toggling_switches_away_and_back(orc):
    """every switch set to another value, a call made under it, and set back: the victim's bytes are a fresh context's"""
    name = "sparse_63x94"
    victim = _scene_victim(name)
    fresh = _on_new_context(None, [victim])
    _check_scene(orc, name, fresh, name)
    toggles = [("set_ialm_variant", (5, 2, 1, 6), 0), ("set_eig_method", (1,), 0), ("set_norm_guard", (0.0, 0.5), 1e-3),
               ("set_pass_tuning", (1, 2, 3), 0), ("force_ccl_multi_kernel", (True,), False)]
    from swiftwatcher_amd import _lib
    c = _lib.Context(0)
    try:
        for setter, values, default in toggles:
            for v in values:
                getattr(c, setter)(v)
                victim(c)          # a call under the other setting: it leaves that route's buffers and tables behind
                getattr(c, setter)(default)
                hc.assert_same(fresh, victim(c), "%s(%r) and back" % (setter, v))
    finally:
        c.close()


def test_a_refused_call_changes_nothing(orc):
    """one refusal of each family's existing refusal test between the dirtiers and the victim"""
    from swiftwatcher_amd import _lib
    import filter_planes as fp
    import stabilize_ref
    name = "sparse_67x95"
    rng = np.random.default_rng(0)
    frames, rect, anchor = stabilize_ref.designed_case(20, 28, 4, 2, seed=5)
    fam = next(f for f in fp.dense_families() if f.name == "dense_33x65")
    y, u, v = fc.yuv420_planes(10, 14)

    def refused(c):
        with pytest.raises(_lib.SwkError):          # test_gpu_parity.py::test_error_paths
            c.batch_run(rng.integers(0, 255, size=(129, 16, 16), dtype=np.uint8), 1, 129)
        with pytest.raises(_lib.SwkError):
            c.batch_run(rng.integers(0, 255, size=(4, 3, 16), dtype=np.uint8), 1, 4)
        with pytest.raises(_lib.SwkError):          # test_filter_planes_gpu.py::test_refusals
            c.debug_filter_fused(fam.planes, params=_lib.default_params(bil_d=11))
        with pytest.raises(_lib.SwkError, match="search"):          # test_stabilize_gpu.py::test_refusals_leave_the_context_working
            c.stabilize(frames, rect, 17, anchor)
        with pytest.raises(_lib.SwkError):          # test_yuv_gpu.py: a rectangle outside the frame
            c.yuv420_to_bgr(y, u, v, rect=(0, 0, 15, 10))
        with pytest.raises(_lib.SwkError):          # test_classifier.py: a crop side above 512
            c.classifier_input([np.zeros((513, 10, 3), np.uint8)], (0.5, 0.5, 0.5), (0.25, 0.25, 0.25))
    fresh = pair(_scene_victim(name), [d_dense_scene] + ialm_sequence("d64", False) + [refused], name + " after refusals")
    _check_scene(orc, name, fresh, name)


# ------------------------------------------------------------------ family 3: the filter chain and the labeller
def _fused(planes, p=None):
    def run(c):
        out = c.debug_filter_fused(planes, params=p)
        return {k: out[k] for k in ("bilateral", "thresh", "opened", "guard")}
    return run


def _fp_params(p, **more):
    from swiftwatcher_amd import _lib
    return _lib.default_params(bil_d=p.d, bil_sigma_color=p.sc, bil_sigma_space=p.ss, bil_fma=int(p.fma), thresh=int(p.thresh), **more)


def test_bilateral_tables_are_rebuilt_and_restored(orc):
    """(d, sigmas) A -> B -> A on one context, through swk_debug_filter_fused and through swk_batch_run: the cached tables are keyed
    by the triple, B's 81 taps overwrite A's 49 and A's must come back"""
    import filter_planes as fp
    from swiftwatcher_amd import _lib
    fam = next(f for f in fp.dense_families() if f.name == "dense_67x95")
    A, B = fp.P(7, 15.0, 1.0, 0, 15), fp.P(9, 40.0, 3.0, 0, 15)
    assert fp.radius(A.d, A.ss) == 3 and fp.radius(B.d, B.ss) == 4
    fresh = {k: _on_new_context(None, [_fused(fam.planes, _fp_params(p))]) for k, p in (("A", A), ("B", B))}
    for k, p in (("A", A), ("B", B)):
        for key, w in zip(("bilateral", "thresh", "opened"), fp.oracle_stages(fam.name, fam.planes, p)):
            assert np.array_equal(fresh[k][key], w), "fresh %s: %s differs from the oracle" % (k, key)
        assert (fresh[k]["guard"] == _lib.DEBUG_FILL).all()
    assert not np.array_equal(fresh["A"]["bilateral"], fresh["B"]["bilateral"])
    c = _lib.Context(0)
    try:
        for k in "ABABBA":
            hc.assert_same(fresh[k], _fused(fam.planes, _fp_params(A if k == "A" else B))(c), "debug_filter_fused %s in A B A B B A" % k)
    finally:
        c.close()
    # the same through the batch call
    name = "sparse_63x94"
    over = dict(bil_d=9, bil_sigma_color=40.0, bil_sigma_space=3.0)
    pA, pB = _lib.default_params(), _lib.default_params(**over)
    fa, fb = _on_new_context(None, [_scene_victim(name, pA)]), _on_new_context(None, [_scene_victim(name, pB)])
    _check_scene(orc, name, fa, name + " d = 7")
    _check_scene(orc, name, fb, name + " d = 9", **over)
    assert not np.array_equal(fa["bilateral"], fb["bilateral"])
    c = _lib.Context(0)
    try:
        for k in "ABAAB":
            hc.assert_same(fa if k == "A" else fb, _scene_victim(name, pA if k == "A" else pB)(c), "batch_run %s in A B A A B" % k)
    finally:
        c.close()


def test_threshold_and_connectivity_changed_and_changed_back(orc):
    from swiftwatcher_amd import _lib
    name = "sparse_67x95"
    variants = {"default": {}, "thresh40": dict(thresh=40), "4way_raster": dict(connectivity=4, label_order=0)}
    fresh = {}
    for k, over in variants.items():
        fresh[k] = _on_new_context(None, [_scene_victim(name, _lib.default_params(**over))])
        _check_scene(orc, name, fresh[k], "%s %s" % (name, k), **over)
    assert not np.array_equal(fresh["default"]["thresh"], fresh["thresh40"]["thresh"])
    c = _lib.Context(0)
    try:
        d_dense_scene(c)
        for k in ("default", "thresh40", "default", "4way_raster", "default", "thresh40"):
            hc.assert_same(fresh[k], _scene_victim(name, _lib.default_params(**variants[k]))(c), "%s after the others" % k)
    finally:
        c.close()


def _orc_fused(orc, planes, thresh=15):
    bil = fc.orc_bilateral(orc, planes, 7)
    thr = np.stack([orc.thresh_tozero_u8(b, thresh) for b in bil])
    return bil, thr, fc.orc_open(orc, thr, (3, 3))


@pytest.mark.parametrize("shape", [(70, 61), (33, 130), (9, 13)], ids=["narrower", "lower", "both"])
def test_filter_on_a_smaller_plane(orc, shape):
    """the fused filter on 21 planes smaller than the 40 bright planes of 70 x 130 before them, in W alone, in H alone and in both:
    its three outputs are cleared by three lines of swk_debug_filter_fused, its tiles read a ring of 4 px beyond the plane"""
    d, _ = hc.PLANE_PAIRS["filter_fused"]
    planes = fc.gray_planes(*shape, seed=5)[:21].copy()
    planes[:, :, :shape[1] // 3] = 0          # a third of every plane filters to 0 at every stage: the kernel stores nothing there
    fresh = pair(_fused(planes), [_fused(_bright_planes(d.count, d.H, d.W)), d_dense_scene], "fused filter %dx%d" % shape)
    want = _orc_fused(orc, planes)
    for key, w in zip(("bilateral", "thresh", "opened"), want):
        assert np.array_equal(fresh[key], w), key
    assert (want[0] == 0).mean() > 0.2 and want[0].any() and want[2].any()
    assert (fresh["guard"] == 0xA5).all()


def _ccl(img, conn, order, forced):
    def run(c):
        c.force_ccl_multi_kernel(forced)
        try:
            n, lab = c.ccl_u8(img, conn, order)
        finally:
            c.force_ccl_multi_kernel(False)
        return dict(ncomp=np.atleast_1d(np.asarray(n, np.int32)), labels=lab)
    return run


CCL_VICTIMS = ["spiral_64x96_gap1", "staircase_main_33x70", "diagonal_contacts_65", "row_wrap_5"]


@pytest.mark.parametrize("order", ["one_workgroup_after_forced", "forced_after_one_workgroup"])
@pytest.mark.parametrize("victim", CCL_VICTIMS)
def test_labeller_routes_after_each_other(orc, victim, order):
    """swk_ccl_u8 on a pattern of tests/ccl_patterns.py after 24 planes of 70 x 130 with 2,275 components each, labelled by
    the other route: the multi-kernel path re-initialises parent (0xFF), rootbits and the counts by one line each"""
    import ccl_patterns as cp
    case = next(c for c in cp.small_families() if c.name == victim)
    busy = _busy_masks(24, 70, 130)
    forced_victim = order == "forced_after_one_workgroup"
    for conn, lab_order in ((8, 1), (4, 0)):
        dirt = [_ccl(busy, conn, lab_order, not forced_victim), _ccl(busy, 4, 0, not forced_victim)]
        fresh = pair(_ccl(case.img, conn, lab_order, forced_victim), dirt, "%s %s %d-way" % (victim, order, conn))
        nref, ref = orc.ccl_u8(case.img, conn, lab_order)
        assert int(fresh["ncomp"][0]) == nref and np.array_equal(fresh["labels"], ref)


def test_records_with_fewer_labels(orc):
    """swk_regionprops_u8 and swk_segment_shapes_u8 on 21 planes of 9 x 13 with 1 .. 21 labels after 24 planes of 70 x 130 with all 255,
    and after the dense scene's batch (255 records a frame in the record slot): the box / sum tables and the record arrays are
    re-initialised per call"""
    labels = fc.label_planes(9, 13)[:21]
    busy = _busy_labels(24, 70, 130)

    def props(planes):
        def run(c):
            segs, nseg = c.regionprops_u8(planes)
            return dict(segs=segs, nseg=nseg)
        return run

    def shapes(planes):
        def run(c):
            recs, nseg = c.segment_shapes_u8(planes)
            return dict(shapes=recs, nseg=nseg)
        return run
    for forced in (False, True):
        def setup(c, forced=forced):
            c.force_ccl_multi_kernel(forced)
        fresh = pair(props(labels), [d_dense_scene, props(busy)], "regionprops_u8 forced=%s" % forced, setup=setup)
        segs, nseg = fc.orc_regionprops(orc, labels, 255)
        assert np.array_equal(fresh["nseg"], nseg) and np.array_equal(fresh["segs"], segs)
    # the one-workgroup labeller with records alone (swk_debug_ccl_frame_props): its record array is cleared by a line of its own
    masks = fc.binary_planes(9, 13)[:21]

    def frame_props(planes):
        def run(c):
            lab, segs, nseg = c.debug_ccl_frame_props(planes)
            return dict(labels=lab, segs=segs, nseg=nseg)
        return run
    fresh = pair(frame_props(masks), [d_dense_scene, frame_props(_busy_masks(24, 70, 130))], "debug_ccl_frame_props")
    lab8 = np.stack([orc.labels_to_u8(orc.ccl_u8(m, 8, 1)[1]) for m in masks])
    segs, nseg = fc.orc_regionprops(orc, lab8, 255)
    assert np.array_equal(fresh["labels"], lab8) and np.array_equal(fresh["nseg"], nseg) and np.array_equal(fresh["segs"], segs)
    fresh = pair(shapes(labels), [d_dense_scene, shapes(busy), props(busy)], "segment_shapes_u8")
    recs, nseg = fc.ref_shapes(labels, 255)
    assert np.array_equal(fresh["nseg"], nseg)
    for key in ("label", "m", "border", "perim", "quads"):
        assert np.array_equal(fresh["shapes"][key], recs[key]), key


# ------------------------------------------------------------------ family 4: swk_batch_run_groups
@functools.lru_cache(maxsize=None)
def _group_rois():
    tiny = roi_stack(1010, 1, 4, 5)
    small = roi_stack(1020, 1, 47, 94)
    assert [(1,) + r.shape[1:3] for r in (tiny, hc.scene_roi("sparse_63x94"), small)] == hc.GROUPS_VICTIM
    return tiny, np.ascontiguousarray(hc.scene_roi("sparse_63x94")), small


def _groups_victim(params=None):
    def run(c):
        specs = [dict(frames=r, nwin=1, n=hc.GROUPS_N) for r in _group_rois()]
        out = {}
        for g, res in enumerate(c.batch_run_groups(specs, params=params)):
            out.update({"g%d_%s" % (g, k): v for k, v in _pick(res).items()})
        return out
    return run


def _d_groups(params=None):
    """a groups call of d64-sized windows: descriptor tables of 2 x 3 windows and 384 frames"""
    def run(c):
        f = hc.dirtier_frames(hc.D64)
        c.batch_run_groups([dict(frames=f, nwin=hc.D64.nwin, n=hc.D64.n), dict(frames=f[:, :60, :100].copy(), nwin=hc.D64.nwin, n=hc.D64.n)],
                           params=params)
    return run


@pytest.mark.parametrize("case", ["full", "truncated"])
def test_groups_call_after_a_dense_call(orc, case):
    """A call mixing a P < n group (4 x 5), the 63 x 94 scene and a 47 x 94 group padded to the scene's pitch, n = 21, after a dense
    single-group call of three saturated windows of 70 x 129 with 21 frames each: the padding pixels p >= H * W of the small group's X
    planes, which the IALM reads as zeros, lie where that call's pixels lay.  truncated: at maxiter 2 (a failed guess: the windows
    run again through the rerun slots, SL_REDO_P included, which a truncated groups call of larger windows filled)."""
    from swiftwatcher_amd import _lib
    p = None
    dense21 = hc.saturated_frames(3, 21, 70, 129, 21001)
    dirt = [lambda c: c.batch_run(dense21, 3, 21), d_dense_scene]
    if case == "truncated":
        p = _lib.default_params(maxiter=2)
        dirt = [_d_groups(p)] + dirt
    fresh = pair(_groups_victim(p), dirt, "groups call, " + case)
    rois = _group_rois()
    for g, roi in enumerate(rois):
        res = {k[3:]: v for k, v in fresh.items() if k.startswith("g%d_" % g)}
        if case == "full":
            ref = orc.window(np.ascontiguousarray(roi))
            for key in ("gray", "rpca", "opened", "labels"):          # helpers.check_against_oracle's stages
                assert np.array_equal(res[key], ref[key]), "group %d: %s vs oracle" % (g, key)
            for i in range(hc.GROUPS_N):
                assert seg_tuples(res, i) == orc_seg_tuples(ref["segments"][i]), (g, i)
        else:
            # the masked image comparison at iterate 2
            gray = np.stack([orc.bgr2gray(np.ascontiguousarray(f)) for f in roi])
            it = tc.trajectory(gray.reshape(hc.GROUPS_N, -1).T, maxiter=2)[-1]
            img = orc.rpca_epilogue(it.E).T.reshape(gray.shape)
            mask = tc.boundary_mask(it.E, tc.BAND).T.reshape(gray.shape)
            assert int(res["iters"][0]) == 2
            assert not ((res["rpca"] != img) & ~mask).any(), "group %d: iterate 2 differs from the oracle's outside the mask" % g


def test_single_group_call_after_a_groups_call(orc):
    """the descriptor tables in SL_GRP describe six windows of other sizes: a one-group call must not consult them"""
    name = "sparse_67x95"
    fresh = pair(_scene_victim(name), [_d_groups(), _groups_victim()], name + " after groups calls")
    _check_scene(orc, name, fresh, name)


# ------------------------------------------------------------------ family 5: the hand-over to the classifier
def _cut(c, frames, records, counts, cap, net_cap, pad=8):
    """swk_segment_inputs on device frames and records -> (total, skipped, net rows, seg_frame) as arrays"""
    import torch
    from swiftwatcher_amd import _lib
    from swiftwatcher_amd.segment_classification import IMAGENET_MEAN, IMAGENET_STD
    dev = torch.device("cuda", 0)
    F, fh, fw = frames.shape[:3]
    dframes = torch.from_numpy(np.ascontiguousarray(frames)).to(dev)
    segs = torch.from_numpy(records.view(np.uint8).reshape(F, cap, 48)).to(dev)
    nseg = torch.from_numpy(counts).to(dev)
    side = 24 + 2 * pad
    x = torch.full((net_cap, 3, side, side), -7.25, dtype=torch.float32, device=dev)
    fidx = torch.full((net_cap,), -99, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    inp = _lib.Input(frames=dframes.data_ptr(), mem=_lib.MEM_DEVICE, channels=3, nwin=1, n=F, Hc=fh, Wc=fw, x0=0, y0=0,
                     frame_stride=fh * fw * 3, row_stride=fw * 3)
    total, skipped = c.segment_inputs(inp, (fh, fw), segs.data_ptr(), nseg.data_ptr(), cap, IMAGENET_MEAN, IMAGENET_STD,
                                      x.data_ptr(), net_cap, pad=pad, seg_frame_ptr=fidx.data_ptr())
    return dict(counts=np.array([total, skipped], np.int32), net=x.cpu().numpy(), seg_frame=fidx.cpu().numpy())


def test_segment_inputs_counts_are_the_calls_own():
    """swk_segment_inputs on two small frames with five boxes of 24 .. 61 px after a call that listed three boxes of 513 px and above
    and one of 4097 rows (skipped): total, skipped and every network input are the victim's own.  The skipped-box counter and the
    large-box list are re-initialised by one line each."""
    import pil_resize_ref as P
    from swiftwatcher_amd import _lib
    from swiftwatcher_amd.segment_classification import IMAGENET_MEAN, IMAGENET_STD
    big = P.formula_image(4097, 600)[None]
    brec = np.zeros((1, 8), _lib.SEGMENT_DTYPE)
    for i, (r0, c0, h, w) in enumerate([(0, 0, 4097, 24), (0, 30, 513, 24), (10, 60, 600, 520), (700, 0, 24, 513), (900, 100, 40, 50)]):
        brec[0, i] = (i + 1, r0, c0, r0 + h, c0 + w, 0, h * w, 0, 0)
    bcount = np.array([5], np.int32)
    small = np.stack([P.formula_image(70, 130, offset=7), P.formula_image(70, 130, offset=55)])
    boxes = [(0, 3, 5, 24, 24), (0, 20, 40, 37, 61), (0, 30, 2, 25, 31), (1, 0, 0, 24, 24), (1, 9, 60, 61, 37)]
    srec = np.zeros((2, 4), _lib.SEGMENT_DTYPE)
    scount = np.zeros(2, np.int32)
    for f, r0, c0, h, w in boxes:
        srec[f, scount[f]] = (scount[f] + 1, r0, c0, r0 + h, c0 + w, 0, h * w, 0, 0)
        scount[f] += 1

    def dirtier(c):
        out = _cut(c, big, brec, bcount, 8, 8)
        assert out["counts"].tolist() == [5, 1], "the dirtier lists five boxes and skips the one of 4097 rows"

    fresh = pair(lambda c: _cut(c, small, srec, scount, 4, 8), [dirtier], "segment_inputs after large and skipped boxes")
    assert fresh["counts"].tolist() == [5, 0]
    assert fresh["seg_frame"].tolist() == [0, 0, 0, 1, 1, -99, -99, -99]
    assert (fresh["net"][5:] == -7.25).all()
    # test_large_crops_gpu.py's expectation: the restated patches through the <= 512 kernel, where a 24 x 24 crop passes through
    patches = [P.patch(small[f, r0:r0 + h, c0:c0 + w]) for f, r0, c0, h, w in boxes]
    exp = _on_new_context(None, [lambda c: c.classifier_input(patches, IMAGENET_MEAN, IMAGENET_STD, pad=8)[1]])
    np.testing.assert_array_equal(fresh["net"][:5], exp)


def test_segment_inputs_last_serves_only_the_last_batch():
    """swk_segment_inputs_last with the generation of a batch that a later call has replaced is refused, at the wrapper and in the
    library (a call that reuses the record slots invalidates the batch); with the last batch's generation it gives what a fresh
    context gives, counts included"""
    import torch
    from swiftwatcher_amd import _lib
    from swiftwatcher_amd.segment_classification import IMAGENET_MEAN, IMAGENET_STD
    busy, name = "sparse_64x96", "sparse_63x94"

    def cut_last(c, gen, cap=64):
        x = torch.full((cap, 3, 40, 40), -7.25, dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        total, skipped = c.segment_inputs_last(gen, IMAGENET_MEAN, IMAGENET_STD, x.data_ptr(), cap)
        return dict(counts=np.array([total, skipped], np.int32), net=x.cpu().numpy())

    def victim(c):
        res = c.batch_run(hc.scene_roi(name), 1, 21, stages=())
        out = cut_last(c, res["generation"])
        out["nseg"], out["segs"] = res["nseg"], res["segs"]
        return out

    def dirtier(c):
        old = c.batch_run(hc.scene_roi(busy), 1, 21, stages=())
        newer = c.batch_run(hc.scene_roi(name), 1, 21, stages=())
        with pytest.raises(_lib.StaleBatch):
            cut_last(c, old["generation"])
        served = cut_last(c, newer["generation"])
        # a stage call that reuses the record slots: the library itself refuses the batch now, whatever the wrapper's count says
        c.regionprops_u8(_busy_labels(24, 70, 130))
        with pytest.raises(_lib.StaleBatch):
            cut_last(c, newer["generation"])
        return served
    fresh = pair(victim, [dirtier], "segment_inputs_last")
    from swiftwatcher_amd import image_filtering as img
    total = int(fresh["counts"][0])
    ref = hc.scene_oracle(name)
    assert fresh["counts"][1] == 0 and total == int(fresh["nseg"].sum()) == sum(len(s) for s in ref["segments"]) > 64
    # the first 64 segments (frame order, then ascending label) against the host's crops of the same records, through
    # swk_classifier_input_window (Pillow-exact: test_classifier.py)
    roi, crops = hc.scene_roi(name), []
    for f in range(21):
        rps = img.regionprops_from_records(fresh["segs"][f, :fresh["nseg"][f]])
        crops += img.extract_segment_images(rps, roi[f], (24, 24), [(0, 0), (roi.shape[2], roi.shape[1])])
    exp = _on_new_context(None, [lambda c: c.classifier_input(crops[:64], IMAGENET_MEAN, IMAGENET_STD, pad=8)[1]])
    np.testing.assert_array_equal(fresh["net"], exp)


def test_classifier_input_with_fewer_and_smaller_crops(golden_dir):
    """swk_classifier_input_window of ten crops of at most 80 px after forty of up to 300 px (packed crops, offsets, sizes, patches and
    the host network input each in a slot of their own): Pillow-exact patches, as test_classifier.py asserts them"""
    from PIL import Image
    from oracle import classifier_ref as ref
    g = np.load(os.path.join(golden_dir, "classifier_model_pt.npz"))
    crops = [g["crop%d" % i] for i in range(hc.CROPS_VICTIM[0])]
    assert max(max(c.shape[:2]) for c in crops) <= hc.CROPS_VICTIM[1]
    rng = np.random.default_rng(3)
    many = [rng.integers(0, 256, size=(int(rng.integers(100, 301)), int(rng.integers(100, 301)), 3), dtype=np.uint8) for _ in range(hc.CROPS_DIRTIER[0])]

    def call(images):
        def run(c):
            patches, net = c.classifier_input(images, ref.MEAN, ref.STD, want_patches=True)
            return dict(patches=patches, net=net)
        return run
    fresh = pair(call(crops), [call(many)], "classifier_input")
    bil = getattr(Image, "Resampling", Image).BILINEAR
    for i, c in enumerate(crops):
        np.testing.assert_array_equal(fresh["patches"][i], np.asarray(Image.fromarray(c).resize((24, 24), bil)))
        np.testing.assert_array_equal(fresh["net"][i], ref.transform(c)[0].numpy())


# ------------------------------------------------------------------ family 6: the stand-alone calls
STYLES = [(0, 255, 0, 48, 256), (0, 0, 255, 128, 255), (0, 255, 255, 1, 200), (255, 128, 0, 40, 0), (255, 255, 255, 0, 256), (0, 0, 0, 160, 0)]
REVIEW_RECT = (2, 1, 13, 9)          # (x0, y0, Wc, Hc) inside 11 x 16 frames


def _overlay(count, text, H=9, W=13):
    boxes, marks, labels = [], [], []
    for f in range(count):
        boxes += [(f, f % 4, 1 + f % 5, min(H, 5 + f % 4), min(W, 8 + f % 5), 1 + f % 2), (f, -1, 6, 4, 20, 2)]
        marks += [(f, 4 + f % 3, 3 + f % 7, 3)]
        labels += [(f, 1, 1 + f % 3, 5, 6, 1, "F%d" % (f % 10))]
    kw = dict(boxes=boxes, marks=marks, styles=STYLES, mark_arm=2, border=1, frame_style=np.array([f % 3 == 0 for f in range(count)], np.int32))
    if text:
        kw["labels"] = labels
    return kw


def _tuple_out(call):
    def run(c):
        out = call(c)
        out = out if isinstance(out, (tuple, list)) else (out,)
        flat = []
        for o in out:
            flat += list(o) if isinstance(o, (tuple, list)) else [o]
        return {"out%d" % i: o for i, o in enumerate(flat) if o is not None}
    return run


def _stand_alone(kind, orc):
    """(victim call, its larger twin, check(fresh)) of one stand-alone entry point"""
    import review_ref as rref
    import review_text_ref as tref
    from swiftwatcher_amd import _lib
    big_bgr = _bright_bgr(30, 70, 130)
    big_rect = (3, 2, 121, 65)
    frames = fc.bgr_frames(11, 16, seed=3)[:21]
    x0, y0, Wc, Hc = REVIEW_RECT
    crop = frames[:, y0:y0 + Hc, x0:x0 + Wc]

    def equal(want):
        def check(fresh):
            got = [fresh[k] for k in sorted(fresh, key=lambda s: int(s[3:]))]
            assert len(got) == len(want)
            for i, (g, w) in enumerate(zip(got, want)):
                if w.dtype.names:
                    for key in w.dtype.names:
                        assert np.array_equal(g[key], w[key]), "%s output %d field %s" % (kind, i, key)
                else:
                    assert g.dtype == w.dtype and np.array_equal(g, w), "%s output %d differs from the restatement" % (kind, i)
        return check

    if kind in ("stabilize", "stabilize_subpel"):
        import stabilize_ref
        import stabilize_subpel_ref as sref
        mod = stabilize_ref if kind == "stabilize" else sref
        (cv, Hv, Wv, Sv), (cd, Hd, Wd, Sd) = hc.STAB_VICTIM, hc.STAB_DIRTIER
        vf, vrect, vanchor = mod.designed_case(Hv, Wv, Sv, cv, seed=11, x_res=1)
        df, drect, danchor = mod.designed_case(Hd, Wd, Sd, cd, seed=12)
        if kind == "stabilize":
            want = stabilize_ref.stabilize(vf, vrect, Sv, vanchor)
            want = [want[0], want[1], want[2]]
        else:
            recs, (tab, sub), pixels = sref.stabilize_subpel(vf, vrect, Sv, vanchor)
            want = [recs, tab, sub, pixels]
        fn = "stabilize" if kind == "stabilize" else "stabilize_subpel"
        return (_tuple_out(lambda c: getattr(c, fn)(vf, vrect, Sv, vanchor, table=True)),
                _tuple_out(lambda c: getattr(c, fn)(df, drect, Sd, danchor, table=True)), equal(want))
    if kind == "bgr_to_yuv420":
        return (_tuple_out(lambda c: c.bgr_to_yuv420(frames, rect=REVIEW_RECT)), _tuple_out(lambda c: c.bgr_to_yuv420(big_bgr, rect=big_rect)),
                equal(list(rref.yuv420(crop))))
    if kind in ("render_review", "render_review_text"):
        text = kind.endswith("text")
        font = _lib.review_font() if text else None
        kw, big_kw = _overlay(21, text), _overlay(30, text, 65, 121)
        want = tref.render(crop, font=font, **kw) if text else rref.render(crop, **kw)
        return (_tuple_out(lambda c: c.render_review(frames, rect=REVIEW_RECT, **kw)),
                _tuple_out(lambda c: c.render_review(big_bgr, rect=big_rect, mask=_busy_masks(1, 65, 121)[0], mask_style=4, **big_kw)), equal(list(want)))
    if kind == "render_review_panels":
        from review_panels_ref import panel_cell, paste
        font, palette = _lib.review_font(), _lib.review_label_palette().astype(np.int64)
        planes = [fc.gray_planes(Hc, Wc, seed=4)[:21], fc.label_planes(Hc, Wc, seed=2)[:21]]
        specs = [dict(kind="gray", gain=2, layers=0, caption=(1, 1, 5, 6, 1, "G")), dict(kind="labels", layers=0, caption=(1, 1, 3, 0, 1, "L"))]
        overlay = dict(styles=STYLES, mark_arm=2, border=1)
        cells = [tref.render(crop, font=font, **overlay)]
        cells += [panel_cell(p, s["kind"], s.get("gain", 1), s["layers"], s["caption"], overlay, font, palette) for p, s in zip(planes, specs)]
        want = paste(cells, Hc, Wc, 2)
        big_planes = [_bright_planes(30, 65, 121), _busy_labels(30, 65, 121)]

        def call(fr, pl, rect):
            panels = [dict(plane=np.ascontiguousarray(p), **s) for p, s in zip(pl, specs)]
            return lambda c: c.render_review_panels(np.ascontiguousarray(fr), panels=panels, cols=2, rect=rect, **overlay)
        return _tuple_out(call(frames, planes, REVIEW_RECT)), _tuple_out(call(big_bgr, big_planes, big_rect)), equal(list(want))
    if kind in ("yuv420_to_bgr", "yuv_to_bgr"):
        import yuv_formats_ref as yref
        import yuv_ref
        H, W, rect = 10, 14, (3, 1, 11, 9)
        rng = np.random.default_rng(5)
        by, bu, bv = (rng.integers(0, 256, size=s, dtype=np.uint8) for s in ((30, 70, 130), (30, 35, 65), (30, 35, 65)))
        if kind == "yuv420_to_bgr":
            y, u, v = (a[:21] for a in fc.yuv420_planes(H, W))
            return (_tuple_out(lambda c: c.yuv420_to_bgr(y, u, v, rect=rect)), _tuple_out(lambda c: c.yuv420_to_bgr(by, bu, bv)),
                    equal([yuv_ref.bgr(y, u, v, rect)]))
        ch, cw = yref.chroma_shape(H, W, 1, 0)
        y, u, v = (rng.integers(0, 256, size=s, dtype=np.uint8) for s in ((21, H, W), (21, ch, cw), (21, ch, cw)))
        bu2, bv2 = (rng.integers(0, 256, size=(30, 70, 65), dtype=np.uint8) for _ in range(2))
        return (_tuple_out(lambda c: c.yuv_to_bgr(y, u, v, subsampling=(1, 0), bits=8, rect=rect)),
                _tuple_out(lambda c: c.yuv_to_bgr(by, bu2, bv2, subsampling=(1, 0), bits=8)), equal([yref.bgr(y, u, v, rect, subsampling=(1, 0), bits=8)]))
    if kind == "grey_open_u8":
        planes = fc.gray_planes(9, 13, seed=2)[:21]
        return (_tuple_out(lambda c: c.grey_open_u8(planes, (4, 7))), _tuple_out(lambda c: c.grey_open_u8(_bright_planes(40, 70, 130), (4, 7))),
                equal([fc.orc_open(orc, planes, (4, 7))]))
    if kind == "resize_linear_u8":
        frame = fc.bgr_frames(9, 13, seed=8)[0]
        return (_tuple_out(lambda c: c.resize_linear_u8(frame, (20, 15))), _tuple_out(lambda c: c.resize_linear_u8(big_bgr[0], (300, 150))),
                equal([orc.resize_linear_u8(frame, (20, 15))]))
    assert kind == "ccl_u8"
    planes = fc.binary_planes(9, 13)[:21]
    ncomp, lab = fc.orc_ccl(orc, planes, 8, 1)
    return _tuple_out(lambda c: c.ccl_u8(planes, 8, 1)), _tuple_out(lambda c: c.ccl_u8(_busy_masks(24, 70, 130), 8, 1)), equal([ncomp, lab])


STAND_ALONE = ["stabilize", "stabilize_subpel", "render_review", "render_review_text", "render_review_panels", "bgr_to_yuv420",
               "yuv420_to_bgr", "yuv_to_bgr", "grey_open_u8", "resize_linear_u8", "ccl_u8"]


@pytest.mark.parametrize("kind", STAND_ALONE)
def test_stand_alone_calls(orc, kind):
    """each entry point on small frames after its own larger twin (smaller search range, fewer and smaller frames) and after
    another family's leftovers; the victim equals the numpy restatement its own module is held to"""
    victim, twin, check = _stand_alone(kind, orc)
    check(pair(victim, [twin], kind + " after its larger twin"))
    pair(victim, [d_unrelated, twin, d_unrelated], kind + " after another family's calls")


# ------------------------------------------------------------------ family 7: the Python level
DEVICE_BOXES = [(0, 3, 5, 24, 24), (0, 20, 40, 37, 61), (0, 30, 2, 25, 31), (1, 0, 0, 24, 24), (1, 9, 60, 61, 37)]          # frame, r0, c0, h, w


def _device_frames():
    import pil_resize_ref as P
    return np.stack([P.formula_image(70, 130, offset=7), P.formula_image(70, 130, offset=55)])


CLASSIFIER_CHILD = r"""
import os, sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
from swiftwatcher_amd import _lib
from swiftwatcher_amd.segment_classification import SegmentClassifier
import test_history_independence_gpu as T
g = np.load(os.path.join(sys.argv[1], "tests", "golden", "classifier_model_pt.npz"))
crops = [g["crop%d" % i] for i in range(int(g["count"]))]
sd = {k[2:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("w:")}
rng = np.random.default_rng(9)
others = [rng.integers(0, 256, size=(int(rng.integers(24, 90)), int(rng.integers(24, 90)), 3), dtype=np.uint8) for _ in range(700)]
keys = np.arange(1000, 1000 + len(crops), dtype=np.uint64)
fresh = SegmentClassifier.from_state_dict(sd)
used = SegmentClassifier.from_state_dict(sd)
assert used._use_graphs == (os.environ["SWK_HIP_GRAPHS"] == "1")
out = {}
sets = {"bucket64": crops[:40], "bucket128": crops, "two_streams": (crops * 7)[:600]}
assert [fresh._bucket(len(s)) for s in sets.values()] == [64, 128, 1024] and fresh._split_rows == 1024

# the device-resident route: the classifier's input slots, and with graphs on the captured forward of a bucket
frames = T._device_frames()
many = [(f, 2 * (k % 20), 3 * (k % 30), 24 + k % 7, 24 + k % 11) for f in (0, 1) for k in range(50)]
def device_scores(clf, ctx, boxes, cap):
    rec = np.zeros((2, cap), _lib.SEGMENT_DTYPE)
    cnt = np.zeros(2, np.int32)
    for f, r0, c0, h, w in boxes:
        rec[f, cnt[f]] = (cnt[f] + 1, r0, c0, r0 + h, c0 + w, 0, h * w, 0, 0)
        cnt[f] += 1
    dev = torch.device("cuda", 0)
    df = torch.from_numpy(frames).to(dev)
    segs, nseg = torch.from_numpy(rec.view(np.uint8).reshape(2, cap, 48)).to(dev), torch.from_numpy(cnt).to(dev)
    fh, fw = frames.shape[1:3]
    inp = _lib.Input(frames=df.data_ptr(), mem=_lib.MEM_DEVICE, channels=3, nwin=1, n=2, Hc=fh, Wc=fw, x0=0, y0=0,
                     frame_stride=fh * fw * 3, row_stride=fw * 3)
    torch.cuda.synchronize()
    s, fidx = clf.scores_from_device(ctx, inp, (fh, fw), segs, nseg, cap)
    return s.cpu().numpy(), fidx.cpu().numpy()

for name, s in sets.items():
    out["fresh_" + name] = fresh.scores(s).cpu().numpy()
out["fresh_dropout"] = fresh.dropout_scores(crops, keys, samples=8, seed=5).cpu().numpy()
ctx = _lib.Context(0)
out["fresh_device"], out["fresh_device_frames"] = device_scores(fresh, ctx, T.DEVICE_BOXES, 4)
used.scores(others)                       # 700 rows: the 1024-row tiles, two streams
used.scores(others[:100])                 # the 128-row bucket
used.dropout_scores(others[:200], np.arange(200, dtype=np.uint64), samples=8, seed=6)
big, _ = device_scores(used, ctx, many, 64)
assert big.shape == (100, 2)
for name, s in sets.items():
    out["after_" + name] = used.scores(s).cpu().numpy()
out["after_dropout"] = used.dropout_scores(crops, keys, samples=8, seed=5).cpu().numpy()
out["after_device"], out["after_device_frames"] = device_scores(used, ctx, T.DEVICE_BOXES, 4)
out["again_device"], _ = device_scores(used, ctx, T.DEVICE_BOXES, 4)          # graphs on: the bucket's captured forward, replayed
ctx.close()
np.savez(sys.argv[2], graph_error=str(used._graph_error), graphs_captured=len(used._graphs), **out)
"""


@functools.lru_cache(maxsize=None)
def _cpu_scores(golden_dir):
    """test_cnn_accuracy.py layer 3: the float32 and the float64 CPU forward of the fixture weights on the fixture's 96 crops, then on
    the five crops of the device-resident route"""
    import torch
    from swiftwatcher_amd.segment_classification import SegmentClassifier, SqueezeNet10
    g = np.load(os.path.join(golden_dir, "classifier_model_pt.npz"))
    crops = [g["crop%d" % i] for i in range(int(g["count"]))]
    frames = _device_frames()
    crops += [np.ascontiguousarray(frames[f, r0:r0 + h, c0:c0 + w]) for f, r0, c0, h, w in DEVICE_BOXES]
    sd = {k[2:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("w:")}
    x = SegmentClassifier.from_state_dict(sd, device="cpu", cropped=False).preprocess(crops)
    out = []
    for dtype in (torch.float32, torch.float64):
        m = SqueezeNet10(2)
        m.load_state_dict(sd, strict=True)
        m = m.to(dtype).eval()
        with torch.no_grad():
            out.append(torch.cat([m(x[i:i + 16].to(dtype)) for i in range(0, len(crops), 16)]).double().numpy())
    return out


@pytest.mark.parametrize("graphs", ["1", "0"], ids=["graphs_on", "graphs_off"])
def test_classifier_scores_do_not_depend_on_earlier_batches(golden_dir, tmp_path, graphs):
    """SegmentClassifier on the fixture weights, in a fresh child process per setting of SWK_HIP_GRAPHS.  The scores of the fixture's
    96 segments -- as 40 (the 64-row bucket), 96 (128 rows) and 600 (1024 rows, two streams) --, their dropout scores under a fixed
    seed, and the scores of five segments cut on the device (the classifier's input slots: 'rows past k hold an earlier chunk:
    scored, dropped'; with graphs on, the captured forward of the bucket) are the same bits from a fresh classifier and from one that
    first scored 700, 100, 200 and, on the device route, 100 other segments.  The 96 and the five are held to the float64 forward with
    test_cnn_accuracy.py's layer-3 bound."""
    import cnn_refs as R
    out = str(tmp_path / "scores.npz")
    env = dict(os.environ, SWK_HIP_GRAPHS=graphs)
    run = subprocess.run([sys.executable, "-c", CLASSIFIER_CHILD, ROOT, out], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                         text=True, timeout=600)
    assert run.returncode == 0, run.stdout[-4000:]
    got = np.load(out)
    assert str(got["graph_error"]) == "None" and (int(got["graphs_captured"]) > 0) == (graphs == "1")
    for name in ("bucket64", "bucket128", "two_streams", "dropout", "device", "device_frames"):
        hc.assert_same({name: got["fresh_" + name]}, {name: got["after_" + name]}, "classifier %s, graphs %s" % (name, graphs))
    hc.assert_same({"device": got["fresh_device"]}, {"device": got["again_device"]}, "classifier device route, second call, graphs %s" % graphs)
    assert got["fresh_device_frames"].tolist() == [b[0] for b in DEVICE_BOXES]
    s32, s64 = _cpu_scores(golden_dir)
    scale, e32 = float(np.abs(s64).max()), float(np.abs(s32 - s64).max())
    bound = max(R.FACTOR * e32, R.FLOOR * scale)
    gpu = np.concatenate([got["fresh_bucket128"], got["fresh_device"]]).astype(np.float64)
    err = float(np.abs(gpu - s64).max())
    print("HISTORY classifier graphs %s: max |gpu - f64| %.3g, |cpu32 - f64| %.3g, bound %.3g" % (graphs, err, e32, bound))
    assert err <= bound


def test_framequeue_planes_from_the_pool(orc):
    """FrameQueue windows whose stage planes come from Context._plane_pool after a busier window of the same byte count (93 x 66 after
    66 x 93) was given back: the stage images read later are the oracle's and those of a fresh Context's host outputs"""
    from swiftwatcher_amd import _lib, synthetic
    from swiftwatcher_amd.data_structures import FrameQueue
    n = 21
    regions = {"first": [(40, 30), (40 + 93, 30 + 66)], "second": [(40, 30), (40 + 66, 30 + 93)]}
    names = {"grayscale": "gray", "RPCA": "rpca", "bilateral": "bilateral", "thresh_15": "thresh", "opened": "opened", "cc_labeling": "labels"}
    ctx = _lib.default_context(0)
    pool_key = (21 * 66 * 93 + 3) // 4 * 4 * 6
    q = FrameQueue()
    held = None
    for which, seed, birds in (("first", 31, 8), ("second", 32, 3)):
        region = regions[which]
        frames = synthetic.full_frames(seed, n, region, frame_hw=(128, 200), birds=birds, bird_len=(8, 12), bird_wid=(3, 5))
        q.push_list_of_frames([frames[i] for i in range(n - 1, -1, -1)], list(range(n)), ["t"] * n)
        q.preprocess_queue(region, None)
        before = len(ctx._plane_pool.get(pool_key, []))
        q.segment_queue((24, 24), region)
        window = [q.pop_frame() for _ in range(n)][::-1]
        if which == "first":
            for f in window:          # read once, so the planes are known to be written, then give the buffer back
                f.get_processed_frame("opened")
            del window, f
            gc.collect()
            assert len(ctx._plane_pool.get(pool_key, [])) == before + 1, "the first window's planes did not go back to the pool"
        else:
            assert before >= 1 and len(ctx._plane_pool.get(pool_key, [])) == before - 1, "the second window did not take the pooled buffer"
            held = (window, frames, region)
    window, frames, ((x0, y0), (x1, y1)) = held
    roi = np.ascontiguousarray(frames[:, y0:y1, x0:x1])
    ref = orc.window(roi)
    lone = _on_new_context(None, [lambda c: c.batch_run(roi, 1, n)])
    for pos in range(n):
        for name, key in names.items():
            img = window[pos].get_processed_frame(name)
            assert np.array_equal(img, lone[key][pos]), "frame %d %s: not a fresh context's bytes" % (pos, name)
            assert np.array_equal(img, ref[key][pos]), "frame %d %s: not the oracle's" % (pos, name)
