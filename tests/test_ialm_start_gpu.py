"""The start of the IALM on the GPU (swk_debug_ialm_start: k_gram_u8 or k_ialm_stats, k_ialm_init, the MODE 0 start pass of every
pass variant, k_gram_reduce) against the references of tests/ialm_start_cases.py, window by window:

  statistics    sum of squares and maximum: exact, from either kernel
  start choice  int_gram is the host-side statement of k_ialm_init's rule, also next to the switch
  scalars       dual_norm, mu_0, thr_0, dnorm within 2 ulp of the float64 restatement
  integer G     bit for bit the int64 X^T X; symmetric; its trace is the sum of squares
  f64 G         of a window that clips nothing: M_1 = c X, so |G - c^2 X^T X| <= (P + 16) 2^-53 c^2 X^T X entrywise -- (P - 1) u for the
                sum of P non-negative products in any order, 2 u for the rounding of each factor's element of M_1 twice over,
                u for the product, the rest slack for the slab sums (derived, not measured; one dropped pixel is about 1 / P);
                of a window that clips: |G - M_1^T M_1| <= (P + 16) 2^-53 |M_1|^T |M_1| against the float64 M_1 of the restatement,
                whose Gram matrix is formed in long double

Every shape runs twice: at the reference's lmbda = 0.01, where most of these small windows clip (the f64 start passes), and at
lmbda = 4, where none can (k_gram_u8 at every shape, block count and alignment)."""
import numpy as np
import pytest

import ialm_start_cases as cases
from ialm_start_cases import LMBDA, LMBDA_ALL, U

pytestmark = pytest.mark.gpu

# (pass variant, integer-start switch).  Variant 6 never takes the integer start (plan_ialm): with the switch on it must behave as off.
COMBOS = [(1, 1), (2, 1), (4, 1), (5, 1), (1, 0), (2, 0), (4, 0), (5, 0), (6, 0), (6, 1)]
COMBO_IDS = ["v%d_%s" % (v, "int" if on else "f64") for v, on in COMBOS]


@pytest.fixture(scope="module")
def ctx():
    from swiftwatcher_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def _run(ctx, combo, x, lmbda):
    variant, on = combo
    ctx.set_ialm_variant(variant)
    ctx.set_integer_start(on)
    res = ctx.debug_ialm_start(x, lmbda)
    assert res["gram8_ran"] == int(bool(on) and variant != 6)
    return res


def _within(G, ref, scale, P, what):
    """|G - ref| <= (P + 16) u scale entrywise, in long double"""
    err = np.abs(G.astype(np.longdouble) - ref)
    bound = (P + 16) * np.longdouble(U) * scale
    bad = err > bound
    worst = float((err / np.where(bound > 0, bound, 1)).max())
    assert not bad.any(), "%s: %d entries over the bound, worst error / bound = %.3g" % (what, int(bad.sum()), worst)


def _check_window(res, w, ref, combo, P, what):
    variant, on = combo
    what = "%s window %d (variant %d, integer start %s)" % (what, w, variant, "on" if on else "off")
    G = res["G"][w]
    assert int(res["sumsq"][w]) == ref["sumsq"], what
    assert int(res["maxv"][w]) == ref["maxv"], what
    for key in ("dual_norm", "mu_0", "thr_0", "dnorm"):
        got, want = float(res[key][w]), float(ref[key])
        assert abs(got - want) <= 2 * np.spacing(want), "%s: %s = %r, restatement %r" % (what, key, got, want)
    integer = bool(on) and variant != 6 and ref["integer"]
    assert int(res["int_gram"][w]) == int(integer), "%s: start choice, margin %.3e" % (what, ref["margin"])
    if integer:
        assert np.array_equal(G, np.rint(G)) and np.abs(G).max() < 2.0 ** 53, what
        Gi = G.astype(np.int64)
        np.testing.assert_array_equal(Gi, ref["G"], err_msg=what)
        np.testing.assert_array_equal(Gi, Gi.T, err_msg=what)
        assert int(np.trace(Gi)) == int(res["sumsq"][w]), what
    elif ref["integer"]:
        exact = ref["c2"] * ref["G"].astype(np.longdouble)
        _within(G, exact, exact, P, what)
    else:
        assert ref["clipped"], what
        _within(G, ref["Gld"], ref["Gabs"].astype(np.longdouble), P, what)


def _check_case(ctx, combo, case, lmbda):
    res = _run(ctx, combo, case.x, lmbda)
    for w in range(case.x.shape[0]):
        _check_window(res, w, cases.window_ref((case.name, w), case.x[w], lmbda), combo, case.x.shape[2], case.name)
    return res


@pytest.mark.parametrize("shape", cases.SHAPES, ids=cases.shape_id)
@pytest.mark.parametrize("combo", COMBOS, ids=COMBO_IDS)
def test_start_at_every_shape(ctx, combo, shape):
    """Every content of the shape (zeros with one 1, all 255, alternating frames, random, a lone 255 at the window's or at every
    frame's last pixel, zero-padded frame tails), in batches whose windows start at every byte offset, at both lmbda."""
    for case in cases.shape_cases(shape):
        for lmbda in (LMBDA, LMBDA_ALL):
            _check_case(ctx, combo, case, lmbda)


@pytest.mark.parametrize("variant", [1, 2, 4, 5, 6])
def test_block_counts_on_both_sides_of_the_slab_sum(ctx, variant):
    """The shapes reach windows of 1..4 Gram slabs (summed by the small-matrix step itself) and of more (k_gram_reduce first); under
    the MFMA variants every count from 1 to 4."""
    seen = set()
    for shape in cases.SHAPES:
        seen.add(_run(ctx, (variant, 1), cases.shape_cases(shape)[3].x, LMBDA_ALL)["nblk"])
    assert min(seen) == 1 and any(1 < b <= 4 for b in seen) and max(seen) > 4, sorted(seen)
    if variant in (2, 4, 5):
        assert {1, 2, 3, 4} <= seen, sorted(seen)


@pytest.mark.parametrize("n,P", cases.NEIGHBOUR_SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("combo", COMBOS, ids=COMBO_IDS)
def test_window_does_not_see_its_neighbour(ctx, combo, n, P):
    """A random window next to an all-255 one, both orders: each window's result is that of the window run alone.  Statistics,
    start choice, scalars and the integer matrix are equal bit for bit; the f64 start pass sums a lone window's slabs in another
    order (the block count follows the batch), so there both runs are held to the same reference by the same bound."""
    for case in cases.neighbour_cases(n, P):
        for lmbda in (LMBDA, LMBDA_ALL):
            both = _check_case(ctx, combo, case, lmbda)
            for w in range(2):
                alone = _check_case(ctx, combo, cases.Case("%s_alone%d" % (case.name, w), case.x[w:w + 1]), lmbda)
                for key in ("sumsq", "maxv", "int_gram", "dual_norm", "mu_0", "thr_0", "dnorm"):
                    assert both[key][w] == alone[key][0], (case.name, w, key)
                if both["int_gram"][w]:
                    np.testing.assert_array_equal(both["G"][w], alone["G"][0])


@pytest.mark.parametrize("combo", COMBOS, ids=COMBO_IDS)
def test_start_choice_next_to_the_switch(ctx, combo):
    """Constant windows one size either side of 1.8 max(X) = 0.008 ||X||_F, and the same with the maximum raised apart from the
    norm: the choice is the restatement's (margins of 4e-6 .. 1.5e-4 against roundings of 1e-16), and both sides' matrices hold."""
    for case, (n, P, v, raised, integer) in zip(cases.boundary_cases(), cases.BOUNDARY):
        ref = cases.window_ref((case.name, 0), case.x[0])
        assert ref["integer"] == integer and abs(ref["margin"]) >= cases.MIN_MARGIN
        _check_case(ctx, combo, case, LMBDA)


@pytest.mark.parametrize("combo", COMBOS, ids=COMBO_IDS)
def test_clipped_windows_take_the_f64_start(ctx, combo):
    """The toy window of test_integer_start_matches_f64_start, a dark window with one saturated pixel, and a clipped window
    between two integer ones in one batch: int_gram = 0 where the first shrinkage clips, whatever the switch, and M_1^T M_1 of the
    start pass within the dot-product bound of the restatement's."""
    for case, clipped in cases.clipped_cases():
        res = _check_case(ctx, combo, case, LMBDA)
        for w, c in enumerate(clipped):
            assert cases.window_ref((case.name, w), case.x[w])["integer"] == (not c)
            if c:
                assert res["int_gram"][w] == 0
