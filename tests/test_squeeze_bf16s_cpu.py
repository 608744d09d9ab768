"""CPU-only companion of tests/test_squeeze_bf16s_gpu.py: the two criteria that file applies to k_squeeze1x1_bf16s (exact integers,
3 x the sequential float32 evaluation on random inputs; tests/cnn_refs.py) accept a simulated intact kernel -- six products per
k-step in the kernel's own reduction order -- and reject one that drops the products i + j >= 2, at K = 384 and at K = 256, on the
very inputs the GPU test launches (tests/squeeze_bf16s_cases.py, whose SEED was chosen here)."""
import numpy as np
import pytest

import cnn_refs as R
import squeeze_bf16s_cases as S


def _simulated(case, family, variant):
    n = 3 if family == "zero_segment" and case[2] < 3 else case[2]
    case = S.with_segments(case, n)
    x, w, b = S.random_inputs(case, family)
    a, w2 = S.rows_of(x, case), w.reshape(case[1], case[0])
    order = S.kernel_k_order(case[0])
    ref = R.f64_product(a, w2, b)
    yard = R.err_stats(R.seq_f32_product(a, w2, b), ref)
    got = R.err_stats(R.split_product(np.ascontiguousarray(a[:, order]), np.ascontiguousarray(w2[:, order]), b, **R.SPLIT_VARIANTS[variant]), ref)
    return got, yard


def test_kernel_order_is_a_permutation():
    for cin in (256, 384):
        assert sorted(S.kernel_k_order(cin)) == list(range(cin))


@pytest.mark.parametrize("case", S.CASES, ids=S.IDS)
def test_criterion_accepts_the_intact_simulation_on_the_gpu_inputs(case):
    for family in R.FAMILIES:
        got, yard = _simulated(case, family, "correct")
        assert R.within(got, yard), (family, got, yard, R.ratios(got, yard))


@pytest.mark.parametrize("case", S.CASES[:3], ids=S.IDS[:3])
def test_criterion_rejects_dropped_products_on_the_gpu_inputs(case):
    """Post-ReLU activations (no cancellation) are where the lost 2**-16 terms show: rms by more than 5 x the yardstick's."""
    got, yard = _simulated(case, "relu3", "dropped")
    assert not R.within(got, yard), (got, yard)
    assert got[1] > 5 * yard[1], (got, yard)


@pytest.mark.parametrize("cin,cout", S.SHAPES)
def test_integer_families_reject_dropped_products(cin, cout):
    """Layer 1 at the squeeze reductions, 50 rows as the GPU cases: the intact simulation reproduces float64 bit for bit on all three
    families, the doctored one neither "wide activations" nor "wide both"."""
    rng = np.random.default_rng(cin + cout)
    order = S.kernel_k_order(cin)
    for family in R.INT_FAMILIES:
        for signed in (False, True):
            w = R.int_weights(rng, family, cout, cin, 1).reshape(cout, cin)
            a = R.int_activations(rng, family, (50, cin), None, signed)
            b = rng.integers(-100, 101, size=(cout,)).astype(np.float32)
            assert float((np.abs(a).astype(np.float64) @ np.abs(w).astype(np.float64).T).max()) + 100 < R.LIMIT
            ref = R.f64_product(a, w, b)
            same = {name: np.array_equal(R.split_product(np.ascontiguousarray(a[:, order]), np.ascontiguousarray(w[:, order]), b,
                                                         **R.SPLIT_VARIANTS[name]).astype(np.float64), ref) for name in ("correct", "dropped")}
            assert same["correct"], (family, signed)
            if family != "narrow":
                assert not same["dropped"], (family, signed)
