"""CPU-only companion of tests/test_cnn_accuracy.py: the float32 yardsticks of tests/cnn_refs.py are what they claim to be, and the
checks that module applies to the HIP kernels reject a subtly wrong split-bf16 kernel (simulated here) while accepting a correct one."""
import numpy as np
import pytest
import torch

import cnn_refs as R


def _conv64(x, w, b):
    return torch.relu(torch.nn.functional.conv2d(torch.from_numpy(x).double(), torch.from_numpy(w).double(), torch.from_numpy(b).double())).numpy()


def test_sequential_float32_yardstick_is_float32_accurate():
    """The numpy loop against float64 on a small 3 x 3 case: a sequential float32 sum of K terms is within K / 2 ulps of the sum of
    magnitudes; measured far inside.  And the patch gather is the convolution's (same values as torch's float64 conv2d)."""
    g = torch.Generator().manual_seed(1)
    x, w, b = (t.numpy() for t in R.random_case(g, "normal", (3, 16, 9, 9), 24, 3))
    ni, yi, xi = R.sample_positions(np.random.default_rng(0), 3, 7, 7, 10 ** 9)
    a = R.gather_patches(x, ni, yi, xi, 3)
    ref = R.f64_product(a, w.reshape(24, -1), b)
    np.testing.assert_allclose(ref, _conv64(x, w, b)[ni, :, yi, xi], rtol=1e-13, atol=1e-13)
    mx, rms = R.err_stats(R.seq_f32_product(a, w.reshape(24, -1), b), ref)
    assert 0 < mx < 2e-6 and rms < 2e-7, (mx, rms)
    # stride 2, 7 x 7: conv1's geometry
    x7 = torch.randn((2, 3, 22, 22), generator=g).numpy()
    w7 = torch.randn((8, 3, 7, 7), generator=g).numpy()
    ref7 = torch.nn.functional.conv2d(torch.from_numpy(x7).double(), torch.from_numpy(w7).double(), stride=2).numpy()
    ni, yi, xi = R.sample_positions(np.random.default_rng(0), 2, 8, 8, 10 ** 9)
    got7 = R.gather_patches(x7, ni, yi, xi, 7, 2).astype(np.float64) @ w7.reshape(8, -1).astype(np.float64).T
    np.testing.assert_allclose(got7, ref7[ni, :, yi, xi], rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("t", [6, 7])
def test_winograd_float32_yardstick_is_float32_accurate(t):
    """The numpy float32 F(2x2, 3x3) against the float64 convolution, even and odd output sizes (the odd one has half-used tiles)."""
    g = torch.Generator().manual_seed(2)
    x, w, b = (v.numpy() for v in R.random_case(g, "relu3", (4, 16, t, t), 20, 3))
    o = t - 2
    ni, ty, tx = R.sample_wino(np.random.default_rng(0), 4, o, 10 ** 9)
    y = R.wino_f32_tiles(R.wino_tiles(x, ni, ty, tx), w, b)
    (ti, a, c), (pn, py, px) = R.wino_positions(ni, ty, tx, o)
    assert len(pn) == 4 * o * o
    ref = _conv64(x, w, b)[pn, :, py, px]
    mx, rms = R.err_stats(y[ti, :, a, c], ref)
    assert 0 < mx < 3e-6 and rms < 4e-7, (mx, rms)


@pytest.mark.parametrize("family", R.INT_FAMILIES)
@pytest.mark.parametrize("signed", [False, True])
def test_yardsticks_are_bit_exact_on_the_integer_families(family, signed):
    """Integer inputs under the 2**24 bound: the float32 yardsticks (direct and Winograd) equal float64 bit for bit."""
    rng = np.random.default_rng(3)
    x, w, b, bits, v = R.int_case(rng, family, signed, (3, 32, 8, 8), 40, 3, R.direct_bound)
    assert v < R.LIMIT and bits == R.start_bits(family)                 # these widths need no narrowing on a direct convolution
    ni, yi, xi = R.sample_positions(rng, 3, 6, 6, 10 ** 9)
    a = R.gather_patches(x, ni, yi, xi, 3)
    assert np.array_equal(R.seq_f32_product(a, w.reshape(40, -1), b).astype(np.float64), R.f64_product(a, w.reshape(40, -1), b))
    x, w, b, bits, v = R.int_case(rng, family, signed, (3, 32, 7, 7), 40, 3, R.wino_bound, wino=True)
    assert v < R.LIMIT
    if family == "wide_act":
        assert bits >= 16                  # B^T d B then spans 18 bits and a sign or more: two bf16 parts cannot carry it
    ni, ty, tx = R.sample_wino(rng, 3, 5, 10 ** 9)
    y = R.wino_f32_tiles(R.wino_tiles(x, ni, ty, tx), w, b)
    (ti, a, c), (pn, py, px) = R.wino_positions(ni, ty, tx, 5)
    assert np.array_equal(y[ti, :, a, c].astype(np.float64), _conv64(x, w, b)[pn, :, py, px])


def test_bf16_split_is_exact_and_round_to_nearest():
    rng = np.random.default_rng(4)
    a = (rng.standard_normal(4096) * np.exp(rng.uniform(-20, 20, 4096))).astype(np.float32)
    p = R.bf16_split(a, 3)
    assert np.array_equal(p[0].astype(np.float64) + p[1].astype(np.float64) + p[2].astype(np.float64), a.astype(np.float64))
    assert all(not (q.view(np.uint32) & 0xFFFF).any() for q in p)
    assert np.all(np.abs(a - p[0]) <= np.abs(p[0]) * 2.0 ** -8)
    assert R.bf16_round(np.array([1.0 + 2.0 ** -8], np.float32))[0] == 1.0          # a tie goes to the even neighbour
    assert R.bf16_round(np.array([1.0 + 3 * 2.0 ** -8], np.float32))[0] == np.float32(1.0 + 2.0 ** -6)


@pytest.mark.parametrize("K,cout", R.FIRE_SHAPES)
def test_criterion_rejects_wrong_split_kernels_on_random_inputs(K, cout):
    """Layer 2's criterion (max and rms within 3 x the sequential float32 evaluation's, against float64) on post-ReLU activations
    and He-scaled weights at every Fire reduction: a three-way split that drops the products i + j >= 2 and a two-way split fail it,
    the correct six-product kernel passes."""
    g = torch.Generator().manual_seed(K * 1000 + cout)
    P = max(64, -(-20000 // cout))
    a = (torch.relu(torch.randn((P, K), generator=g)) * 3.0).numpy()
    w = (torch.randn((cout, K), generator=g) * (2.0 / K) ** 0.5).numpy()
    b = (torch.randn((cout,), generator=g) * 0.3).numpy()
    ref = R.f64_product(a, w, b)
    yard = R.err_stats(R.seq_f32_product(a, w, b), ref)
    got = {name: R.err_stats(R.split_product(a, w, b, **kw), ref) for name, kw in R.SPLIT_VARIANTS.items()}
    assert R.within(got["correct"], yard), (got, yard)
    assert not R.within(got["dropped"], yard), (got, yard)
    assert not R.within(got["two_way"], yard), (got, yard)
    assert got["dropped"][1] > 5 * yard[1] and got["two_way"][1] > 5 * yard[1], (got, yard)          # rms decides, with room


@pytest.mark.parametrize("K,cout", [(64, 256), (512, 64), (576, 256)])
def test_integer_families_expose_wrong_split_kernels(K, cout):
    """Layer 1's families through the simulated kernels: the correct split reproduces all three exactly; neither wrong split reproduces
    "wide activations"; the one that drops products does not reproduce "wide both"."""
    rng = np.random.default_rng(K + cout)
    P = 400
    for family in R.INT_FAMILIES:
        for signed in (False, True):
            w = R.int_weights(rng, family, cout, K, 1).reshape(cout, K)
            a = R.int_activations(rng, family, (P, K), None, signed)
            b = rng.integers(-100, 101, size=(cout,)).astype(np.float32)
            assert float((np.abs(a).astype(np.float64) @ np.abs(w).astype(np.float64).T).max()) + 100 < R.LIMIT
            ref = R.f64_product(a, w, b)
            same = {name: np.array_equal(R.split_product(a, w, b, **kw).astype(np.float64), ref) for name, kw in R.SPLIT_VARIANTS.items()}
            assert same["correct"], (family, signed)
            if family == "wide_act":
                assert not same["dropped"] and not same["two_way"], (family, signed, same)
            if family == "wide_both":
                assert not same["dropped"], (family, signed, same)


@pytest.mark.parametrize("cin,cout", [(32, 128), (64, 256)])
def test_winograd_integer_families_expose_wrong_split_kernels(cin, cout):
    """The same for F(2x2, 3x3), where the bound narrows the activations and the wide families sit on the centre tap: the simulated
    split-bf16 Winograd kernel (V = B^T d B and U = G g G^T split, sixteen per-position products) reproduces all three families
    exactly when correct; neither wrong split reproduces "wide activations" (V still needs three parts), and the one that drops
    products does not reproduce "wide both" (V and U need two parts each: the product (1, 1) is missing)."""
    rng = np.random.default_rng(cin + cout)
    n, t = 5, 7
    for family in R.INT_FAMILIES:
        for signed in (False, True):
            x, w, b, bits, v = R.int_case(rng, family, signed, (n, cin, t, t), cout, 3, R.wino_bound, wino=True)
            assert v < R.LIMIT
            ni, ty, tx = R.sample_wino(rng, n, t - 2, 10 ** 9)
            (ti, a, c), (pn, py, px) = R.wino_positions(ni, ty, tx, t - 2)
            ref = _conv64(x, w, b)[pn, :, py, px]
            d = R.wino_tiles(x, ni, ty, tx)
            same = {name: np.array_equal(R.split_wino_tiles(d, w, b, **kw)[ti, :, a, c].astype(np.float64), ref)
                    for name, kw in R.SPLIT_VARIANTS.items()}
            assert same["correct"], (family, signed, bits)
            if family == "wide_act":
                assert not same["dropped"] and not same["two_way"], (family, signed, bits, same)
            if family == "wide_both":
                assert not same["dropped"], (family, signed, bits, same)
