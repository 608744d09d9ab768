"""The designed crops of tests/resize_taps.py test what they are named for, shown without a GPU: they are Pillow's resize, every changed
restatement (a tap lost, no rounding term, coefficients reversed, channels swapped) differs on them at every size, and a lost outermost
tap differs at the byte designed for it."""
import time

import numpy as np
import pytest

import pil_resize_ref as P
import resize_taps as T


@pytest.fixture(scope="module")
def designs():
    """Every design, built once; the build time is printed (pytest -s)."""
    t = time.time()
    small = [T.design(s) for s in T.SMALL_SIZES]
    t_small = time.time() - t
    t = time.time()
    large = [T.design(s) for s in T.LARGE_SIZES]
    print("designed signals: %.1f s for the %d sizes 1..512, %.1f s for the %d large-route sizes"
          % (t_small, len(small), time.time() - t, len(large)))
    return small, large


def _crops(d):
    return (("horizontal", d.horizontal()), ("vertical", d.vertical()))


def test_sizes_are_the_ones_named():
    assert T.SMALL_SIZES == list(range(1, 24)) + list(range(25, 513))
    grow = [s for s in range(513, 4097) if (s - 1) % 24 == 0]
    assert len(grow) == 149 and T.LARGE_SIZES == sorted(grow + [s - 1 for s in grow] + [4096])
    for s in T.LARGE_SIZES:          # the device's bound on the coefficients per sample, 2 ceil(s / 24) + 1, grows at `grow` and holds
        bound = 2 * -(-s // 24) + 1
        assert max(len(k) for k in T.coeffs(s)[1]) <= bound <= P.MAX_K
        assert (bound > 2 * -(-(s - 1) // 24) + 1) == (s in grow)


def test_unchanged_copy_is_the_restatement():
    for shape in [(1, 1), (24, 24), (24, 31), (40, 24), (3, 500), (37, 61), (512, 300), (24, 1296), (600, 513), (30, 4096)]:
        image = P.formula_image(*shape, offset=17)
        np.testing.assert_array_equal(T.resize(image), P.patch(image), err_msg=str(shape))


def test_every_nonzero_target_has_a_signal_and_few_targets_are_moved(designs):
    small, large = designs
    missing = [m for d in small + large for m in d.missing]
    assert not missing, "no signal for (size, output sample, 0 = first / 1 = last): %r" % missing
    share_small, share_large = T.moved_share(T.SMALL_SIZES), T.moved_share(T.LARGE_SIZES)
    print("targets moved inwards by a zero coefficient: %.4f of sizes 1..512, %.4f of the large-route sizes" % (share_small, share_large))
    assert share_small <= 0.05 and share_large <= 0.30
    for d in small + large:          # a target is a non-zero coefficient with only zeros outside it; the signal holds 255 there
        for xx, k in enumerate(d.ks):
            first, last = d.target[xx]
            assert k[first] > 0 and k[last] > 0 and not k[:first].any() and not k[last + 1:].any()
            assert d.signals[xx][0][first] == 255 and d.signals[xx][1][last] in (255, 254)
            assert d.signals[xx][0].dtype == np.uint8 and len(d.signals[xx][0]) == len(k) == d.bounds[xx][1]


def test_signals_flip_the_byte_and_stay_below_the_clip(designs):
    """The accumulators themselves, in Python integers: without the target tap the byte is lower, with it at most 255."""
    small, large = designs
    for d in small + large:
        for xx, k in enumerate(d.ks):
            for e in (0, 1):
                t = int(d.target[xx, e])
                full = T.HALF + sum(int(a) * int(v) for a, v in zip(k, d.signals[xx][e]))
                without = full - int(d.signals[xx][e][t]) * int(k[t])
                assert (without >> 22) < (full >> 22) <= 255, (d.size, xx, e)


@pytest.mark.parametrize("which", ["small", "large"])
def test_designed_crops_are_pillows_resize(designs, which):
    """One pass runs on these shapes, so the installed Pillow's pass order cannot matter."""
    from PIL import Image
    bil = getattr(Image, "Resampling", Image).BILINEAR
    for d in designs[0 if which == "small" else 1]:
        for axis, crop in _crops(d):
            assert crop.shape == ((24, d.size, 3) if axis == "horizontal" else (d.size, 24, 3))
            exp = np.asarray(Image.fromarray(crop).resize((24, 24), bil))
            np.testing.assert_array_equal(P.patch(crop), exp, err_msg="%s crop of size %d" % (axis, d.size))
    d = designs[0][100]          # outside a row's taps and in channel 2 the crop is the formula image
    crop, formula = d.horizontal(), P.formula_image(24, d.size, offset=d.size % 256)
    assert np.array_equal(crop[:, :, 2], formula[:, :, 2])
    for r in range(24):
        xmin, xmax = d.bounds[r]
        outside = np.ones(d.size, bool)
        outside[xmin:xmin + xmax] = False
        assert np.array_equal(crop[r, outside], formula[r, outside])


def test_combined_crops_lose_a_byte_with_either_pass_cut_short():
    """Both passes run: compared with the restatement only (tall shapes must not be compared with the installed Pillow, see
    pil_resize_ref.py).  No shape had to be dropped: every one has an offset."""
    for shape in T.COMBINED_SMALL + T.COMBINED_LARGE:
        image, offset = T.combined(shape)
        assert image is not None, "no offset in 0..255 for %r" % (shape,)
        assert image.shape == shape + (3,) and np.array_equal(image, P.formula_image(*shape, offset=offset))
        true = P.patch(image)
        np.testing.assert_array_equal(T.resize(image), true)
        for change in (dict(drop_x="last"), dict(drop_y="last"), dict(drop_x="first"), dict(drop_y="first"), dict(rounding=0)):
            assert not np.array_equal(T.resize(image, **change), true), (shape, change)


def _undetectable(d, name):
    """Sizes at which no content at all can show a change: every output sample is one input sample times 2^22 (nothing to round),
    every sample's coefficients read the same in both directions (nothing to reverse)."""
    if name == "no_rounding_term":
        return all((k % T.ONE == 0).all() for k in d.ks)
    if name == "coefficients_reversed":
        return all(np.array_equal(k, k[::-1]) for k in d.ks)
    return False


@pytest.mark.parametrize("which", ["small", "large"])
def test_every_changed_restatement_differs_on_every_designed_crop(designs, which):
    exempt = {}
    for d in designs[0 if which == "small" else 1]:
        diag = np.arange(24)
        for a, (axis, crop) in enumerate(_crops(d)):
            true = T.resize(crop)
            where = "%s crop of size %d" % (axis, d.size)
            for name, kwargs in T.MUTANTS.items():
                got = T.resize(crop, **kwargs[a])
                if _undetectable(d, name):
                    exempt.setdefault(name, set()).add(d.size)
                    continue
                assert not np.array_equal(got, true), "%s: %s passes" % (where, name)
                if name in ("first_tap_dropped", "last_tap_dropped"):          # ... at the designed byte of every target it drops
                    e = 0 if name == "first_tap_dropped" else 1
                    hit = got[diag, diag, e] != true[diag, diag, e]
                    assert hit[~d.moved[:, e]].all(), "%s: %s, output samples %r" % (where, name, np.flatnonzero(~hit & ~d.moved[:, e]))
            for e in (0, 1):          # the target tap itself, moved inwards or not, decides its byte
                got = T.resize(crop, **{("drop_x", "drop_y")[a]: d.target[:, e]})
                assert (got[diag, diag, e] != true[diag, diag, e]).all(), "%s: target %d" % (where, e)
    for d in designs[0 if which == "small" else 1]:          # a last-tap signal peaks at 254 exactly where one tap is both targets
        for xx in range(24):
            one_tap = d.target[xx, 0] == d.target[xx, 1]
            assert d.signals[xx][1][d.target[xx, 1]] == (254 if one_tap else 255) and (not one_tap or d.size < 24)
    # size 1 is one sample with coefficient 2^22; nothing else is exempt
    assert exempt == ({"no_rounding_term": {1}, "coefficients_reversed": {1}} if which == "small" else {}), exempt


def test_float32_statement_of_the_network_input_is_the_oracles():
    """(float32(byte) / float32(255) - mean) / std, each operation rounded to float32, against oracle.classifier_ref.transform (a
    24 x 24 image passes through its resize), bit for bit."""
    from oracle import classifier_ref as ref
    ramp = (np.arange(24 * 24 * 3) % 256).astype(np.uint8).reshape(24, 24, 3)
    patches = [ramp, 255 - ramp, P.patch(T.design(511).horizontal()), P.patch(T.design(37).vertical()), P.patch(T.combined((47, 48))[0])]
    for p in patches:
        exp = ref.transform(p)[0].numpy()
        got = T.net_input(p, ref.MEAN, ref.STD, 100)
        assert got.dtype == exp.dtype == np.float32 and np.array_equal(got.view(np.int32), exp.view(np.int32))
    lut = T.net_lut(ref.MEAN, ref.STD)
    assert lut.shape == (3, 256) and len(np.unique(np.stack(patches))) == 256          # every byte value was compared
    inner = T.net_interior(np.stack(patches), ref.MEAN, ref.STD)
    np.testing.assert_array_equal(inner[0], T.net_input(patches[0], ref.MEAN, ref.STD, 0))
