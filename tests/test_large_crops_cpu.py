"""The yardstick of the large-crop route (segment boxes with a side of 513..4096): tests/pil_resize_ref.py, Pillow's antialiased
bilinear resize restated with the horizontal pass first, against Pillow itself.  Tall shapes are compared with the fixture written by a
Pillow 8 (tools/make_pil_resize_goldens.py): newer Pillows run the vertical pass first on some of them.  Shapes of at most 1400 rows
are compared with the installed Pillow as well, and with the product's host statement of the same transform, resize_segment."""
import os

import numpy as np
import pytest

import pil_resize_ref as P

# rows x columns, every one of at most 1400 rows: the installed Pillow runs these horizontal pass first
LIVE_SHAPES = [(513, 24), (24, 513), (512, 513), (3, 1299), (700, 1300), (600, 700), (528, 528), (24, 1296)]
# shapes the fixture must hold: where the installed Pillow may differ (8000 x 30 is beyond the device route's 4096 and serves this
# file only), a wide one, a 4K frame, and the smallest boxes of the route
FIXTURE_MUST_HOLD = [(4096, 25), (3000, 25), (4096, 40), (8000, 30), (30, 4096), (2160, 3840), (513, 24), (24, 513)]


@pytest.fixture(scope="module")
def fixture(golden_dir):
    g = np.load(os.path.join(golden_dir, "pil_resize_large.npz"))
    return [tuple(int(v) for v in s) for s in g["shapes"]], g["patches"]


def test_fixture_holds_the_shapes_the_route_is_defined_on(fixture):
    shapes, patches = fixture
    assert set(FIXTURE_MUST_HOLD) <= set(shapes)
    assert patches.shape == (len(shapes), 24, 24, 3) and patches.dtype == np.uint8


def test_restatement_equals_every_patch_of_the_fixture(fixture):
    shapes, patches = fixture
    for (h, w), exp in zip(shapes, patches):
        np.testing.assert_array_equal(P.patch(P.formula_image(h, w)), exp, err_msg="%d x %d" % (h, w))


@pytest.mark.parametrize("shape", LIVE_SHAPES, ids=lambda s: "%dx%d" % s)
def test_restatement_equals_installed_pillow_and_resize_segment(shape):
    from PIL import Image
    from swiftwatcher_amd.segment_classification import resize_segment
    image = P.formula_image(*shape, offset=shape[0] % 7)
    got = P.patch(image)
    bil = getattr(Image, "Resampling", Image).BILINEAR
    np.testing.assert_array_equal(got, np.asarray(Image.fromarray(image).resize((24, 24), bil)))
    np.testing.assert_array_equal(got, resize_segment(image))


def test_coefficient_tables_are_normalised_and_fit_the_device_layout():
    """What the int32 accumulators and the 343-entry rows of the device tables rely on, at every input size of the route."""
    for size in list(range(1, 60)) + [511, 512, 513, 1023, 1024, 1025, 2160, 3840, 4095, 4096]:
        bounds, table = P.coeff_table(size)
        assert bounds[:, 1].max() <= P.MAX_K and (bounds[:, 0] >= 0).all() and (bounds[:, 0] + bounds[:, 1] <= size).all()
        sums = table.sum(axis=1)
        assert (np.abs(sums - (1 << 22)) <= P.MAX_K).all()          # each coefficient is rounded: the sum is 2^22 within one per tap
        assert (table >= 0).all() and 255 * int(sums.max()) + (1 << 21) < 2 ** 31
