"""The host derivation of the shape properties (image_filtering.ShapeMeasures, ShapeRegionProps, data_structures.Segment) on hand-made
records -- no GPU: closed forms on rectangles, a pixel, a ring, diagonal lines; translation invariance bit for bit; agreement with
the independent derivation of tests/shape_props_ref.py; the names that are not provided.

Exact checks compare the unrounded rationals (ShapeMeasures.exact_central), before the single rounding.

Orientation of a rectangle: the specified rule is, with a, b, b, c = inertia_tensor.flat = (mu02, -mu11, -mu11, mu20) / mu00,
0.5 atan2(-2 b, c - a).  For a rectangle wider than high a > c and b = 0, which gives +-pi / 2, and one higher than wide gives 0:
the angle is measured from the row axis.  That is what is asserted below (the closed form of the rule itself)."""
import copy
import math
from fractions import Fraction

import numpy as np
import pytest

import shape_props_ref as ref
from swiftwatcher_amd import image_filtering as img
from swiftwatcher_amd.data_structures import Segment

RTOL = 1e-12          # < 20 correctly rounded operations on bit-identical inputs at a conditioning below 1e2 (l1 / l2 >= 1.2)


def measures(mask, origin=(0, 0)):
    return img.ShapeMeasures(*ref.measures_input(mask, origin))


def rect(h, w):
    return np.ones((h, w), bool)


RECTS = [(3, 3), (3, 7), (7, 3), (4, 9), (10, 4), (5, 5), (12, 31), (40, 6)]


@pytest.mark.parametrize("h,w", RECTS)
def test_rectangle_closed_forms(h, w):
    m = measures(rect(h, w), (11, 5))
    area = h * w
    mu = m.exact_central
    assert mu[(2, 0)] == Fraction(area * (h * h - 1), 12)
    assert mu[(0, 2)] == Fraction(area * (w * w - 1), 12)
    assert mu[(1, 1)] == 0
    assert mu[(0, 0)] == area and mu[(1, 0)] == 0 and mu[(0, 1)] == 0
    assert m.moments_central[2, 0] == area * (h * h - 1) / 12 and m.moments_central[0, 2] == area * (w * w - 1) / 12
    assert m.major_axis_length == pytest.approx(4 * math.sqrt((max(h, w) ** 2 - 1) / 12), rel=RTOL)
    assert m.minor_axis_length == pytest.approx(4 * math.sqrt((min(h, w) ** 2 - 1) / 12), rel=RTOL)
    if h == w:
        assert m.eccentricity == 0.0
        assert m.orientation == math.pi / 4
    elif w > h:
        assert abs(m.orientation) == math.pi / 2
    else:
        assert m.orientation == 0.0
    assert m.extent == 1.0 and m.bbox_area == area
    assert m.euler_number == 1
    # border: the outline; four corners of weight (1 + sqrt 2) / 2 ... as the helper classifies them
    border, perim = ref.border_and_classes(rect(h, w))
    assert border == 2 * (h - 2) + 2 * (w - 2) + 4
    assert m.perimeter == perim[0] + perim[1] * math.sqrt(2) + perim[2] * ((1 + math.sqrt(2)) / 2)
    assert perim[0] + perim[1] + perim[2] <= border
    assert m.equivalent_diameter == math.sqrt(4 * area / math.pi)


def test_single_pixel():
    m = measures(np.ones((1, 1), bool), (7, 9))
    for name in img.SHAPE_PROPERTIES:
        v = np.asarray(getattr(m, name), dtype=np.float64)
        if name in ("moments", "moments_central", "moments_normalized"):
            p, q = np.indices((4, 4))
            low = 2 if name == "moments_normalized" else 0
            keep = (p + q <= 3) & (p + q >= low)
            assert np.all(np.isfinite(v[keep])) and np.all(np.isnan(v[~keep]))
        else:
            assert np.all(np.isfinite(v)), name
    assert m.perimeter == 0.0 and m.major_axis_length == 0.0 and m.minor_axis_length == 0.0 and m.eccentricity == 0.0
    assert m.euler_number == 1 and m.extent == 1.0 and m.local_centroid == (0.0, 0.0)
    assert m.moments[0, 0] == 1.0 and m.moments[1, 0] == 0.0


def ring(n=9, t=2):
    m = np.ones((n, n), bool)
    m[t:-t, t:-t] = False
    return m


def test_ring_has_euler_number_zero():
    m = measures(ring())
    assert m.euler_number == 0 == ref.euler_by_labelling(ring())
    assert m.eccentricity == 0.0 and m.orientation == math.pi / 4


def test_two_diagonal_holes_are_two_holes():
    """The documented deviation: two holes that touch diagonally are two holes of the 8-connected Euler number (1 - 2 = -1); counted
    with an 8-neighbourhood, as skimage 0.15 does, they are one (1 - 1 = 0)."""
    mask = np.ones((6, 6), bool)
    mask[2, 2] = mask[3, 3] = False
    m = measures(mask)
    assert m.euler_number == -1 == ref.euler_by_labelling(mask)
    assert 1 - ref.holes_8(mask) == 0


@pytest.mark.parametrize("k", [3, 4, 9, 30])
@pytest.mark.parametrize("anti", [False, True])
def test_diagonal_line(k, anti):
    mask = np.eye(k, dtype=bool)
    if anti:
        mask = mask[:, ::-1]
    bbox, rec = ref.measures_input(mask, (4, 2))
    assert rec[2][1] == k - 2 and rec[1] == k          # perim[1], border
    m = img.ShapeMeasures(bbox, rec)
    # a == c; b = -mu11 / mu00 is negative on the main diagonal (mu11 > 0)
    assert m.orientation == (math.pi / 4 if anti else -math.pi / 4)
    assert m.minor_axis_length == 0.0 and m.eccentricity == 1.0
    assert m.perimeter == pytest.approx((k - 2) * math.sqrt(2), rel=RTOL)
    assert m.euler_number == 1


def ellipse(H, W, cy, cx, a, b, theta):
    yy, xx = np.mgrid[0:H, 0:W]
    u = (xx - cx) * math.cos(theta) + (yy - cy) * math.sin(theta)
    v = -(xx - cx) * math.sin(theta) + (yy - cy) * math.cos(theta)
    return (u / a) ** 2 + (v / b) ** 2 <= 1.0


def families():
    out = {}
    for i, theta in enumerate((0.0, 0.3, 0.8, 1.2, 1.57, 2.1, 2.9)):
        out["ellipse_%d" % i] = ellipse(40, 48, 19.3, 23.7, 14.0, 5.5, theta)
    out["ellipse_fat"] = ellipse(30, 30, 14.2, 15.1, 11.0, 9.0, 0.4)
    L = np.zeros((12, 9), bool)
    L[:, :3] = True
    L[9:, :] = True
    out["L"] = L
    out["L_flipped"] = L[::-1, ::-1].copy()
    T = np.zeros((9, 15), bool)
    T[:2, :] = True
    T[:, 6:8] = True
    out["T"] = T
    rng = np.random.default_rng(5)
    blob = ellipse(33, 41, 16, 20, 15, 8, 0.6) & (rng.random((33, 41)) > 0.2)
    out["ragged"] = blob
    out["with_hole"] = ellipse(31, 45, 15, 22, 20, 9, 2.5) & ~ellipse(31, 45, 15, 22, 6, 3, 2.5)
    out["rect_3x17"] = rect(3, 17)
    out["rect_21x4"] = rect(21, 4)
    return out


FAMILIES = families()


@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_agrees_with_the_independent_derivation(name):
    mask = FAMILIES[name]
    want = ref.derive(mask)
    m = measures(mask, (100, 3000))
    assert m.exact_central == want["central_exact"]
    cen = m.moments_central
    assert np.array_equal(cen, want["moments_central"], equal_nan=True)          # bit for bit: one exact rational rounded once
    assert np.array_equal(m.inertia_tensor, want["inertia_tensor"])
    l1, l2 = want["eigvals"]
    assert l2 > 0 and l1 / l2 >= 1.2, "the case must keep sqrt(1 - l2 / l1) and atan2 well conditioned"
    assert m.inertia_tensor_eigvals == pytest.approx(want["eigvals"], rel=RTOL)
    for key in ("major_axis_length", "minor_axis_length", "eccentricity", "orientation", "perimeter", "extent", "equivalent_diameter"):
        assert getattr(m, key) == pytest.approx(want[key], rel=RTOL), key
    assert m.euler_number == want["euler_number"] == ref.euler_by_labelling(mask)
    assert np.allclose(m.moments_hu, want["moments_hu"], rtol=1e-9, atol=1e-18)
    # bbox-local raw moments against the coordinates themselves
    rr, cc = np.nonzero(mask)
    r, c = (rr - rr.min()).astype(object), (cc - cc.min()).astype(object)
    for p in range(4):
        for q in range(4):
            if p + q <= 3:
                assert m.moments[p, q] == float(int((r ** p * c ** q).sum()))
            else:
                assert math.isnan(m.moments[p, q])
    assert m.local_centroid == (float(Fraction(int(r.sum()), len(r))), float(Fraction(int(c.sum()), len(c))))


@pytest.mark.parametrize("name", ["ellipse_1", "ragged", "L"])
def test_translation_changes_no_bit(name):
    mask = FAMILIES[name]
    base = measures(mask, (0, 0))
    for origin in ((0, 1), (1, 0), (17, 4000), (4000, 4000 - mask.shape[1]), (32768 - mask.shape[0], 32768 - mask.shape[1])):
        m = measures(mask, origin)
        for key in ("moments", "moments_central", "moments_hu", "moments_normalized"):
            assert np.array_equal(getattr(m, key), getattr(base, key), equal_nan=True), (key, origin)
        assert m.exact_central == base.exact_central
        assert m.orientation == base.orientation and m.eccentricity == base.eccentricity


def test_names_that_are_not_provided_raise_and_name_the_list():
    m = measures(rect(3, 4))
    props = img.ShapeRegionProps(1, m.bbox, (1.0, 1.5), 12, m)
    seg = Segment(img.RegionProps(1, m.bbox, (1.0, 1.5), 12), 3, "00:00:00.100", None)
    seg._shape = ref.measures_input(rect(3, 4))[1]
    for obj in (m, props, seg):
        for name in img.SHAPE_NOT_PROVIDED:
            with pytest.raises(AttributeError) as exc:
                getattr(obj, name)
            assert name in str(exc.value) and "solidity" in str(exc.value) and "coords" in str(exc.value)
        with pytest.raises(AttributeError):
            obj.no_such_thing
    assert {"convex_area", "convex_image", "solidity", "filled_area", "filled_image", "image", "coords"} <= set(img.SHAPE_NOT_PROVIDED)
    assert props.orientation == m.orientation and props.label == 1 and props.area == 12
    assert seg.orientation == m.orientation and seg.euler_number == 1


def test_plain_regionprops_and_segments_are_unchanged():
    plain = img.RegionProps(2, (0, 0, 3, 4), (1.0, 1.5), 12)
    assert img.RegionProps.__slots__ == ("label", "bbox", "centroid", "area")
    assert not hasattr(plain, "orientation") and not hasattr(plain, "shape")
    seg = Segment(plain, 3, "00:00:00.100", None)
    assert sorted(seg.__dict__) == ["_image", "area", "bbox", "centroid", "label", "parent_frame_number", "parent_timestamp",
                                    "segment_history", "status"]
    with pytest.raises(AttributeError) as exc:
        seg.eccentricity
    assert "shape_props" in str(exc.value)


def test_deepcopy_keeps_the_record():
    mask = FAMILIES["ellipse_2"]
    bbox, rec = ref.measures_input(mask)
    seg = Segment(img.RegionProps(1, bbox, (0.0, 0.0), int(mask.sum())), 3, "00:00:00.100", None)
    seg._shape = rec
    first = seg.orientation
    twin = copy.deepcopy([[seg]])[0][0]
    assert twin._shape == rec and twin.orientation == first and twin.perimeter == seg.perimeter
    fresh = copy.deepcopy(Segment(img.RegionProps(1, bbox, (0.0, 0.0), int(mask.sum())), 3, "00:00:00.100", None))
    assert "_shape" not in fresh.__dict__


def test_shape_records_gives_plain_integers():
    from swiftwatcher_amd import _lib
    recs = np.zeros(2, _lib.SHAPE_DTYPE)
    recs["m"][1] = np.arange(10) * (1 << 40)
    recs["quads"][1] = (4, 0, 0)
    out = img.shape_records(recs)
    assert out[1][0] == tuple(k << 40 for k in range(10)) and out[1][3] == (4, 0, 0)
    assert all(type(x) is int for x in out[1][0])
