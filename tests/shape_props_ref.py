"""Reference for swk_segment_shapes_u8 and for the host derivation of the shape properties (image_filtering.ShapeMeasures), with
numpy, scipy.ndimage and the standard library alone.

records(plane): per non-zero value of a u8 label plane, ascending, the record the kernel must give -- the ten power sums from
coordinate arrays in Python-int (object) precision; border pixels and perimeter classes the way skimage.measure.perimeter(image, 4)
of scikit-image 0.15.0 finds them, on that value's own mask (binary_erosion with the 4-connected cross and border_value=0, then
ndimage.convolve of the border image with [[10, 2, 10], [2, 1, 2], [10, 2, 10]], mode="constant"); bit quads from a zero-padded 2x2
sliding count.

derive(mask): the derived properties of one region, independently of ShapeMeasures: central moments from fractions.Fraction
coordinates minus the Fraction centroid, rounded once; eigenvalues and angles from those in 50-digit decimal arithmetic."""
import math
from decimal import Decimal, getcontext
from fractions import Fraction

import numpy as np
from scipy import ndimage

ORDER = ((0, 0), (1, 0), (0, 1), (2, 0), (1, 1), (0, 2), (3, 0), (2, 1), (1, 2), (0, 3))
CROSS = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], bool)
WEIGHTS = np.array([[10, 2, 10], [2, 1, 2], [10, 2, 10]])
CLASS_CODES = ((5, 7, 15, 17, 25, 27), (21, 33), (13, 23))


def power_sums(mask, origin=(0, 0)):
    rr, cc = np.nonzero(mask)
    r = (rr + origin[0]).astype(object)
    c = (cc + origin[1]).astype(object)
    return [int((r ** p * c ** q).sum()) if len(r) else 0 for p, q in ORDER]


def border_and_classes(mask):
    mask = mask.astype(bool)
    border = mask & ~ndimage.binary_erosion(mask, CROSS, border_value=0)
    codes = ndimage.convolve(border.astype(np.int64), WEIGHTS, mode="constant", cval=0)
    hist = np.bincount(codes.ravel(), minlength=50)
    # (only border pixels have an odd code, and every class code is odd)
    return int(border.sum()), [int(sum(hist[k] for k in ks)) for ks in CLASS_CODES]


def quads(mask):
    p = np.pad(mask.astype(np.int64), 1)
    a, b, c, d = p[:-1, :-1], p[:-1, 1:], p[1:, :-1], p[1:, 1:]
    n = a + b + c + d
    diag = (n == 2) & (a == d)          # two set, and the two on one diagonal are equal: both set or both clear
    return [int((n == 1).sum()), int((n == 3).sum()), int(diag.sum())]


def record(plane, v):
    """(the value's mask is cut to its bounding box first: outside it everything is zero, which is what border_value=0, cval=0 and
    the zero padding of the quads stand for)"""
    mask = plane == v
    rr, cc = np.nonzero(mask)
    r0, c0 = int(rr.min()), int(cc.min())
    mask = mask[r0:int(rr.max()) + 1, c0:int(cc.max()) + 1]
    border, perim = border_and_classes(mask)
    return {"label": int(v), "m": power_sums(mask, (r0, c0)), "border": border, "perim": perim, "quads": quads(mask)}


def records(plane):
    """ascending-value records of a u8 plane (labels above 255 have aliased before they got here)"""
    return [record(plane, v) for v in np.unique(plane) if v]


def as_dicts(recs):
    """SHAPE_DTYPE records -> the dicts of records()"""
    return [{"label": int(r["label"]), "m": [int(x) for x in r["m"]], "border": int(r["border"]), "perim": [int(x) for x in r["perim"]],
             "quads": [int(x) for x in r["quads"]]} for r in recs]


def measures_input(mask, origin=(0, 0)):
    """(bbox, record tuple) of one region for image_filtering.ShapeMeasures, the region placed at `origin` of a plane"""
    rr, cc = np.nonzero(mask)
    bbox = (int(rr.min()) + origin[0], int(cc.min()) + origin[1], int(rr.max()) + 1 + origin[0], int(cc.max()) + 1 + origin[1])
    border, perim = border_and_classes(mask)
    return bbox, (tuple(power_sums(mask, origin)), border, tuple(perim), tuple(quads(mask)))


def central_exact(mask):
    """{(p, q): Fraction} for p + q <= 3, from the coordinates minus the Fraction centroid"""
    rr, cc = np.nonzero(mask)
    r = [Fraction(int(x)) for x in rr]
    c = [Fraction(int(x)) for x in cc]
    n = len(r)
    rb, cb = sum(r) / n, sum(c) / n
    return {(p, q): sum((a - rb) ** p * (b - cb) ** q for a, b in zip(r, c)) for p in range(4) for q in range(4 - p)}


def _dec(x):
    return Decimal(x.numerator) / Decimal(x.denominator)


def derive(mask):
    getcontext().prec = 60
    mu = central_exact(mask)
    out = {"central_exact": mu}
    cen = np.full((4, 4), np.nan)
    for (p, q), v in mu.items():
        cen[p, q] = float(v)
    out["moments_central"] = cen
    n = mu[(0, 0)]
    a, b, c = mu[(0, 2)] / n, -mu[(1, 1)] / n, mu[(2, 0)] / n
    out["inertia_tensor"] = np.array([[float(a), float(b)], [float(b), float(c)]])
    half_trace, det = _dec(a + c) / 2, _dec(a * c - b * b)
    disc = (half_trace * half_trace - det).max(Decimal(0)).sqrt()
    l1, l2 = float(half_trace + disc), max(float(half_trace - disc), 0.0)
    out["eigvals"] = [l1, l2]
    out["major_axis_length"] = 4 * math.sqrt(l1)
    out["minor_axis_length"] = 4 * math.sqrt(l2)
    out["eccentricity"] = 0.0 if l1 == 0 else math.sqrt(1 - l2 / l1)
    if a == c:
        out["orientation"] = -math.pi / 4 if b < 0 else math.pi / 4
    else:
        out["orientation"] = 0.5 * math.atan2(float(-2 * b), float(c - a))
    nu = {pq: cen[pq] / cen[0, 0] ** ((pq[0] + pq[1]) / 2 + 1) for pq in mu if pq[0] + pq[1] >= 2}
    n20, n02, n11, n30, n03, n21, n12 = (nu[k] for k in ((2, 0), (0, 2), (1, 1), (3, 0), (0, 3), (2, 1), (1, 2)))
    out["moments_hu"] = np.array([
        n20 + n02,
        (n20 - n02) ** 2 + 4 * n11 ** 2,
        (n30 - 3 * n12) ** 2 + (3 * n21 - n03) ** 2,
        (n30 + n12) ** 2 + (n21 + n03) ** 2,
        (n30 - 3 * n12) * (n30 + n12) * ((n30 + n12) ** 2 - 3 * (n21 + n03) ** 2)
        + (3 * n21 - n03) * (n21 + n03) * (3 * (n30 + n12) ** 2 - (n21 + n03) ** 2),
        (n20 - n02) * ((n30 + n12) ** 2 - (n21 + n03) ** 2) + 4 * n11 * (n30 + n12) * (n21 + n03),
        (3 * n21 - n03) * (n30 + n12) * ((n30 + n12) ** 2 - 3 * (n21 + n03) ** 2)
        - (n30 - 3 * n12) * (n21 + n03) * (3 * (n30 + n12) ** 2 - (n21 + n03) ** 2)])
    rr, cc = np.nonzero(mask)
    area = len(rr)
    bbox_area = int(rr.max() + 1 - rr.min()) * int(cc.max() + 1 - cc.min())
    border, perim = border_and_classes(mask)
    out["perimeter"] = perim[0] + perim[1] * math.sqrt(2) + perim[2] * ((1 + math.sqrt(2)) / 2)
    out["extent"] = area / bbox_area
    out["equivalent_diameter"] = math.sqrt(4 * area / math.pi)
    q = quads(mask)
    out["euler_number"] = (q[0] - q[1] - 2 * q[2]) // 4
    return out


def euler_by_labelling(mask):
    """8-connected components minus 4-connected holes (background components that do not reach the padded frame)"""
    eight = np.ones((3, 3), bool)
    ncomp = ndimage.label(mask, eight)[1]
    bg = np.pad(~mask.astype(bool), 1, constant_values=True)
    nbg = ndimage.label(bg, CROSS)[1]
    return ncomp - (nbg - 1)


def holes_8(mask):
    """holes counted with an 8-neighbourhood, as skimage 0.15's euler_number counts them"""
    bg = np.pad(~mask.astype(bool), 1, constant_values=True)
    return ndimage.label(bg, np.ones((3, 3), bool))[1] - 1
