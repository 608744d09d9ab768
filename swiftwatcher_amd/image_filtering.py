"""Drop-in for the preprocessing + segmentation sections of the reference's
swiftwatcher/image_filtering.py (lines 188-369): same function names, argument meaning and
return types, every pixel operation running as a HIP kernel on the MI355X through
libswk.so (ctypes, swiftwatcher_amd/_lib.py).  No OpenCV / SciPy / scikit-image involved
and no CPU fallback: without the GPU library these functions raise SwkError.

The ROI-mask section of the reference file (generate_regions / generate_roi_mask and friends, lines 20-28 and
99-180) runs once per video on a few hundred by a hundred pixels and feeds the host-side tracker: it is host C++ in
the same library (csrc/roi_mask.cpp), same function names here.
"""
import math

import numpy as np

from . import _lib

###############################################################################
# crop geometry -- pure integer arithmetic, image_filtering.py:31-91
###############################################################################


def determine_chimney_extents(corners):
    """image_filtering.py:78-91: (left, right, bottom) of the two chimney corners."""
    left = min(corners[0][0], corners[1][0])
    right = max(corners[0][0], corners[1][0])
    bottom = max(corners[0][1], corners[1][1])
    return left, right, bottom


def generate_crop_region(corners):
    """image_filtering.py:31-53: [(x0, y0), (x1, y1)], 1.25 x 0.625 chimney widths."""
    left, right, bottom = determine_chimney_extents(corners)
    width = right - left
    return [(left - int(0.125 * width), bottom - int(0.5 * width)),
            (right + int(0.125 * width), bottom + int(0.125 * width))]


def generate_roi_crop_region(corners):
    """image_filtering.py:56-75."""
    left, right, bottom = determine_chimney_extents(corners)
    width = right - left
    return [(int(left + 0.025 * width), int(bottom - 0.25 * width)),
            (int(right - 0.025 * width), int(bottom))]


def crop_frame(frame, crop_region):
    """image_filtering.py:199-203: a view, like the reference."""
    return frame[crop_region[0][1]:crop_region[1][1], crop_region[0][0]:crop_region[1][0]]


###############################################################################
# ROI mask -- once per video, host C++ (image_filtering.py:20-28, 99-180); PARITY UNPINNED (cv2)
###############################################################################


def generate_regions(first_frame, corners):
    """image_filtering.py:20-28: (crop_region, roi_mask, resize_dim) for a video, from its first frame and the two
    chimney corners.  resize_dim is handed through like in the reference (its resize step is commented out there)."""
    resize_dim = (300, 150)
    crop_region, roi_mask = _lib.roi_mask(first_frame, corners)
    return crop_region, roi_mask, resize_dim


def generate_roi_mask(frame, corners, crop_region=None, resize_dim=None):
    """image_filtering.py:99-122 (crop_region is recomputed from the corners, as generate_regions does)."""
    return _lib.roi_mask(frame, corners)[1]


def median_blur(image, kernel_size):
    """image_filtering.py:125-131 (cv2.medianBlur)."""
    return _lib.median_blur_u8(image, kernel_size)


def split_bgr_channels(image):
    """image_filtering.py:134-139 (cv2.split)."""
    return (np.ascontiguousarray(image[:, :, 0]), np.ascontiguousarray(image[:, :, 1]), np.ascontiguousarray(image[:, :, 2]))


def threshold_channel(image):
    """image_filtering.py:142-151: Otsu's threshold, binary 0 / 255 output."""
    return _lib.otsu_threshold_u8(image)[1]


def detect_canny_edges(image):
    """image_filtering.py:154-159: cv2.Canny(image, 0, 256)."""
    return _lib.canny_u8(image, 0, 256)


def dilate_upwards(image, N):
    """image_filtering.py:162-170: N x 1 kernel anchored at its top, so edges only grow upwards."""
    return _lib.dilate_up_u8(image, N)


def create_mask(mask, frame_region, frame):
    """image_filtering.py:173-181: the ROI-sized mask pasted into a blank single-channel image of the frame's size."""
    out = np.zeros(frame.shape[:2], np.uint8)
    out[frame_region[0][1]:frame_region[1][1], frame_region[0][0]:frame_region[1][0]] = mask
    return out


###############################################################################
# stages -- each one a HIP kernel behind the C ABI
###############################################################################


def _ctx():
    return _lib.default_context()


def convert_grayscale(frame, gray_mode=_lib.GRAY_Q14):
    """image_filtering.py:188-196.  3-channel BGR -> gray with OpenCV 4.1.0's fixed-point
    weights; a 2-D frame passes through unchanged (:193-194)."""
    if frame.ndim == 2:
        return frame
    return _ctx().bgr2gray(frame, gray_mode)


def inexact_augmented_lagrange_multiplier(X, lmbda=0.01, tol=0.001, maxiter=100, verbose=False):
    """image_filtering.py:256-301.  X: (pixels, frames) uint8 matrix of column-vector images.
    Returns (A, E) float64 (pixels, frames)."""
    X = np.asarray(X)
    if X.dtype != np.uint8:
        raise TypeError("the HIP IALM takes the uint8 image matrix the reference passes (image_filtering.py:234-241)")
    planes = np.ascontiguousarray(X.T)
    A, E, it = _ctx().ialm(planes, lmbda, tol, maxiter, want_E=True)
    if verbose:
        print("Finished at iteration %d" % it)
    return A, E


def rpca(frame_list):
    """image_filtering.py:220-253: list of n gray frames -> list of n uint8 sparse images."""
    stack = np.ascontiguousarray(np.array(frame_list), np.uint8)
    n, H, W = stack.shape
    res = _ctx().batch_run(stack, 1, n, stages=("rpca",), seg_cap=1)
    return [res["rpca"][i] for i in range(n)]


def bilateral_blur(frame, d, sigmaColor, sigmaSpace, use_fma=False):
    """image_filtering.py:304-307."""
    return _ctx().bilateral_u8(frame, d, float(sigmaColor), float(sigmaSpace), use_fma)


def thresh_to_zero(frame, thresh):
    """image_filtering.py:310-316."""
    return _ctx().thresh_tozero_u8(frame, int(thresh))


def grayscale_opening(frame, SE):
    """image_filtering.py:319-322: scipy.ndimage.grey_opening(frame, size=SE).  (3, 3) -- the window the reference uses
    (data_structures.py:202) -- runs on the tiled kernel, any other window on the general one."""
    if tuple(SE) == (3, 3):
        return _ctx().grey_open3x3_u8(frame)
    return _ctx().grey_open_u8(frame, tuple(SE))


def resize_frame(frame, dimensions):
    """image_filtering.py:206-212: cv2.resize(frame, dimensions) with dimensions = (width, height).  The reference's two call
    sites are commented out (data_structures.py:179-181, image_filtering.py:117-118); PARITY UNPINNED (cv2)."""
    return _ctx().resize_linear_u8(frame, dimensions)


def cc_labeling(frame, connectivity=None, effective_connectivity=8, label_order=_lib.ORDER_BLOCK2X2):
    """image_filtering.py:325-329.

    The reference calls cv2.connectedComponents(frame, connectivity) with connectivity=4
    (data_structures.py:206), but the binding's second positional parameter is `labels`, so
    OpenCV runs its defaults: 8-connectivity, BBDT numbering.  To stay a drop-in the positional
    `connectivity` is accepted and, like there, has no effect; use effective_connectivity /
    label_order to choose something else.  Returns uint8 labels (wraps mod 256 like astype)."""
    _, lab = _ctx().ccl_u8(frame, effective_connectivity, label_order)
    return (lab & 0xff).astype(np.uint8)


class RegionProps:
    """The regionprops fields the rest of swiftwatcher reads (label, bbox, centroid, area)."""
    __slots__ = ("label", "bbox", "centroid", "area")

    def __init__(self, label, bbox, centroid, area):
        self.label = label
        self.bbox = bbox
        self.centroid = centroid
        self.area = area

    def __repr__(self):
        return "RegionProps(label=%d, bbox=%r, centroid=%r, area=%d)" % (self.label, self.bbox, self.centroid, self.area)


def regionprops_from_records(records):
    """swk_segment records -> RegionProps list.  The centroid is sum/area in float64, which is
    bit-identical to skimage's coords.mean(axis=0)."""
    if len(records) == 0:
        return []
    area = records["area"].astype(np.float64)
    cr = (records["sum_r"].astype(np.float64) / area).tolist()
    cc = (records["sum_c"].astype(np.float64) / area).tolist()
    return [RegionProps(lab, (r0, c0, r1, c1), (a, b), ar)
            for lab, r0, c0, r1, c1, ar, a, b in zip(records["label"].tolist(), records["r0"].tolist(), records["c0"].tolist(),
                                                     records["r1"].tolist(), records["c1"].tolist(), records["area"].tolist(),
                                                     cr, cc)]


def get_segment_properties(frame, shape=False):
    """image_filtering.py:332-335: one RegionProps per distinct nonzero label, ascending.  shape=True: ShapeRegionProps, which
    also carry the shape properties of ShapeMeasures (one more library call, swk_segment_shapes_u8)."""
    segs, _ = _ctx().regionprops_u8(frame)
    props = regionprops_from_records(segs)
    if not shape:
        return props
    recs, _ = _ctx().segment_shapes_u8(np.ascontiguousarray(frame, np.uint8))
    return [ShapeRegionProps(p.label, p.bbox, p.centroid, p.area, ShapeMeasures(p.bbox, rec)) for p, rec in zip(props, shape_records(recs))]


###############################################################################
# shape properties -- derived on the host from the exact integer sums of swk_segment_shapes_u8
###############################################################################

SHAPE_PROPERTIES = ("moments", "local_centroid", "moments_central", "moments_normalized", "moments_hu", "inertia_tensor",
                    "inertia_tensor_eigvals", "major_axis_length", "minor_axis_length", "eccentricity", "orientation", "bbox_area",
                    "extent", "equivalent_diameter", "perimeter", "euler_number")
SHAPE_NOT_PROVIDED = ("convex_area", "convex_image", "solidity", "filled_area", "filled_image", "image", "coords", "intensity_image",
                      "max_intensity", "mean_intensity", "min_intensity", "weighted_centroid", "weighted_local_centroid",
                      "weighted_moments", "weighted_moments_central", "weighted_moments_hu", "weighted_moments_normalized")
_MOMENT_INDEX = {pq: k for k, pq in enumerate(_lib.SHAPE_MOMENT_ORDER)}
_BINOM = ((1,), (1, 1), (1, 2, 1), (1, 3, 3, 1))


def shape_records(records):
    """SHAPE_DTYPE records -> per record the plain tuple ShapeMeasures takes: (m (10 ints), border, perim (3), quads (3))."""
    return [(tuple(m), b, tuple(p), tuple(q)) for m, b, p, q in zip(records["m"].tolist(), records["border"].tolist(),
                                                                      records["perim"].tolist(), records["quads"].tolist())]


def _not_provided(name):
    return AttributeError("%s is not provided: the shape properties are functions of a region's integer sums (%s); not provided are %s"
                          % (name, ", ".join(SHAPE_PROPERTIES), ", ".join(SHAPE_NOT_PROVIDED)))


def _translated(m, dr, dc, order=3):
    """Power sums about another origin: sum (r - dr)^p (c - dc)^q for p + q <= order from the sums m about 0, by the binomial
    expansion; exact for int and Fraction shifts.  {(p, q): value}."""
    out = {}
    for p in range(order + 1):
        for q in range(order + 1 - p):
            total = 0
            for i in range(p + 1):
                for j in range(q + 1):
                    total += _BINOM[p][i] * _BINOM[q][j] * (-dr) ** (p - i) * (-dc) ** (q - j) * m[_MOMENT_INDEX[(i, j)]]
            out[(p, q)] = total
    return out


def _sqrt_fraction(x, bits=160):
    """sqrt of a non-negative Fraction as a Fraction, to `bits` bits below one (exact when x is a rational square)."""
    from fractions import Fraction
    return Fraction(math.isqrt((x.numerator * x.denominator) << (2 * bits)), x.denominator << bits)


class ShapeMeasures:
    """The regionprops attributes that are functions of one region's integer sums (a swk_segment_shape record: m = sums of r^p c^q
    in absolute plane coordinates, border, perim, quads) and its bbox, each computed when first read and kept.  Every value is
    carried in exact Python integers / Fractions up to the one point where a float is formed.

    PARITY UNPINNED: scikit-image is not installed where this project is built and tested; the formulas below (skimage's, in
    row / column coordinates) are the specification.
      moments             4x4 float64, M[p, q] = sum (r - r0)^p (c - c0)^q (bbox-local raw moments), from the absolute sums by the
                          binomial expansion in integers.  DEVIATION: entries with p + q > 3 are nan (none of the derived
                          properties reads them; they would need 128-bit sums)
      local_centroid      (M10 / M00, M01 / M00)
      moments_central     mu[p, q] about the centroid, formed as exact rationals (mu20 = (m20 m00 - m10^2) / m00, ...) and rounded
                          once; nan for p + q > 3.  exact_central gives the rationals
      moments_normalized  nu[p, q] = mu[p, q] / mu00^((p + q) / 2 + 1) for p + q >= 2, nan below (and above 3)
      moments_hu          the seven invariants of nu
      inertia_tensor      [[mu02, -mu11], [-mu11, mu20]] / mu00
      inertia_tensor_eigvals  descending, clipped at 0: (T +- sqrt(D)) / 2 of the exact tensor, T its trace, D = (a - c)^2 + 4 b^2,
                          the square root taken to 160 bits and the value rounded once
      major_axis_length, minor_axis_length  4 sqrt(l1), 4 sqrt(l2)
      eccentricity        sqrt(1 - l2 / l1), 0 when l1 == 0
      orientation         with a, b, b, c = inertia_tensor.flat: 0.5 atan2(-2 b, c - a); when a == c, -pi / 4 for b < 0 and pi / 4
                          otherwise.  a == c is decided and -2 b and c - a are formed on the exact tensor
      bbox_area, extent   extent = area / bbox_area
      equivalent_diameter sqrt(4 area / pi)
      perimeter           perim[0] + perim[1] sqrt(2) + perim[2] (1 + sqrt(2)) / 2 (skimage.measure.perimeter(image, 4) of 0.15.0)
      euler_number        (quads[0] - quads[1] - 2 quads[2]) / 4, the 8-connected Euler number.  DEVIATION: skimage 0.15 counts holes
                          with an 8-neighbourhood; the two differ only where two holes touch diagonally
    Not provided (reading one raises AttributeError): SHAPE_NOT_PROVIDED."""

    def __init__(self, bbox, record):
        self.bbox = tuple(int(x) for x in bbox)
        m, border, perim, quads = record
        self.m, self.border, self.perim, self.quads = tuple(int(x) for x in m), int(border), tuple(perim), tuple(quads)
        self.area = self.m[0]
        self._cache = {}

    def __getattr__(self, name):
        if name in SHAPE_PROPERTIES or name in ("exact_central", "exact_tensor"):
            cache = self.__dict__["_cache"]
            if name not in cache:
                cache[name] = getattr(self, "_" + name)()
            return cache[name]
        if name in SHAPE_NOT_PROVIDED:
            raise _not_provided(name)
        raise AttributeError(name)

    @staticmethod
    def _matrix(values):
        out = np.full((4, 4), np.nan)
        for (p, q), v in values.items():
            out[p, q] = v if isinstance(v, float) else v.numerator / v.denominator
        return out

    def _moments(self):
        return self._matrix(_translated(self.m, self.bbox[0], self.bbox[1]))

    def _local_centroid(self):
        M = _translated(self.m, self.bbox[0], self.bbox[1], 1)
        return (M[(1, 0)] / M[(0, 0)], M[(0, 1)] / M[(0, 0)])

    def _exact_central(self):
        """{(p, q): Fraction} for p + q <= 3"""
        from fractions import Fraction
        # in integers: with N = m00, sum (N r - m10)^p (N c - m01)^q = N^(p + q) mu[p, q], and the sums of (N r)^i (N c)^j are N^(i + j) m[i, j]
        n = self.m[0]
        scaled = [v * n ** (i + j) for (i, j), v in zip(_lib.SHAPE_MOMENT_ORDER, self.m)]
        return {pq: Fraction(v, n ** (pq[0] + pq[1])) for pq, v in _translated(scaled, self.m[1], self.m[2]).items()}

    def _moments_central(self):
        return self._matrix(self.exact_central)

    def _moments_normalized(self):
        mu = self.moments_central
        nu = np.full((4, 4), np.nan)
        for p in range(4):
            for q in range(4 - p):
                if p + q >= 2:
                    nu[p, q] = mu[p, q] / mu[0, 0] ** ((p + q) / 2 + 1)
        return nu

    def _moments_hu(self):
        nu = self.moments_normalized
        n20, n02, n11, n30, n03, n21, n12 = nu[2, 0], nu[0, 2], nu[1, 1], nu[3, 0], nu[0, 3], nu[2, 1], nu[1, 2]
        t0, t1 = n30 + n12, n21 + n03
        q0, q1 = t0 * t0, t1 * t1
        n4 = 4 * n11
        s, d = n20 + n02, n20 - n02
        hu = np.zeros(7)
        hu[0] = s
        hu[1] = d * d + n4 * n11
        hu[3] = q0 + q1
        hu[5] = d * (q0 - q1) + n4 * t0 * t1
        t0, t1 = t0 * (q0 - 3 * q1), t1 * (3 * q0 - q1)
        q0, q1 = n30 - 3 * n12, 3 * n21 - n03
        hu[2] = q0 * q0 + q1 * q1
        hu[4] = q0 * t0 + q1 * t1
        hu[6] = q1 * t0 - q0 * t1
        return hu

    def _exact_tensor(self):
        """(a, b, c) of [[a, b], [b, c]] as Fractions"""
        mu = self.exact_central
        n = mu[(0, 0)]
        return mu[(0, 2)] / n, -mu[(1, 1)] / n, mu[(2, 0)] / n

    def _inertia_tensor(self):
        a, b, c = (x.numerator / x.denominator for x in self.exact_tensor)
        return np.array([[a, b], [b, c]])

    def _inertia_tensor_eigvals(self):
        a, b, c = self.exact_tensor
        root = _sqrt_fraction((a - c) ** 2 + 4 * b * b)
        l1, l2 = (a + c + root) / 2, (a + c - root) / 2
        return [max(l1.numerator / l1.denominator, 0.0), max(l2.numerator / l2.denominator, 0.0)]

    def _major_axis_length(self):
        return 4 * math.sqrt(self.inertia_tensor_eigvals[0])

    def _minor_axis_length(self):
        return 4 * math.sqrt(self.inertia_tensor_eigvals[1])

    def _eccentricity(self):
        l1, l2 = self.inertia_tensor_eigvals
        return 0.0 if l1 == 0 else math.sqrt(1 - l2 / l1)

    def _orientation(self):
        a, b, c = self.exact_tensor
        if a == c:
            return -math.pi / 4 if b < 0 else math.pi / 4
        y, x = -2 * b, c - a
        return 0.5 * math.atan2(y.numerator / y.denominator, x.numerator / x.denominator)

    def _bbox_area(self):
        r0, c0, r1, c1 = self.bbox
        return (r1 - r0) * (c1 - c0)

    def _extent(self):
        return self.area / self.bbox_area

    def _equivalent_diameter(self):
        return math.sqrt(4 * self.area / math.pi)

    def _perimeter(self):
        p = self.perim
        return p[0] + p[1] * math.sqrt(2) + p[2] * ((1 + math.sqrt(2)) / 2)

    def _euler_number(self):
        q = self.quads
        return (q[0] - q[1] - 2 * q[2]) // 4


class ShapeRegionProps(RegionProps):
    """RegionProps that also answers the shape properties (SHAPE_PROPERTIES) from its ShapeMeasures, each made on first read."""
    __slots__ = ("shape",)

    def __init__(self, label, bbox, centroid, area, shape):
        RegionProps.__init__(self, label, bbox, centroid, area)
        self.shape = shape

    def __getattr__(self, name):
        if name in SHAPE_PROPERTIES:
            return getattr(self.shape, name)
        if name in SHAPE_NOT_PROVIDED:
            raise _not_provided(name)
        raise AttributeError(name)


def segment_crop_box(bbox, frame_shape, min_seg_size, crop_region):
    """The rows / columns of the full frame extract_segment_images slices for one region (image_filtering.py:345-366)."""
    r0, c0, r1, c1 = bbox
    h, w = r1 - r0, c1 - c0
    if h < min_seg_size[0]:
        d = min_seg_size[0] - h
        r0 -= d // 2
        r1 += d - d // 2
    if w < min_seg_size[1]:
        d = min_seg_size[1] - w
        c0 -= d // 2
        c1 += d - d // 2
    oy, ox = crop_region[0][1], crop_region[0][0]
    return max(r0 + oy, 0), max(r1 + oy, 0), max(c0 + ox, 0), max(c1 + ox, 0)


def segment_image_getter(segment, frame, min_seg_size, crop_region):
    """Zero-argument callable that cuts one region's segment image (the same view extract_segment_images makes) when it is
    first needed: data_structures.Segment resolves it on the first read of .segment_image."""
    bbox = segment.bbox

    def cut():
        r0, r1, c0, c1 = segment_crop_box(bbox, frame.shape, min_seg_size, crop_region)
        return frame[r0:r1, c0:c1]
    return cut


def extract_segment_images(segments, frame, min_seg_size, crop_region):
    """image_filtering.py:338-369: expand each bbox to at least min_seg_size (floor/ceil split),
    translate by the crop origin and slice the FULL frame (views).

    One deliberate deviation: a box whose top or left edge leaves the frame is intersected with the frame.
    The reference's unchecked slice wraps a negative start around (numpy semantics), which yields an empty or
    unrelated crop that its classifier then fails on; boxes leaving the bottom / right edge are clipped by numpy
    in the reference too.  swk_segment_inputs (the device-resident path) uses the same rule, so both
    classification paths see the same crop for every segment."""
    images = []
    oy, ox = crop_region[0][1], crop_region[0][0]
    for segment in segments:
        r0, c0, r1, c1 = segment.bbox
        h, w = r1 - r0, c1 - c0
        if h < min_seg_size[0]:
            d = min_seg_size[0] - h
            r0 -= math.floor(d / 2)
            r1 += math.ceil(d / 2)
        if w < min_seg_size[1]:
            d = min_seg_size[1] - w
            c0 -= math.floor(d / 2)
            c1 += math.ceil(d / 2)
        images.append(frame[max(r0 + oy, 0):max(r1 + oy, 0), max(c0 + ox, 0):max(c1 + ox, 0)])
    return images
