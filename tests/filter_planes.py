"""Designed u8 planes for the fused filter kernel of the batch calls (csrc/filters.hip, k_filter_fused<GEOM, R>: bilateral filter,
to-zero threshold, 3 x 3 grey opening on one 32 x 64 tile per workgroup) and a plain float64 statement of the three stages, shared by
tests/test_filter_planes_cpu.py and tests/test_filter_planes_gpu.py.  swk_debug_filter_fused (include/swk_debug.h) hands the kernel
these planes; in a batch call it only ever reads what the RPCA left: dark blobs of 50-90 grey levels on a zero background.

Every family is deterministic and yields Family tuples: a name, a (F, H, W) u8 stack and the parameter sets P(d, sc, ss, fma, thresh)
it runs at.  What each family is for:

  dense       full-range and near-threshold planes at every shape at which the tile arithmetic changes: the live list fills, the
              colour table is read to its far end, sum / wsum comes near rounding ties;
  lone        70 x 135 frames (two full tiles and a ragged third, both ways), zero except one pixel or one 3 x 3 block placed at
              chosen distances from the tile seams, and "tips": pixels at distance exactly R left, right, above and below an
              empty cell (all four, or one pair).  Wide sigmas, because at the reference's sigma_space = 1 a lone pixel leaves
              nothing at distance R;
  border      content within R + 2 of the edges and corners only (BORDER_REFLECT_101 of the filter, edge handling of the opening);
  thresholds  thresh 0, 15, 16, 254, 255 on random planes, all-15 and all-16 planes;
  geom        several plane sizes in one buffer at byte offsets of every residue mod 4 with gaps between them.

The numpy mutants at the bottom are wrong kernels a test can run on the CPU: tests/test_filter_planes_cpu.py shows that each differs
from the oracle on the family meant to catch it, and where."""
import functools
from collections import namedtuple

import numpy as np

Family = namedtuple("Family", "name planes params")
P = namedtuple("P", "d sc ss fma thresh")
GeomCase = namedtuple("GeomCase", "name buf geom planes params")          # geom: [(H, W, byte offset)], planes: the stacks at those places

TILE_H, TILE_W = 32, 64                                   # kTH, kTW of csrc/filters.hip
DEFAULT = (7, 15.0, 1.0)                                  # the reference's bilateral parameters: radius 3
WIDE = [(9, 40.0, 3.0), (-1, 25.0, 2.5), (7, 60.0, 3.0), (5, 40.0, 2.0)]          # radius 4, 4 (from sigma_space), 3, 2
THRESHOLDS = (0, 15, 16, 254, 255)
LONE_VALUES = (16, 30, 60, 255)
LONE_SHAPE = (70, 135)
LONE_ROWS = (0, 1) + tuple(range(29, 36)) + tuple(range(61, 67)) + (68, 69)
LONE_COLS = (0, 1) + tuple(range(59, 70)) + tuple(range(123, 132)) + (133, 134)
DENSE_SHAPES = [(4, 4), (4, 5), (5, 4), (5, 7), (4, 130), (130, 4), (31, 63), (32, 64), (33, 65), (36, 68), (47, 94), (67, 95),
                (64, 128), (65, 129), (40, 61), (40, 62), (40, 63), (40, 64), (40, 65), (40, 66), (40, 67)]
GEOM_SHAPES = [(70, 135), (4, 4), (33, 65), (5, 7), (47, 94), (40, 64)]          # the last one all zero


def bil_list():
    """the radius 1..4 sets of tests/test_batch_bilateral_params_gpu.py (one list for both files)"""
    from test_batch_bilateral_params_gpu import BIL
    return list(BIL)


def radius(d, sigma_space):
    """OpenCV's: from the diameter, or from sigma_space when d <= 0; at least 1"""
    ss = sigma_space if sigma_space > 0 else 1.0
    r = int(np.rint(ss * 1.5)) if d <= 0 else d // 2
    return max(r, 1)


def psets(bils, fmas=(0, 1), threshs=(15,)):
    return [P(b[0], b[1], b[2], f, t) for b in bils for f in fmas for t in threshs]


# ------------------------------------------------------------------ float64 reference
def reflect101_index(n, R):
    """source index of positions -R .. n + R - 1 under BORDER_REFLECT_101, reflected as often as a small image needs"""
    out = []
    for p in range(-R, n + R):
        while n > 1 and (p < 0 or p >= n):
            p = -p if p < 0 else 2 * (n - 1) - p
        out.append(p if n > 1 else 0)
    return np.array(out)


def clamp_index(n, R):
    return np.clip(np.arange(-R, n + R), 0, n - 1)


def padded(planes, R, border="reflect101"):
    idx = reflect101_index if border == "reflect101" else clamp_index
    return planes[:, idx(planes.shape[1], R)][:, :, idx(planes.shape[2], R)]


def bilateral_quotient(planes, d, sc, ss, border="reflect101"):
    """sum / wsum of the bilateral filter in float64: taps with i^2 + j^2 <= R^2, weights exp(-(i^2 + j^2) / (2 ss^2)) exp(-dv^2 / (2 sc^2))"""
    planes = np.asarray(planes)
    F, H, W = planes.shape
    R = radius(d, ss)
    sc = sc if sc > 0 else 1.0
    ss = ss if ss > 0 else 1.0
    cw = np.exp(-0.5 * np.arange(256, dtype=np.float64) ** 2 / (sc * sc))
    pad = padded(planes, R, border).astype(np.int16)
    v0 = planes.astype(np.int16)
    s = np.zeros((F, H, W), np.float64)
    ws = np.zeros((F, H, W), np.float64)
    for i in range(-R, R + 1):
        for j in range(-R, R + 1):
            if i * i + j * j > R * R:
                continue
            v = pad[:, R + i:R + i + H, R + j:R + j + W]
            w = np.exp(-0.5 * (i * i + j * j) / (ss * ss)) * cw[np.abs(v - v0)]
            s += v * w
            ws += w
    return s / ws


def round_u8(q):
    return np.rint(q).astype(np.uint8)          # cvRound: half to even


def thresh_tozero(img, thresh, ge=False):
    return np.where(img >= thresh if ge else img > thresh, img, 0).astype(np.uint8)


def grey_open3x3(stack, zero_border=False):
    from scipy import ndimage
    kw = dict(mode="constant", cval=0) if zero_border else dict(mode="reflect")
    return ndimage.grey_opening(np.asarray(stack), size=(1, 3, 3), **kw)


def reference_stages(planes, p):
    """(bilateral, thresholded, opened) by the float64 statement"""
    bil = round_u8(bilateral_quotient(planes, p.d, p.sc, p.ss))
    thr = thresh_tozero(bil, p.thresh)
    return bil, thr, grey_open3x3(thr)


# ------------------------------------------------------------------ the CPU oracle on a stack, once per (family, parameter set)
_ORACLE = {}


def oracle_stages(name, planes, p):
    """(bilateral, thresholded, opened) stacks of oracle.reference_path on every plane; cached by family name and parameter set"""
    key = (name, p)
    if key not in _ORACLE:
        from oracle import reference_path as orc
        bil = np.stack([orc.bilateral_u8(f, p.d, p.sc, p.ss, bool(p.fma)) for f in planes])
        thr = np.stack([orc.thresh_tozero_u8(f, p.thresh) for f in bil])
        opened = np.stack([orc.grey_open_u8(f, (3, 3)) for f in thr])
        for a in (bil, thr, opened):
            a.setflags(write=False)
        _ORACLE[key] = (bil, thr, opened)
    return _ORACLE[key]


# ------------------------------------------------------------------ dense
def dense_stack(H, W, seed):
    """uniform random 0..255, random 0..40, 1- and 2-pixel checkerboards of 0 / 255, all 255, all 16, all 15, all 0, a horizontal ramp"""
    rng = np.random.default_rng(seed)
    r, c = np.indices((H, W))
    frames = [rng.integers(0, 256, size=(H, W)), rng.integers(0, 41, size=(H, W)),
              np.where((r + c) % 2 == 0, 255, 0), np.where((r // 2 + c // 2) % 2 == 0, 255, 0),
              np.full((H, W), 255), np.full((H, W), 16), np.full((H, W), 15), np.zeros((H, W)),
              (c * 255) // max(W - 1, 1) + 0 * r]
    return np.ascontiguousarray(np.stack(frames).astype(np.uint8))


DENSE_FRAMES = ("random", "random40", "checker1", "checker2", "all255", "all16", "all15", "all0", "ramp")


@functools.lru_cache(maxsize=None)
def dense_families():
    """every dense shape as one stack of nine frames (an odd H * W puts the plane bases on every residue mod 4) at radius 1..4 through
    the BIL list and the default set, bil_fma 0 and 1"""
    sets = psets(bil_list() + [DEFAULT])
    return [Family("dense_%dx%d" % (H, W), dense_stack(H, W, 4100 + 131 * H + W), sets) for H, W in DENSE_SHAPES]


# ------------------------------------------------------------------ thresholds
@functools.lru_cache(maxsize=None)
def threshold_families():
    """thresh 0, 15, 16, 254, 255 on the dense stacks (random 0..40, full range, all-15 and all-16 among them) of four shapes"""
    out = []
    for H, W in [(5, 7), (33, 65), (40, 66), (67, 95)]:
        out.append(Family("thresholds_%dx%d" % (H, W), dense_stack(H, W, 4100 + 131 * H + W), psets([DEFAULT, WIDE[0]], threshs=THRESHOLDS)))
    return out


# ------------------------------------------------------------------ lone
def lone_places():
    """the cross product of LONE_ROWS and LONE_COLS: 18 x 24 places, one frame each"""
    return [(r, c) for r in LONE_ROWS for c in LONE_COLS]


TIPS = {"tips": ((-1, 0), (1, 0), (0, -1), (0, 1)), "hpair": ((0, -1), (0, 1)), "vpair": ((-1, 0), (1, 0))}


def tips_frames():
    """[(kind, R, (r, c))]: pixels of 30 at distance exactly R from the empty cell (r, c), nothing nearer -- left, right, above and
    below it ("tips"), left and right only ("hpair"), above and below only ("vpair")"""
    centres = {"tips": ((32, 64), (31, 63), (33, 66), (35, 128), (4, 4), (65, 130)), "hpair": ((32, 64), (31, 63), (35, 128)),
               "vpair": ((32, 64), (31, 63), (35, 128))}
    return [(kind, R, rc) for kind in ("tips", "hpair", "vpair") for R in (2, 3, 4) for rc in centres[kind]]


# kind: "pixel", "block" (3 x 3, top-left corner clipped into the frame), "tipsR" / "hpairR" / "vpairR" (R the distance)
LoneFrame = namedtuple("LoneFrame", "kind r c value")


@functools.lru_cache(maxsize=None)
def lone_layout():
    out = []
    for r, c in lone_places():          # kinds and values change along rows and along columns
        ri, ci = LONE_ROWS.index(r), LONE_COLS.index(c)
        out.append(LoneFrame("block" if (ri + ci) % 3 == 2 else "pixel", r, c, LONE_VALUES[(ci - ri) % 4]))
    out += [LoneFrame("%s%d" % (kind, R), r, c, 30) for kind, R, (r, c) in tips_frames()]
    return tuple(out)


def lone_stack():
    H, W = LONE_SHAPE
    lay = lone_layout()
    st = np.zeros((len(lay), H, W), np.uint8)
    for k, f in enumerate(lay):
        if f.kind == "pixel":
            st[k, f.r, f.c] = f.value
        elif f.kind == "block":
            r0, c0 = min(f.r, H - 3), min(f.c, W - 3)
            st[k, r0:r0 + 3, c0:c0 + 3] = f.value
        else:
            R = int(f.kind[-1])
            for dr, dc in TIPS[f.kind[:-1]]:
                st[k, f.r + R * dr, f.c + R * dc] = f.value
    return st


@functools.lru_cache(maxsize=None)
def lone_families():
    return [Family("lone_70x135", lone_stack(), psets(WIDE + [DEFAULT]))]


# ------------------------------------------------------------------ border
BORDER_BAND = 6          # R + 2 at the largest radius


def border_stack(H, W, seed):
    """content within BORDER_BAND of the edges only: random 0..255, random 0..60, the four corners alone, a constant 200"""
    rng = np.random.default_rng(seed)
    r, c = np.indices((H, W))
    b = BORDER_BAND
    band = (r < b) | (r >= H - b) | (c < b) | (c >= W - b)
    corner = ((r < b) | (r >= H - b)) & ((c < b) | (c >= W - b))
    frames = [np.where(band, rng.integers(0, 256, size=(H, W)), 0), np.where(band, rng.integers(0, 61, size=(H, W)), 0),
              np.where(corner, rng.integers(17, 256, size=(H, W)), 0), np.where(band, 200, 0)]
    return np.ascontiguousarray(np.stack(frames).astype(np.uint8))


@functools.lru_cache(maxsize=None)
def border_families():
    """the dense shapes up to 67 x 95, radius 1, 2, 3 and 4"""
    sets = psets([(3, 15.0, 1.0), (5, 15.0, 1.0), DEFAULT, WIDE[0]])
    return [Family("border_%dx%d" % (H, W), border_stack(H, W, 5200 + 131 * H + W), sets) for H, W in DENSE_SHAPES if H <= 67 and W <= 95]


def all_families():
    return dense_families() + threshold_families() + lone_families() + border_families()


# ------------------------------------------------------------------ geom
def _geom_plane(H, W, k, rng):
    if (H, W) == (40, 64):
        return np.zeros((H, W), np.uint8)
    if (H, W) == LONE_SHAPE:          # sparse: pixels and blocks at the seams on a zero background, and a dense patch over a tile corner
        p = np.zeros((H, W), np.uint8)
        for r, c, v in ((31, 63, 255), (32, 64, 60), (0, 134, 30), (69, 0, 200), (63, 127, 90)):
            p[r, c] = v
        p[28:36, 60:70] = rng.integers(0, 256, size=(8, 10))
        p[60:63, 100:103] = 120
        return p
    return rng.integers(0, 41 if k % 2 else 256, size=(H, W)).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def geom_cases():
    """One buffer per order (as listed, and shuffled) holding the GEOM_SHAPES planes: plane k starts gap_k = 1..7 bytes behind the
    plane before it, gaps chosen so that the plane bases take every residue mod 4; the bytes between planes hold 0xEE."""
    rng = np.random.default_rng(6100)
    planes = [_geom_plane(H, W, k, rng) for k, (H, W) in enumerate(GEOM_SHAPES)]
    out = []
    for name, order in (("geom_listed", list(range(len(planes)))), ("geom_shuffled", [3, 5, 0, 4, 1, 2])):
        geom, off = [], 0
        gaps = []
        for k, i in enumerate(order):
            want = (1, 2, 3, 0, 1, 3)[k]                         # residue of this plane's base
            gap = next(g for g in range(1, 5) if (off + g) % 4 == want)
            gap += 4 if k % 2 and gap <= 3 else 0
            gaps.append(gap)
            off += gap
            H, W = planes[i].shape
            geom.append((H, W, off))
            off += H * W
        total = off + 5
        buf = np.full(total, 0xEE, np.uint8)
        for (H, W, o), i in zip(geom, order):
            buf[o:o + H * W] = planes[i].ravel()
        assert {o % 4 for _, _, o in geom} == {0, 1, 2, 3} and all(1 <= g <= 7 for g in gaps)
        out.append(GeomCase(name, buf, geom, [planes[i] for i in order], psets([DEFAULT, WIDE[0]])))
    return out


# ------------------------------------------------------------------ numpy mutants: wrong kernels
def live_mask(planes, R, dr, dc):
    """cells with a nonzero source pixel (reflected copies included, as the kernel's source tile holds them) within dr rows and dc columns"""
    F, H, W = planes.shape
    nz = padded(planes, R) != 0
    out = np.zeros((F, H, W), bool)
    for i in range(-dr, dr + 1):
        for j in range(-dc, dc + 1):
            out |= nz[:, R + i:R + i + H, R + j:R + j + W]
    return out


def stages_from_bilateral(bil, thresh, ge=False, zero_border=False):
    thr = thresh_tozero(bil, thresh, ge)
    return bil, thr, grey_open3x3(thr, zero_border)


def reference_bilateral(planes, p):
    return round_u8(bilateral_quotient(planes, p.d, p.sc, p.ss))


def mutant_narrow_live(planes, p, bil, rows=True, cols=True):
    """live neighbourhood one too small: a cell of bil (the right bilateral image) filters to 0 unless a nonzero pixel lies within
    R - 1 rows (rows) / R - 1 columns (cols) of it"""
    R = radius(p.d, p.ss)
    bil = np.where(live_mask(planes, R, R - 1 if rows else R, R - 1 if cols else R), bil, 0).astype(np.uint8)
    return stages_from_bilateral(bil, p.thresh)


def mutant_ring_dropped(p, bil):
    """ring columns 64..67 of every tile dropped: the cells at image columns c0 + 62 .. c0 + 65 never count as live for the tile at c0"""
    W = bil.shape[2]
    outs = [np.zeros_like(bil) for _ in range(3)]
    for c0 in range(0, W, TILE_W):
        mod = bil.copy()
        mod[:, :, c0 + TILE_W - 2:c0 + TILE_W + 2] = 0
        for o, st in zip(outs, stages_from_bilateral(mod, p.thresh)):
            o[:, :, c0:c0 + TILE_W] = st[:, :, c0:c0 + TILE_W]
    return tuple(outs)


def mutant_borders(planes, p, bil, bilateral=True, opening=True):
    """bilateral border by edge replication instead of reflect-101 (bilateral), opening with a zero border instead of edge
    replication (opening); bil: the right bilateral image, used where the bilateral border is left right"""
    if bilateral:
        bil = round_u8(bilateral_quotient(planes, p.d, p.sc, p.ss, border="replicate"))
    return stages_from_bilateral(bil, p.thresh, zero_border=opening)


def mutant_thresh_ge(p, bil):
    """v >= thresh instead of v > thresh"""
    return stages_from_bilateral(bil, p.thresh, ge=True)


def outer_tap_quotient(bil, ntaps):
    """The largest float64 quotient sum / wsum, over pixel values 1..255, of a cell whose only nonzero neighbours are ntaps pixels of
    one value at distance exactly R along its row or column (the disc holds four such taps): below 0.5 the outermost taps alone
    cannot change that many-pixel cell's rounded output, whatever the value."""
    d, sc, ss = bil
    R = radius(d, ss)
    sw = {(i, j): np.exp(-0.5 * (i * i + j * j) / (ss * ss)) for i in range(-R, R + 1) for j in range(-R, R + 1) if i * i + j * j <= R * R}
    S, wR = sum(sw.values()), sw[(0, R)]
    v = np.arange(1, 256, dtype=np.float64)
    cw = np.exp(-0.5 * v * v / (sc * sc))
    return float(np.max(ntaps * v * wR * cw / (S - ntaps * wR + ntaps * wR * cw)))
