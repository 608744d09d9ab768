"""Windows and references for the start of the IALM (csrc/swk_api.hip ialm_start: k_ialm_stats or k_gram_u8, k_ialm_init, the MODE 0
start pass, k_gram_reduce), shared by tests/test_ialm_start_cpu.py and tests/test_ialm_start_gpu.py.

A case is a batch of uint8 windows [nwin][n][P] as swk_debug_ialm_start takes them.  Everything is deterministic.  The references:

  int_ref(x)       X^T X, sum of squares and maximum of one window from integers: exact.
  float_start(x)   the reference's first iteration restated (image_filtering.py:269-284): dual_norm, mu_0, Y_0 = X / dual,
                   E_1 = shrink(X + Y_0 / mu_0, lmbda / mu_0), M_1 = X - E_1 + Y_0 / mu_0, statement by statement in float64 (or in
                   np.longdouble, for the check of the closed form M_1 = c X of a window whose first shrinkage removes nothing).
  gram_ld(m)       M^T M accumulated in np.longdouble with pairwise sums.
  expected_integer_start / start_margin   which start a window takes, and how far it lies from the switch.
"""
from collections import namedtuple

import numpy as np

LMBDA = 0.01          # image_filtering.py:256: at the sizes of this file most windows clip and take the f64 start pass
# From lmbda = 2.25 on nothing can be clipped (dual = ||X||_F, raw_max = 1.8 max(X) <= lmbda ||X||_F / 1.25): with it every
# window of every shape starts from k_gram_u8's integers, also the small ones that one, two, three or four blocks cover
LMBDA_ALL = 4.0
U = 2.0 ** -53        # unit roundoff of float64

Case = namedtuple("Case", "name x")          # x: uint8 [nwin][n][P]

P_LIST = (1, 3, 15, 16, 17, 63, 64, 65, 127, 600, 1021, 4096, 107 * 214)
N_LIST = (1, 2, 15, 16, 17, 21, 31, 32, 33, 48, 49, 63, 64)
# three more pixel counts, for the slab sums: ialm_pass_nblk gives a window of 208 / 300 / 500 pixels 2 / 3 / 4 Gram slabs under
# pass variants 2, 4 and 5 (P_LIST alone gives 1 slab up to 127 pixels and 5 or more from 600 on), which k_ialm_small's own
# gram_reduce sums; 208 is a multiple of 16
EXTRA_P = (208, 300, 500)
CONTENTS = ("one", "all255", "alt", "random", "last255", "rowend255", "tail37")
PAD_TAIL = 37          # zero pixels at the end of every frame: the padding of mixed-geometry groups (swk_batch_run_groups)


# ------------------------------------------------------------------ references
def expected_integer_start(gray, lmbda=0.01):
    """k_ialm_init's rule restated on the host: the integer start stands iff the first shrinkage (:283) removes
    nothing, i.e. max(X + Y0/mu0) = 1.8 max(X) <= lmbda/mu0 = 0.008 ||X||_F (when ||X||_F >= max(X)/lmbda)."""
    x = gray.astype(np.float64)
    fro = np.sqrt((x * x).sum())
    dual = max(fro, x.max() / lmbda)
    inv_mu = fro / 1.25
    return x.max() + inv_mu * (x.max() / dual) <= lmbda * inv_mu


def start_scalars(sumsq, maxv, lmbda=LMBDA):
    """dual_norm, mu_0, thr_0, dnorm (:269-276, :283) in float64 from the exact window statistics"""
    norm_two = np.sqrt(np.float64(int(sumsq)))          # sumsq < 2^53: exact in float64, the root correctly rounded
    norm_inf = np.float64(int(maxv)) / lmbda
    dual = max(norm_two, norm_inf)
    mu = 1.25 / norm_two
    return dual, mu, lmbda / mu, norm_two


def margin_from_stats(sumsq, maxv, lmbda=LMBDA):
    """(raw_max - thr_0) / thr_0 in float64: negative or zero = nothing is clipped, the integer start stands"""
    dual, mu, thr, _ = start_scalars(sumsq, maxv, lmbda)
    raw_max = np.float64(int(maxv)) + (1.0 / mu) * (np.float64(int(maxv)) / dual)
    return float((raw_max - thr) / thr)


def start_margin(x, lmbda=LMBDA):
    xi = x.astype(np.int64)
    return margin_from_stats(int((xi * xi).sum()), int(xi.max()), lmbda)


def int_ref(x):
    """(X^T X as int64 [n][n], sum of squares, maximum) of one window x[n][P].  The products run in float64 on purpose: every
    partial sum is an integer below 255^2 * P < 2^53, so any summation order is exact."""
    assert x.dtype == np.uint8 and x.ndim == 2 and 255 * 255 * x.shape[1] < 2 ** 53
    xf = x.astype(np.float64)
    g = (xf @ xf.T).astype(np.int64)
    return g, int(np.trace(g)), int(x.max())


def float_start(x, lmbda=LMBDA, dtype=np.float64):
    """The reference's first iteration on one window x[n][P] (frames as rows; the reference holds them as columns, which changes
    no element).  Returns dict(dual, mu, M, clipped)."""
    X = x.astype(dtype)
    lm = dtype(lmbda)
    norm_two = np.sqrt((X * X).sum())                  # :269 (integers below 2^53: the sum is exact)
    norm_inf = X.max() / lm                            # :270
    dual = max(norm_two, norm_inf)                     # :271
    Y = X / dual                                       # :272
    mu = dtype(1.25) / norm_two                        # :276
    Eraw = X + (1 / mu) * Y                            # :282 (A = 0)
    E = np.maximum(Eraw - lm / mu, 0) + np.minimum(Eraw + lm / mu, 0)          # :283
    M = X - E + (1 / mu) * Y                           # :284
    return dict(dual=dual, mu=mu, M=M, clipped=bool((E != 0).any()))


def gram_ld(m):
    """M M^T of m[n][P] in np.longdouble; every entry one pairwise sum (numpy's reduction over a contiguous axis).  Pixels that are
    zero in every frame are dropped first: they add nothing."""
    m = np.asarray(m)
    keep = (m != 0).any(axis=0)
    ml = np.ascontiguousarray(m[:, keep].astype(np.longdouble))
    n = ml.shape[0]
    g = np.zeros((n, n), np.longdouble)
    for i in range(n):
        g[i, i:] = (ml[i][None, :] * ml[i:]).sum(axis=1)
        g[i:, i] = g[i, i:]
    return g


def scale_c2(dual, mu):
    """c^2 of M_1 = c X, c = 1 + 1 / (mu_0 dual), in np.longdouble"""
    c = np.longdouble(1) + np.longdouble(1) / (np.longdouble(mu) * np.longdouble(dual))
    return c * c


_REF = {}


def window_ref(key, x, lmbda=LMBDA):
    """Everything the tests hold one window x[n][P] against, computed once per key: G int64, sumsq, maxv, integer (the start
    choice), margin, the four scalars, c2; for a window whose first shrinkage clips also Gld = M_1^T M_1 (longdouble) and
    Gabs = |M_1|^T |M_1|."""
    key = (key, lmbda)
    if key not in _REF:
        g, sumsq, maxv = int_ref(x)
        integer = bool(expected_integer_start(x, lmbda))
        dual, mu, thr, dnorm = start_scalars(sumsq, maxv, lmbda)
        r = dict(G=g, sumsq=sumsq, maxv=maxv, integer=integer, margin=margin_from_stats(sumsq, maxv, lmbda),
                 dual_norm=dual, mu_0=mu, thr_0=thr, dnorm=dnorm, c2=scale_c2(dual, mu))
        if not integer:
            fs = float_start(x, lmbda)
            r["clipped"] = fs["clipped"]
            r["Gld"] = gram_ld(fs["M"])
            a = np.abs(fs["M"])
            r["Gabs"] = a @ a.T
        _REF[key] = r
    return _REF[key]


# ------------------------------------------------------------------ window contents
def fill(content, n, P, seed):
    """One window [n][P] of the named content; none is all zero (such a window is done before it starts)."""
    rng = np.random.default_rng(seed)
    x = np.zeros((n, P), np.uint8)
    if content == "one":                      # all 0 except one pixel of value 1
        x[n // 2, P // 2] = 1
    elif content == "all255":                 # the largest biased operand (+127) everywhere
        x[:] = 255
    elif content == "alt":                    # frames 255, 0, 255, ...: both extreme operands (-128 for 0)
        x[0::2] = 255
    elif content == "random":
        x[:] = rng.integers(0, 256, size=(n, P), dtype=np.uint8)
    elif content == "last255":                # the window's very last pixel
        x[n - 1, P - 1] = 255
    elif content == "rowend255":              # the last pixel of every frame: a row tail that runs into the next frame
        x[:, P - 1] = 255
    elif content == "tail37":                 # random, the trailing 37 pixels of every frame zero (all but the first pixel where
        x[:] = rng.integers(1, 256, size=(n, P), dtype=np.uint8)          # the frame is no longer than that)
        x[:, max(P - PAD_TAIL, 1):] = 0
    else:
        raise ValueError(content)
    return x


# ------------------------------------------------------------------ shapes
def _covering_shapes():
    """(n, P, nwin): every P with 21 and 64 frames, every n with a P that is a multiple of 16 (one 16-byte load per lane) and one
    that is not (five dwords and a byte shift); batches of 3 and 4 windows of an odd number of bytes, so that windows start at
    byte offsets 0..3 of the batch; the largest batch is 3 windows of 64 x 22,898."""
    shapes = []
    for P in P_LIST:
        shapes.append((21, P, 4 if P % 2 else 1))          # 21 P odd: windows at byte offsets 0, 1, 2, 3 (or 0, 3, 2, 1)
        shapes.append((64, P, 3 if P == P_LIST[-1] else 1))
    for P in EXTRA_P:
        shapes += [(21, P, 1), (64, P, 1)]
    aligned, unaligned, unaligned_even_n = (16, 64, 4096), (17, 63, 65, 127, 1021), (600, 63, 1021)
    k = 0
    for n in N_LIST:
        if n in (21, 64):
            continue
        odd = n % 2 == 1
        shapes.append((n, aligned[k % 3], 3 if k % 2 else 1))
        pu = unaligned[k % 5] if odd else unaligned_even_n[k % 3]
        shapes.append((n, pu, 4 if odd and pu % 2 else 1))
        k += 1
    return tuple(shapes)


SHAPES = _covering_shapes()


def shape_id(shape):
    return "n%d_P%d_w%d" % shape


_X = {}


def shape_cases(shape):
    """The cases of one shape: one batch per content; window w of the batch for content c holds content c + w, so every batch of
    several windows also puts different contents next to each other."""
    if shape not in _X:
        n, P, nwin = shape
        out = []
        for ci, content in enumerate(CONTENTS):
            x = np.stack([fill(CONTENTS[(ci + w) % len(CONTENTS)], n, P, seed=1000 * ci + 17 * w + n + P) for w in range(nwin)])
            out.append(Case("%s_%s" % (shape_id(shape), content), x))
        _X[shape] = out
    return _X[shape]


# ------------------------------------------------------------------ neighbours
NEIGHBOUR_SHAPES = ((21, 17), (21, 600), (21, 107 * 214), (64, 65), (64, 1021), (33, 127), (16, 4096), (48, 64))


def neighbour_cases(n, P):
    """A random window next to an all-255 window, both orders: what a window reading a pixel of its neighbour would show most."""
    rnd, full = fill("random", n, P, seed=7 + n + P), fill("all255", n, P, seed=0)
    sid = "n%d_P%d" % (n, P)
    return [Case("nb_%s_random_255" % sid, np.stack([rnd, full])), Case("nb_%s_255_random" % sid, np.stack([full, rnd]))]


# ------------------------------------------------------------------ windows near the switch between the two starts
# A constant image of value v has max = v and ||X||_F = v sqrt(nP): raw_max = 1.8 v against thr_0 = 0.008 v sqrt(nP), so the switch
# lies at nP = 225^2 = 50,625 whatever v.  nP = 50,625 itself (15 x 3375) is an exact tie, decided by rounding: not a case.  The
# closest sizes on either side with n in N_LIST are nP = 50,624 and 50,626; the issue's example 21 x 2410 / 21 x 2411 rides along.
# With one pixel raised from v = 254 to 255 the maximum and the norm no longer move together (raw_max = 1.8 * 255, thr_0 =
# 0.008 sqrt(254^2 (nP - 1) + 255^2)): the switch moves to nP = 51,024.4, closest sizes 51,024 and 51,025 (= 25 x 2041: the one
# frame count of this file outside N_LIST).
# (n, P, v, raised, integer start?) and the margin (raw_max - thr_0) / thr_0 of the float64 restatement (start_margin):
BOUNDARY = (
    (64, 791, 255, False, False),          # nP = 50,624   margin +9.877e-06
    (34, 1489, 255, False, True),          # nP = 50,626   margin -9.876e-06
    (21, 2410, 100, False, False),         # nP = 50,610   margin +1.482e-04
    (21, 2411, 100, False, True),          # nP = 50,631   margin -5.925e-05
    (48, 1063, 254, True, False),          # nP = 51,024   margin +3.908e-06
    (25, 2041, 254, True, True),           # nP = 51,025   margin -5.891e-06
)
MIN_MARGIN = 1e-9          # no rounding of a square root or a division moves raw_max / thr_0 by more than a few 1e-16


def boundary_window(n, P, v, raised):
    x = np.full((n, P), v, np.uint8)
    if raised:
        x[n // 3, P // 3] = 255
    return x


def closest_boundary_sizes(v, raised, n_list=tuple(range(1, 65)), span=60):
    """The totals nP closest to the switch on either side -- (clipped side, integer side) -- among those with a margin of at least
    MIN_MARGIN and a factorisation n x P, n in n_list; from the closed-form statistics of boundary_window."""
    best = {}
    centre = 50625 if not raised else 51024
    for t in range(centre - span, centre + span + 1):
        if not any(t % n == 0 for n in n_list):
            continue
        sumsq = v * v * t + ((255 * 255 - v * v) if raised else 0)
        m = margin_from_stats(sumsq, 255 if raised else v)
        if abs(m) < MIN_MARGIN:
            continue
        side = m <= 0
        if side not in best or abs(m) < abs(best[side][1]):
            best[side] = (t, m)
    return best[False][0], best[True][0]


def boundary_cases():
    return [Case("boundary_n%d_P%d_v%d%s" % (n, P, v, "_raised" if raised else ""), boundary_window(n, P, v, raised)[None])
            for n, P, v, raised, _ in BOUNDARY]


# ------------------------------------------------------------------ windows whose first shrinkage clips
def toy_window():
    """The toy window of test_integer_start_matches_f64_start (tests/test_gpu_parity.py), in grey: 7 frames of 16 x 16"""
    from oracle import reference_path as orc
    from swiftwatcher_amd import synthetic
    roi = synthetic.roi_window(7, 7, 16, 16, birds=1, bird_len=(4, 6), bird_wid=(2, 3))
    return np.stack([orc.bgr2gray(f) for f in roi]).reshape(7, 256)


def dark_window(n=21, P=1021, seed=5):
    """Night sky, one saturated pixel"""
    x = np.random.default_rng(seed).integers(0, 16, size=(n, P), dtype=np.uint8)
    x[n // 2, P // 2] = 255
    return x


def clipped_cases():
    """name, batch, per window: does its first shrinkage clip?  The mixed batch puts a clipped window between two integer ones."""
    n, P = 21, 107 * 214
    mixed = np.stack([fill("random", n, P, seed=41), dark_window(n, P, seed=42), fill("all255", n, P, seed=0)])
    return [(Case("clipped_toy", toy_window()[None]), (True,)),
            (Case("clipped_dark", dark_window()[None]), (True,)),
            (Case("clipped_mixed", mixed), (False, True, False))]
