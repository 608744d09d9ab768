"""Windows and the 256-bit reference for the first step of the IALM (csrc/swk_api.hip ialm_first_step: the small-matrix step of
k = 0 -- k_ialm_small or k_ialm_small_wide -- and k_ialm_refine_start), shared by tests/test_ialm_first_step_cpu.py and
tests/test_ialm_first_step_gpu.py.

A window is x[n][P] uint8 (frames as rows) and enters the library as pixels, through the chain's own start.  The first iteration
computes A_1 = M_1 B_1 (M_1 pixels x frames) with

    B_1 = I - K^(-1/2) / (c_1 mu_0),    K = X^T X and c_1 = 1 + 1 / (mu_0 dual)   where the window starts on the integer cores,
                                        K = M_1^T M_1 of the float64 M_1, c_1 = 1  where it runs the f64 start pass,

M_1, mu_0 and dual as tests/ialm_start_cases.py restates them from image_filtering.py:269-284.  The reference forms K exactly (Python
integers) and K^(-1/2) in fixed point with 256 fractional bits by the coupled Newton-Schulz iteration, and proves itself:
max |I - W K W| < 2^-150 and W = W^T, in the same arithmetic.

The metric is the error of A_1 in grey levels,

    err(B) = max over pixels and frames of |M_1 (B - B_exact)|,

with B - B_exact formed in fixed point, rounded once to float64 and multiplied by the float64 M_1.  B is taken as the pass kernels
read it (csrc/ialm.hip, ialm_mfma.hip, ialm_mstate.hip: A[p][i] = sum_j M[p][j] Bm[j * n + i]), so with x[n][P] the product is
B^T M_1: a transposed read of the refined, unsymmetric B shows.

The two bound shapes (eps = 2^-53, cond = sigma_max / sigma_min of M_1 from the float64 SVD):

    standard route   err <= 8 C_GRAM eps cond^2 / mu_0      refined route   err <= 8 C_REF eps cond / mu_0

C_GRAM and C_REF are the largest constants of two float64 stand-ins over every case of this file -- numpy.linalg.eigh of K for the
Gram route, numpy.linalg.svd of M_1 (V S^-1 V^T) for the refined one -- measured on the CPU (tests/test_ialm_first_step_cpu.py holds
them; the per-case table is in DESIGN.md section 2)."""
import functools
from collections import namedtuple

import numpy as np

from ialm_start_cases import LMBDA, LMBDA_ALL, float_start, int_ref

EPS = 2.0 ** -53
FRAC = 256                       # fractional bits of the fixed-point reference
ONE = 1 << FRAC
M_SHIFT = 60                     # M_1 2^60 is an integer for every window of this file (asserted)

# Largest constants of the float64 stand-ins over CASES, rounded up to two digits (measured 2026-10-19 with numpy's bundled LAPACK; the
# per-case table is in DESIGN.md section 2): 0.5745 at square_n3_P4 and 1.0974 at frames_n15_P4933_clip -- typical values are 0.03 .. 0.2
C_GRAM = 0.58
C_REF = 1.1

Case = namedtuple("Case", "name n P sigma seed lmbda integer kind")
# kind: "plain", "null" (frame n // 2 all zero), "dup" (the last frame repeated: io_video.py:51-53)


# ------------------------------------------------------------------ scenes
def scene(n, P, sigma, seed):
    """One static random sky, 100..220 per pixel, plus Gaussian noise, rounded to uint8: x[n][P]"""
    rng = np.random.default_rng(seed)
    sky = rng.uniform(100.0, 220.0, size=P)
    return np.clip(np.rint(sky[None, :] + sigma * rng.standard_normal((n, P))), 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def window(case):
    x = scene(case.n, case.P, case.sigma, case.seed)
    if case.kind == "null":
        x[case.n // 2] = 0
    elif case.kind == "dup":
        x[case.n - 1] = x[case.n - 2]
    x.setflags(write=False)
    return x


# ------------------------------------------------------------------ exact integers
def _exact_int(m, shift=M_SHIFT):
    """m 2^shift as Python integers (object array), from float.as_integer_ratio: nothing is rounded"""
    out = np.empty(m.shape, object)
    flat = out.reshape(-1)
    for i, v in enumerate(np.asarray(m, np.float64).reshape(-1)):
        num, den = float(v).as_integer_ratio()
        q, r = divmod(num << shift, den)
        assert r == 0, "M_1 has bits below 2^-%d" % shift
        flat[i] = q
    return out


def gram_exact(m, shift=M_SHIFT):
    """(m m^T) 2^(2 shift) of the float64 m[n][P] as Python integers, exactly.  m 2^shift (integers below 2^72, asserted) is cut
    into six limbs of 12 bits; a product of limbs is below 2^24 and a sum of up to 2^20 of them below 2^53, so every limb-pair Gram
    matrix is exact in a float64 matrix product, whatever its summation order."""
    m = np.asarray(m, np.float64)
    n, P = m.shape
    assert np.all(m >= 0) and m.max() < 2.0 ** (72 - shift) and P <= 2 ** 20
    g = np.zeros((6, 6, n, n), np.float64)
    for p0 in range(0, P, 16384):
        q = m[:, p0:p0 + 16384] * 2.0 ** shift                 # a power of two: exact
        assert np.array_equal(q, np.floor(q)), "M_1 has bits below 2^-%d" % shift
        limbs = [None] * 6
        for l in range(5, -1, -1):                             # from the top: floor, scaling and subtraction are all exact
            limbs[l] = np.floor(q * 2.0 ** (-12 * l))
            q = q - limbs[l] * 2.0 ** (12 * l)
        assert not q.any() and all(lb.max() < 4096.0 for lb in limbs)
        for a in range(6):
            for b in range(a, 6):
                g[a, b] += limbs[a] @ limbs[b].T
    assert g.max() < 2.0 ** 53
    k = np.zeros((n, n), object)
    for a in range(6):
        for b in range(a, 6):
            gi = g[a, b].astype(np.int64).astype(object)
            k = k + ((gi + gi.T if b > a else gi) << (12 * (a + b)))
    return k


# ------------------------------------------------------------------ K^(-1/2) in 256-bit fixed point
def _limbs16(x):
    """x (Python integers) as signed 16-bit limbs in float64, least significant first: [limb][row][column]"""
    flat = [int(v) for v in x.reshape(-1)]
    nbytes = max(2, (max(abs(v) for v in flat).bit_length() + 15) // 16 * 2)
    u = np.frombuffer(b"".join(abs(v).to_bytes(nbytes, "little") for v in flat), dtype="<u2").reshape(x.shape + (nbytes // 2,))
    sign = np.array([(v > 0) - (v < 0) for v in flat], np.float64).reshape(x.shape)
    return np.ascontiguousarray(np.moveaxis(u.astype(np.float64) * sign[..., None], -1, 0))


def int_matmul(a, b):
    """The exact product of two matrices of Python integers -- what numpy's object product a @ b gives (the host test compares them),
    7 times faster at 128 frames.  Both are cut into signed 16-bit limbs; every limb-pair product is one float64 matrix product whose
    entries stay below m 2^32, and those that share a weight 2^(16 d) sum to less than 2^46 (asserted): exact, in any order.  The
    sums go back to Python integers and are shifted into place."""
    n, m = a.shape
    p = b.shape[1]
    la, lb = _limbs16(a), _limbs16(b)
    assert m * 65535.0 ** 2 * min(len(la), len(lb)) < 2.0 ** 46
    nd = len(la) + len(lb) - 1
    prod = (la.reshape(-1, m) @ lb.transpose(1, 0, 2).reshape(m, -1)).reshape(len(la), n, len(lb), p)
    D = np.zeros((nd + 1, n, p), np.float64)
    for i in range(len(la)):
        for j in range(len(lb)):
            D[i + j] += prod[i, :, j, :]
    Di = D.astype(np.int64)
    out = np.zeros((n, p), object)
    for d in range(0, nd, 2):          # two neighbouring weights at a time: below 2^46 + 2^62 in int64
        out = out + ((Di[d] + (Di[d + 1] << 16)).astype(object) << (16 * d))
    return out


def _mm(a, b):
    return int_matmul(a, b) >> FRAC          # floor of the exact product: an error below 2^-256 per entry


def _eye(n):
    e = np.zeros((n, n), object)
    for i in range(n):
        e[i, i] = ONE
    return e


def invsqrt_fixed(k_int, kshift):
    """W = K^(-1/2) in fixed point (FRAC bits), K = k_int / 2^kshift a symmetric positive definite matrix of Python integers:
    coupled Newton-Schulz  Y_0 = K / 2^s, Z_0 = I;  T = (3 I - Z Y) / 2;  Y <- Y T, Z <- T Z  until max |I - Z Y| < 2^-200, then
    W = Z / 2^(s / 2).  Returns (W, steps, self-proof residual max |I - W K W| as a float)."""
    n = k_int.shape[0]
    trace = sum(int(k_int[i, i]) for i in range(n))
    s = trace.bit_length() - kshift                          # 2^s > trace K >= lambda_max
    s += s & 1                                               # even: W = Z 2^(-s/2)
    sh = FRAC - kshift - s
    y = np.array([[int(v) << sh if sh >= 0 else int(v) >> -sh for v in row] for row in k_int], object)
    assert sh >= 0, "K does not fit the fixed-point format exactly"
    z = _eye(n)
    eye = _eye(n)
    steps = 0
    while True:
        zy = _mm(z, y)
        res = max(abs(int(v)) for v in (eye - zy).reshape(-1))
        if res < (1 << (FRAC - 200)):
            break
        assert steps < 80, "the reference's Newton-Schulz iteration did not converge"
        t = (3 * eye - zy) >> 1
        y, z = _mm(y, t), _mm(t, z)
        steps += 1
    w = z >> (s // 2)
    # the proof, in the same arithmetic: W K W = I and W = W^T
    wkw = int_matmul(int_matmul(w, k_int), w) >> (FRAC + kshift)
    proof = max(abs(int(v)) for v in (eye - wkw).reshape(-1))
    asym = max(abs(int(v)) for v in (w - w.T).reshape(-1))
    assert proof < (1 << (FRAC - 150)), "reference: max |I - W K W| = 2^%d" % (proof.bit_length() - FRAC)
    assert asym < (1 << (FRAC - 150)), "reference: max |W - W^T| = 2^%d" % (asym.bit_length() - FRAC)
    return w, steps, max(proof, asym) / float(ONE)


def to_fixed(a):
    """a float64 array as fixed-point integers, exactly"""
    return _exact_int(a, FRAC)


Ref = namedtuple("Ref", "x M K kshift W B c1 inv_mu mu dual integer clipped cond smax smin steps proof live")


def _start(x, lmbda, integer):
    fs = float_start(x, lmbda)
    mu, dual = float(fs["mu"]), float(fs["dual"])
    inv_mu = 1.0 / mu
    c1 = 1.0 + inv_mu / dual if integer else 1.0             # k_ialm_refine_start's and gram_reduce's float64 number
    return fs, mu, dual, inv_mu, c1


def _b_exact(w, c1, inv_mu):
    """I - W inv_mu / c1 in fixed point; c1 and inv_mu are float64 numbers, taken exactly"""
    n = w.shape[0]
    an, ad = float(inv_mu).as_integer_ratio()
    cn, cd = float(c1).as_integer_ratio()
    return _eye(n) - (w * (an * cd)) // (ad * cn)


@functools.lru_cache(maxsize=None)
def reference(case):
    """The 256-bit reference of one case (a few seconds at 64 frames; cached for the session)"""
    x = window(case)
    n = case.n
    fs, mu, dual, inv_mu, c1 = _start(x, case.lmbda, case.integer)
    M = np.ascontiguousarray(fs["M"])
    live = np.array([bool(x[i].any()) for i in range(n)])
    if case.integer:
        assert not fs["clipped"], "%s: an integer start needs a window whose first shrinkage removes nothing" % case.name
        k_int, kshift = int_ref(x)[0].astype(object), 0
    else:
        k_int, kshift = gram_exact(M), 2 * M_SHIFT
    sv = np.linalg.svd(M[live], compute_uv=False)
    if case.kind == "dup":
        # rank deficient by construction: no inverse square root.  The tests hold such a window to the float64 statement of the
        # project's definition (definition_f64) with the conditioning of its live part
        sv = sv[:-1]
        w = steps = proof = B = None
    else:
        idx = np.flatnonzero(live)
        wl, steps, proof = invsqrt_fixed(k_int[np.ix_(idx, idx)], kshift)
        w = np.zeros((n, n), object)          # a null frame: weight 0, embedded with a zero row and column
        w[np.ix_(idx, idx)] = wl
        B = _b_exact(w, c1, inv_mu)
    return Ref(x=x, M=M, K=k_int, kshift=kshift, W=w, B=B, c1=c1, inv_mu=inv_mu, mu=mu, dual=dual, integer=case.integer,
               clipped=bool(fs["clipped"]), cond=float(sv[0] / sv[-1]), smax=float(sv[0]), smin=float(sv[-1]), steps=steps,
               proof=proof, live=live)


def k_float(ref):
    """K rounded to float64 (the stand-ins' input)"""
    scale = 2.0 ** -ref.kshift
    return np.array([[float(int(v)) * scale for v in row] for row in ref.K], np.float64)


# ------------------------------------------------------------------ the metric and the bounds
def err_vs(B, B_exact_fixed, M):
    """max |M_1 (B - B_exact)| in grey levels: the difference in fixed point, rounded once to float64, times the float64 M_1[n][P]"""
    d_fixed = to_fixed(np.asarray(B, np.float64)) - B_exact_fixed
    d = np.array([[int(v) / ONE for v in row] for row in d_fixed], np.float64)
    return float(np.abs(d.T @ M).max())


def err(B, ref):
    return err_vs(B, ref.B, ref.M)


def bound_std(ref):
    return 8.0 * C_GRAM * EPS * ref.cond ** 2 * ref.inv_mu


def bound_ref(ref):
    return 8.0 * C_REF * EPS * ref.cond * ref.inv_mu


# ------------------------------------------------------------------ float64 stand-ins and the project's definition
def standin_eigh(ref):
    """The Gram route in float64 LAPACK: B from numpy.linalg.eigh of K"""
    lam, v = np.linalg.eigh(k_float(ref))
    w = (v * lam ** -0.5) @ v.T
    return np.eye(len(lam)) - w * (ref.inv_mu / ref.c1)


def standin_svd_parts(ref):
    """The refined route in float64 LAPACK: the SVD of the window itself -- of X where it starts on the integer cores (M_1 = c_1 X),
    of the float64 M_1 otherwise; returns (V, S) with K = V S^2 V^T"""
    a = ref.x.astype(np.float64) if ref.integer else ref.M
    _, s, vt = np.linalg.svd(a.T, full_matrices=False)
    return vt.T, s


def standin_svd(ref):
    v, s = standin_svd_parts(ref)
    return np.eye(len(s)) - ((v / s) @ v.T) * (ref.inv_mu / ref.c1)


def cholesky_fixed(k_int, kshift):
    """The lower Cholesky factor of K = k_int / 2^kshift in fixed point (FRAC bits: what the kernel's double-double factor approximates),
    rounded once to float64"""
    import math
    n = k_int.shape[0]
    a = [[int(k_int[i, j]) << (FRAC - kshift) for j in range(n)] for i in range(n)]
    L = [[0] * n for _ in range(n)]
    for j in range(n):
        d = a[j][j] - (sum(v * v for v in L[j][:j]) >> FRAC)
        assert d > 0
        L[j][j] = math.isqrt(d << FRAC)
        for i in range(j + 1, n):
            L[i][j] = ((a[i][j] - (sum(x * y for x, y in zip(L[i][:j], L[j][:j])) >> FRAC)) << FRAC) // L[j][j]
    return np.array([[v / ONE for v in row] for row in L], np.float64)


def standin_refine_route(ref):
    """k_ialm_refine_start's own route restated in float64 (csrc/ialm_refine.hip): K = L L^T with L rounded to float64; R^-1 = (L^-1)^T
    by forward substitution, one column of L^-1 at a time; U = polar(R) by the coupled Newton-Schulz iteration from Y_0 = R / s,
    Z_0 = Y_0^T with the kernel's SCALED steps (T = a I - c Z Y while the tracked bound is below 1) and its stopping rule; W = R^-1 U
    used as the product, NOT symmetrised.  Returns (B, B with W transposed).  The scaled steps leave U with an unstructured forward
    error of eps cond: through R^-1 U it meets the orthonormal Q of M_1 = Q R, through its transpose it meets R and costs eps cond^2."""
    n = ref.K.shape[0]
    L = cholesky_fixed(ref.K, ref.kshift)
    X = np.zeros((n, n))                                  # column c solves L x = e_c
    for c in range(n):
        X[c, c] = 1.0 / L[c, c]
        for r in range(c + 1, n):
            X[r, c] = -(L[r, c:r] @ X[c:r, c]) / L[r, r]
    Ri = X.T
    s = np.sqrt((L * L).sum()) * (1.0 + 1e-12)           # ||R||_F = sqrt(trace K)
    Z, Y, eye = L / s, L.T / s, np.eye(n)
    lo = 0.999 / (np.sqrt((Ri * Ri).sum()) * s)
    prev, plain, final = 1e300, False, False
    for _ in range(100):
        plain = plain or prev < 0.25
        unit = plain or not lo < 0.9999
        P = Z @ Y
        E = eye - P
        if unit:
            T = eye + 0.5 * E
        else:
            alpha = np.sqrt(3.0 / (1.0 + lo + lo * lo))
            ta, tc = 1.5 * alpha, 0.5 * alpha ** 3
            lo = lo * (ta - tc * lo * lo)
            T = ta * eye - tc * P
        Y, Z = Y @ T, T @ Z
        prev = float((E * E).sum())
        if final:
            break
        final = prev < 1e-8 and unit
    else:
        raise AssertionError("the stand-in's Newton-Schulz iteration did not converge")
    w = Ri @ Y
    return eye - w * (ref.inv_mu / ref.c1), eye - w.T * (ref.inv_mu / ref.c1)


def definition_f64(ref):
    """The project's definition for rank-deficient windows, stated in float64: eigen-directions of G_1 below
    1e-13 lambda_max carry weight 0"""
    lam, v = np.linalg.eigh(k_float(ref))
    wgt = np.where(lam > 1e-13 * lam.max(), 1.0, 0.0) / np.sqrt(np.where(lam > 1e-13 * lam.max(), lam, 1.0))
    return np.eye(len(lam)) - ((v * wgt) @ v.T) * (ref.inv_mu / ref.c1)


def cond_estimate(ref):
    """(cond_sum, estimate) of note_conditioning from float64 eigvalsh of G_1 = c_1^2 K: ||G_1||_F sum 1 / lambda_i over the live
    directions, and 1.1e-16 cond_sum / mu_0.  eigvalsh leaves every eigenvalue with an absolute error of a few eps lambda_max, so the
    sum of reciprocals is good to about n eps cond(K): below 1e-7 for cond(K) <= 1e7, which the caller asserts."""
    g = k_float(ref) * ref.c1 ** 2
    lam = np.linalg.eigvalsh(g)
    lam = lam[lam > 1e-13 * lam.max()]
    cond_sum = float(np.sqrt((lam * lam).sum()) * (1.0 / lam).sum())
    return cond_sum, 1.1e-16 * cond_sum * ref.inv_mu, float(lam.max() / lam.min())


# ------------------------------------------------------------------ the case list
FRAMES = (1, 2, 3, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64)          # four block counts, three layouts, the switch at 48
WIDE_FRAMES = (65, 100, 128)


def pixels_for(n):
    """A pixel count for n frames: at least 2 n and 100, no multiple of 16 (so of no 16 NB: the last chunk of the double-double Gram
    matrix from the pixels is partial at every width)"""
    P = max(2 * n, 100) + 7 * n + 5
    while P % 16 == 0:
        P += 1
    return P


def clip_pixels(n):
    """A pixel count at which the first shrinkage of a 100..220 sky clips SOME pixels at lmbda = 0.01.  A pixel is clipped when
    1.8 x > lmbda / mu_0 = 0.008 ||X||_F, i.e. x > 0.73 sqrt(n P) for a sky of rms 165, and a clipped pixel becomes the constant
    lmbda / mu_0 in M_1: below n P = 18,600 every pixel clips and M_1 is a constant matrix (rank one -- no window for this test), above
    90,000 none does.  n P = 74,000 puts the limit at 200; capped at 37,000 pixels (limit 141 for one frame)."""
    P = min(74000 // n, 37000)
    while P % 16 == 0:
        P += 1
    return P


def _seed(n, P, tag):
    return 100000 * tag + 1000 * (n % 97) + P % 991


def _mk(name, n, P, sigma, tag, start, kind="plain"):
    lmbda, integer = {"int": (LMBDA_ALL, True), "f64": (LMBDA_ALL, False), "clip": (LMBDA, False)}[start]
    return Case("%s_n%d_P%d_s%g_%s" % (name, n, P, sigma, start), n, P, sigma, _seed(n, P, tag), lmbda, integer, kind)


STARTS = ("int", "f64", "clip")
# every frame count at sigma = 0.6 (cond about 2500 from 15 frames on), from each of the three starts
FRAME_CASES = {(n, st): _mk("frames", n, clip_pixels(n) if st == "clip" else pixels_for(n), 0.6, 1, st) for n in FRAMES for st in STARTS}
# the from-pixels route at P = n + 1 (below 16 frames one partial chunk and nothing else); from the f64 start at lmbda = 4, since at
# lmbda = 0.01 so small a window is clipped to a constant (clip_pixels); sigma = 8 keeps a nearly square window regular
SQUARE_CASES = {n: _mk("square", n, n + 1, 8.0, 2, "f64") for n in (3, 17, 33)}
# well-conditioned windows, and the other noise levels
SIGMA_CASES = {(n, sg): _mk("sigma", n, P, sg, 3, "int") for n, P, sg in ((21, 300, 8.0), (33, 500, 8.0), (21, 300, 2.0), (17, 200, 0.3))}
# the two scenes of the issue's table that the frame counts do not reach
TABLE_CASES = {(n, P): _mk("table", n, P, 0.6, 4, st) for n, P, st in ((64, 744, "clip"), (64, 4418, "int"))}
# give-ups: a null frame and a repeated last frame, from the integer start and from the pixels
GIVEUP_CASES = {(kind, st): _mk(kind, 21, clip_pixels(21) if st == "clip" else 300, 8.0, 5, st, kind)
                for kind in ("null", "dup") for st in ("int", "clip")}
# long windows (k_ialm_small_wide); variant 6 never takes the integer start
WIDE_CASES = {n: _mk("wide", n, 2 * n + 45, 8.0, 6, "f64") for n in WIDE_FRAMES}
# the work cap of the from-pixels route: 64 frames from the f64 start are 2080 pairs = 3 rounds per pixel
CAP_UNDER = _mk("cap", 64, 133333, 2.0, 7, "f64")
CAP_OVER = _mk("cap", 64, 133334, 2.0, 7, "f64")

# one call of five windows: refined, unflagged, null frame, repeated frame, refined -- from the integer start, and from the pixels
BATCH_CASES = {st: [_mk("batch%d" % i, 21, clip_pixels(21) if st == "clip" else 300, sg, 8 + i, st, kind)
                    for i, (sg, kind) in enumerate(((0.6, "plain"), (8.0, "plain"), (0.6, "null"), (0.6, "dup"), (0.6, "plain")))]
               for st in ("int", "clip")}
# the flag and its estimate: one window per start and block count
FLAG_CASES = [FRAME_CASES[(17, "int")], FRAME_CASES[(33, "f64")], FRAME_CASES[(48, "clip")], FRAME_CASES[(64, "int")],
              SIGMA_CASES[(21, 8.0)]]

# the full-rank windows: the stand-ins' constants are maxima over these
CASES = (list(FRAME_CASES.values()) + list(SQUARE_CASES.values()) + list(SIGMA_CASES.values()) + list(TABLE_CASES.values())
         + list(WIDE_CASES.values()) + [CAP_UNDER])
# ... and the windows with a null frame, whose reference is that of the remaining frames
PROOF_CASES = CASES + [c for c in GIVEUP_CASES.values() if c.kind == "null"]
# Where the refinement decides the accuracy: the Gram route in float64 (LAPACK's eigh, whose constant is as low as 0.03 on these windows)
# misses the refined tolerance 8 C_REF eps cond / mu_0 tenfold once C cond >= 80 C_REF -- measured on every sigma = 0.6 window from 47
# frames on (cond 2250 .. 3030) and on the 744-pixel scene (cond 4370), 14 to 36 times; tests/test_ialm_first_step_cpu.py holds it
ILL_CONDITIONED = [c for (n, st), c in FRAME_CASES.items() if n >= 47] + [TABLE_CASES[(64, 744)]]


def case_id(case):
    return case.name
