"""Windows and float64 trajectories of the inexact-ALM decomposition, shared by tests/test_ialm_trajectory_cpu.py and
tests/test_ialm_trajectory_gpu.py.

The library can be stopped after exactly k iterations (maxiter = k), so every iterate of a window is the result of a full, legal run.
The reference here is the loop of oracle.reference_path.ialm_defined restated with its iterates kept:

    trajectory(X)        the SVD route (image_filtering.py:282-297 with the DEAD_EIG rule and exact zeros for null frames):
                         [(A_k, E_k, ratio_k)] for k = 1..K, ratio_k = ||Z_k||_F / ||X||_F, K the iteration that stops by tol
    gram_trajectory(X)   the same loop on the Gram route in float64 -- numpy.linalg.eigh of M^T M, B = P - W / mu, A = M B --
                         the CPU stand-in for what the kernels do: what it loses against the SVD route is the price of the route

X is (pixels, frames) like the oracle's; the library takes the transpose (frames as rows of uint8 pixels).

boundary_mask(E, band) marks the elements whose sparse-image byte trunc(clip(-E, 0, 255)) can change under a perturbation of E below
band: those where -E lies within band of an integer 1..255."""
import functools
from collections import namedtuple

import numpy as np

from oracle import reference_path as orc
from oracle.reference_path import DEAD_EIG

ATOL_AE = 1e-5          # BASELINE.json north_star: A and E within 1e-5 of the reference -- here at every k
ATOL_STANDIN = 1e-6     # the float64 Gram route against the SVD route, every k of every case (measured: 1.7e-7 at most)
# The two copies of a duplicated frame share one decomposition, but no route keeps them equal to the bit: their columns of G^(-1/2) are
# rounded separately (the oracle's own copies differ by up to 1.4e-11 through LAPACK's SVD, the float64 Gram route's by 1e-8).  What
# separates them is rounding of the Gram route and nothing else, so they are held to the bound of that rounding, ATOL_STANDIN --
# twenty times closer to each other than two results within ATOL_AE of the reference have to be.
ATOL_COPIES = ATOL_STANDIN
BAND = 1e-5             # boundary_mask's band: the bound on E
MASK_CAP = 2e-4         # largest share of a window's elements the mask may cover
RATIO_MARGIN = 1e-2     # |ratio_k / tol - 1| of every stopping test: ten guard bands (1e-3) away from deciding

Iterate = namedtuple("Iterate", "A E ratio")


# ------------------------------------------------------------------ the two routes
def _low_rank_svd(M, inv_mu):
    U, S, Vt = np.linalg.svd(M, full_matrices=False)                                  # :284
    w = np.where(S * S > DEAD_EIG * S[0] * S[0], S - inv_mu, 0.0)                     # :285-290 with the zero-direction rule
    return np.dot(U * w, Vt)


def _low_rank_gram(M, inv_mu):
    """A = M B, B = P - W / mu: P the projector on the live eigen-directions of G = M^T M, W = G^(-1/2) on them"""
    lam, V = np.linalg.eigh(M.T @ M)
    live = lam > DEAD_EIG * lam.max()
    Vl = V[:, live]
    B = Vl @ Vl.T - (Vl / np.sqrt(lam[live])) @ Vl.T * inv_mu
    return M @ B


def _loop(X, low_rank, lmbda, tol, maxiter, mu_late_at=None, keep_dead_weight=False):
    """ialm_defined's loop with every iterate kept.  The two mutations serve the sensitivity test only: mu_late_at = k applies the
    growth of mu one iteration late at iteration k (iteration k + 1 runs on mu_k once more, the one after on 2.25 mu_k);
    keep_dead_weight gives dead directions the reference's weight -1/mu from iteration 2 on."""
    Xf = np.asarray(X, np.float64)
    flat = Xf.ravel()
    two_norm = np.linalg.norm(flat, 2)                        # :269
    inf_norm = np.linalg.norm(flat, np.inf) / lmbda           # :270
    Y = Xf / max(two_norm, inf_norm)                          # :271-272
    A = np.zeros(Xf.shape)
    x_fro = np.linalg.norm(Xf, 'fro')                         # :275
    mu = 1.25 / two_norm                                      # :276
    null_cols = ~Xf.any(axis=0)
    out = []
    k = 0
    while True:
        raw = Xf - A + (1 / mu) * Y                                                  # :282
        E = np.maximum(raw - lmbda / mu, 0) + np.minimum(raw + lmbda / mu, 0)        # :283
        M = Xf - E + (1 / mu) * Y
        A = low_rank(M, 1 / mu)
        if keep_dead_weight and k >= 1:
            A = A + _dead_term(M, 1 / mu)
        A[:, null_cols] = 0.0
        Z = Xf - A - E                                        # :293
        Y = Y + mu * Z                                        # :294
        k += 1
        if mu_late_at is None or k != mu_late_at:
            mu = mu * 1.5 * (1.5 if mu_late_at is not None and k == mu_late_at + 1 else 1.0)     # :295
        ratio = np.linalg.norm(Z, 'fro') / x_fro
        out.append(Iterate(A, E, float(ratio)))
        if ratio < tol or k >= maxiter:                       # :297
            break
    return out


def _dead_term(M, inv_mu):
    """What the reference's always-full svp adds for every dead direction: -(1/mu) u v^T, u the unit left vector LAPACK happens to
    return for the zero singular value"""
    U, S, Vt = np.linalg.svd(M, full_matrices=False)
    dead = ~(S * S > DEAD_EIG * S[0] * S[0])
    return -inv_mu * np.dot(U[:, dead], Vt[dead])


def trajectory(X, lmbda=0.01, tol=1e-3, maxiter=100):
    """The oracle's iterates [(A_k, E_k, ratio_k)], k = 1..K (list index k - 1)"""
    return _loop(X, _low_rank_svd, lmbda, tol, maxiter)


def gram_trajectory(X, lmbda=0.01, tol=1e-3, maxiter=100):
    return _loop(X, _low_rank_gram, lmbda, tol, maxiter)


def mutant_trajectory(X, which, lmbda=0.01, tol=1e-3, maxiter=100):
    """A deliberately wrong Gram-route stand-in: "mu_late" grows mu one iteration late at k = 3 only, "dead_weight" keeps the
    dead-direction weight from iteration 2 on"""
    if which == "mu_late":
        return _loop(X, _low_rank_gram, lmbda, tol, maxiter, mu_late_at=3)
    assert which == "dead_weight"
    return _loop(X, _low_rank_gram, lmbda, tol, maxiter, keep_dead_weight=True)


def boundary_mask(E, band=BAND):
    """True where -E lies within band of an integer 1..255"""
    v = -np.asarray(E, np.float64)
    r = np.rint(v)
    return (np.abs(v - r) <= band) & (r >= 1.0) & (r <= 255.0)


def sparse_u8(E):
    """image_filtering.py:244-245 in numpy: clip(-E, 0, 255) truncated to uint8 (oracle.rpca_epilogue is the C statement of it)"""
    return np.clip(-np.asarray(E, np.float64), 0.0, 255.0).astype(np.uint8)


# ------------------------------------------------------------------ the windows
Case = namedtuple("Case", "name K n Hc Wc null dup")
# K: the iteration that stops by tol; null: leading all-zero frames; dup: index of a frame that repeats the next one (or None)


def _gray(roi):
    return np.stack([orc.bgr2gray(f) for f in roi])


@functools.lru_cache(maxsize=None)
def frames(name):
    """(n, Hc, Wc) uint8 grey frames of a case, queue order (read-only)"""
    from swiftwatcher_amd.synthetic import roi_window
    small = dict(birds=3, bird_len=(8, 14), bird_wid=(3, 6))
    if name == "plain21":
        roi = roi_window(40, 21, 64, 96, **small)
    elif name == "null21":
        roi = roi_window(11, 21, 64, 96, birds=4, bird_len=(8, 14), bird_wid=(3, 6), null_frames=4)
    elif name == "short5":
        roi = roi_window(505, 5, 120, 160, birds=3)
    elif name == "full64":
        roi = roi_window(564, 64, 48, 80, birds=3)
    elif name == "wide70":
        roi = roi_window(570, 70, 48, 80, birds=3)
    elif name == "wide65":
        roi = roi_window(565, 65, 48, 80, birds=3)
    elif name == "dup":
        # the last window of a video, newest first: [null ... null, duplicate, last real frame, older frames ...] (io_video.py:40-53)
        n, real = 21, 15
        roi = roi_window(730, n, 64, 96, **small)
        pad = n - real - 1
        roi[:pad] = 0
        roi[pad] = roi[pad + 1]
    elif name == "n37":
        roi = roi_window(937, 37, 48, 80, **small)          # 142,080 elements, three MFMA frame blocks, n mod 4 = 1
    else:
        raise KeyError(name)
    g = _gray(roi)
    g.setflags(write=False)
    return g


CASES = {c.name: c for c in (
    Case("plain21", 23, 21, 64, 96, 0, None),
    Case("null21", 23, 21, 64, 96, 4, None),
    Case("short5", 15, 5, 120, 160, 0, None),
    Case("full64", 24, 64, 48, 80, 0, None),
    Case("wide70", 24, 70, 48, 80, 0, None),
    Case("wide65", 24, 65, 48, 80, 0, None),
    Case("dup", 22, 21, 64, 96, 5, 5),
    Case("n37", 24, 37, 48, 80, 0, None),
)}
FULL_RANK = ("plain21", "short5", "full64", "wide70", "wide65", "n37")


def planes(name):
    """(n, P) uint8: the window as the library takes it"""
    g = frames(name)
    return g.reshape(g.shape[0], -1)


def matrix(name):
    """(P, n): the window as the oracle takes it"""
    return planes(name).T


@functools.lru_cache(maxsize=None)
def reference(name):
    """trajectory() of a case, cached for the session; the arrays are read-only"""
    tr = trajectory(matrix(name))
    for it in tr:
        it.A.setflags(write=False)
        it.E.setflags(write=False)
    return tr


@functools.lru_cache(maxsize=None)
def standin(name):
    return gram_trajectory(matrix(name))


def steps(name):
    """K of a case"""
    return len(reference(name))


def ks_to_test(name):
    """Every cap k = 1..K + 1 (the 25 runs of a 64- or 70-frame window take 0.03 to 0.3 s on an MI355X: no need to thin them out)"""
    return list(range(1, steps(name) + 2))


# ------------------------------------------------------------------ the assertions of the GPU test, on any trajectory
def check_iterate(name, k, A, E, iters, ratio=None, err_bound=0.0):
    """What tests/test_ialm_trajectory_gpu.py asserts of a run stopped at maxiter = k (A, E (P, n)): the iteration count, A_k and E_k
    within ATOL_AE, exact zeros in null frames, the copies of a duplicated frame within ATOL_COPIES, and the stopping norm within the bound the
    triangle inequality gives it: Z = X - A - E, so | ||Z|| - ||Z_k|| | <= ||(A - A_k) + (E - E_k)||_F.  Returns (max |A - A_k|,
    max |E - E_k|)."""
    case, tr = CASES[name], reference(name)
    K = len(tr)
    ref = tr[min(k, K) - 1]
    assert iters == min(k, K), "%s maxiter %d: %d iterations, reference %d" % (name, k, iters, min(k, K))
    dA, dE = A - ref.A, E - ref.E
    eA, eE = float(np.abs(dA).max()), float(np.abs(dE).max())
    assert eA <= ATOL_AE, "%s k=%d: max |A - A_k| = %.3e" % (name, k, eA)
    assert eE <= ATOL_AE, "%s k=%d: max |E - E_k| = %.3e" % (name, k, eE)
    if case.null:
        assert not A[:, :case.null].any() and not E[:, :case.null].any(), "%s k=%d: a null frame is not exactly 0" % (name, k)
    if case.dup is not None:
        cA, cE = copies_differ(A, case.dup), copies_differ(E, case.dup)
        assert cA <= ATOL_COPIES and cE <= ATOL_COPIES, "%s k=%d: the two copies of the duplicated frame differ by %.3e in A, %.3e in E" % (name, k, cA, cE)
    if ratio is not None:
        x_fro = np.linalg.norm(matrix(name).astype(np.float64), 'fro')
        bound = np.linalg.norm(dA + dE, 'fro') / x_fro + 1e-10 * ref.ratio
        assert abs(ratio - ref.ratio) <= bound, "%s k=%d: ratio %.12e, reference %.12e, bound %.3e" % (name, k, ratio, ref.ratio, bound)
        assert err_bound == 0.0
    return eA, eE


def copies_differ(a, dup):
    """max |a[:, dup] - a[:, dup + 1]|"""
    return float(np.abs(a[:, dup] - a[:, dup + 1]).max())


def check_final_only(name, tr):
    """The check the suite had before: the same K, and the last A and E within ATOL_AE"""
    ref = reference(name)
    return len(tr) == len(ref) and np.abs(tr[-1].A - ref[-1].A).max() <= ATOL_AE and np.abs(tr[-1].E - ref[-1].E).max() <= ATOL_AE
