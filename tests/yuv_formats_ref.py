"""Test-side restatement of the YUV -> BGR definition of swk_yuv_to_bgr (include/swk.h) for every format: bits d = 8 .. 16, chroma
shifts (sx, sy), limited or full range, mono -- the plain formula, evaluated elementwise over int64 arrays.  The limited-range
constants are literals (OpenCV 4.1.0's); the full-range ones are derived here from Kr = 299/1000 and Kb = 114/1000 as exact
fractions and compared with the literals of the definition.  Also a forward transform BGR -> planes, used only to make clips."""
from fractions import Fraction

import numpy as np

LIMITED = (1220542, 2116026, -409993, -852492, 1673527)          # CY, CUB, CUG, CVG, CVR


def _round20(x):
    """floor(x * 2^20 + 1/2) of an exact fraction"""
    return (x * (1 << 20) + Fraction(1, 2)).__floor__()


def _full_constants():
    kr, kb = Fraction(299, 1000), Fraction(114, 1000)
    kg = 1 - kr - kb
    assert kg == Fraction(587, 1000)
    return (1 << 20, _round20(2 * (1 - kb)), _round20(-2 * kb * (1 - kb) / kg), _round20(-2 * kr * (1 - kr) / kg), _round20(2 * (1 - kr)))


FULL = _full_constants()
assert FULL == (1048576, 1858077, -360853, -748826, 1470104), FULL

SUBSAMPLINGS = {"444": (0, 0), "422": (1, 0), "420": (1, 1), "411": (2, 0)}


def chroma_shape(H, W, sx, sy):
    return ((H - 1) >> sy) + 1, ((W - 1) >> sx) + 1


def pixels(Y, U, V, bits=8, full_range=False):
    """(B, G, R) of equally shaped arrays of Y, U, V samples (one chroma value per pixel already)."""
    Y, U, V = (np.asarray(a).astype(np.int64) for a in (Y, U, V))
    k = bits - 8
    cy, cub, cug, cvg, cvr = FULL if full_range else LIMITED
    yt = Y if full_range else np.maximum(Y - (16 << k), 0)
    uu = U - (128 << k)
    vv = V - (128 << k)
    h, s = 1 << (19 + k), 20 + k
    sat8 = lambda x: np.minimum(np.maximum(x, 0), 255)          # noqa: E731
    B = sat8((cy * yt + cub * uu + h) >> s)                      # (numpy's >> on signed integers is arithmetic)
    G = sat8((cy * yt + cug * uu + cvg * vv + h) >> s)
    R = sat8((cy * yt + cvr * vv + h) >> s)
    return B, G, R


def bgr(y, u=None, v=None, rect=None, subsampling=(1, 1), bits=8, full_range=False, msb_aligned=False):
    """BGR (..., Hr, Wr, 3) uint8 of planes y (..., H, W), u and v (..., ceil(H / 2^sy), ceil(W / 2^sx)) or None (mono);
    rect = (x0, y0, Wr, Hr) or the whole frame.  msb_aligned: the sample is word >> (16 - bits)."""
    sx, sy = subsampling
    H, W = y.shape[-2:]
    x0, y0, Wr, Hr = rect if rect is not None else (0, 0, W, H)
    rr = np.arange(y0, y0 + Hr)
    cc = np.arange(x0, x0 + Wr)
    down = (16 - bits) if (msb_aligned and bits > 8) else 0
    Ys = y[..., rr[:, None], cc[None, :]].astype(np.int64) >> down
    if u is None:
        Us = Vs = np.full(Ys.shape, 128 << (bits - 8), np.int64)
    else:
        Us = u[..., (rr >> sy)[:, None], (cc >> sx)[None, :]].astype(np.int64) >> down
        Vs = v[..., (rr >> sy)[:, None], (cc >> sx)[None, :]].astype(np.int64) >> down
    return np.stack(pixels(Ys, Us, Vs, bits, full_range), axis=-1).astype(np.uint8)


def bgr_to_planes(frames, subsampling=(1, 1), bits=8, full_range=False, mono=False):
    """Any BGR -> YUV formula serves the tests that need material (BT.601 in float, chroma averaged over each cell, edge cells over
    what exists): (y, u, v) of BGR frames (F, H, W, 3), uint8 at 8 bits and uint16 (LSB-aligned) above; u = v = None for mono."""
    sx, sy = subsampling
    f = frames.astype(np.float64)
    B, G, R = f[..., 0], f[..., 1], f[..., 2]
    luma = 0.299 * R + 0.587 * G + 0.114 * B
    cb, cr = (B - luma) / 1.772, (R - luma) / 1.402          # -127.5 .. 127.5
    scale = float(1 << (bits - 8))
    top = (1 << bits) - 1
    if full_range:
        Y, U, V = luma * scale, (128 + cb) * scale, (128 + cr) * scale
    else:
        Y, U, V = (16 + luma * 219 / 255) * scale, (128 + cb * 224 / 255) * scale, (128 + cr * 224 / 255) * scale
    dt = np.uint16 if bits > 8 else np.uint8
    q = lambda a: np.clip(np.rint(a), 0, top).astype(dt)          # noqa: E731
    if mono:
        return q(Y), None, None
    F, H, W = Y.shape
    ch, cw = chroma_shape(H, W, sx, sy)

    def sub(P):
        pad = np.full((F, ch << sy, cw << sx), np.nan)
        pad[:, :H, :W] = P
        return np.nanmean(pad.reshape(F, ch, 1 << sy, cw, 1 << sx), axis=(2, 4))
    return q(Y), q(sub(U)), q(sub(V))
