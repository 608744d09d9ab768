"""Test-side restatement of 4:2:0 YUV -> BGR as cv2.cvtColor(yuv, COLOR_YUV2BGR_I420 / _NV12) of OpenCV 4.1.0 computes it
(ITU-R BT.601, limited range, 20-bit fixed point): the plain scalar formula, evaluated elementwise over int64 arrays, plus hand
vectors.  Chroma is not interpolated: pixel (r, c) uses chroma sample (r >> 1, c >> 1)."""
import numpy as np

CY, CUB, CUG, CVG, CVR, SHIFT = 1220542, 2116026, -409993, -852492, 1673527, 20

# (Y, U, V) -> (B, G, R), worked by hand
HAND_VECTORS = [
    ((16, 128, 128), (0, 0, 0)),
    ((235, 128, 128), (255, 255, 255)),
    ((128, 128, 128), (130, 130, 130)),
    ((81, 90, 240), (0, 0, 254)),
    ((145, 54, 34), (1, 255, 0)),
    ((41, 240, 110), (255, 0, 0)),
    ((0, 0, 0), (0, 154, 0)),
    ((255, 255, 255), (255, 125, 255)),
]


def sat8(x):
    return np.minimum(np.maximum(x, 0), 255)


def pixels(Y, U, V):
    """(B, G, R) of equally shaped arrays of Y, U, V values (one chroma value per pixel already)."""
    Y, U, V = (np.asarray(a).astype(np.int64) for a in (Y, U, V))
    y = np.maximum(0, Y - 16) * CY
    uu = U - 128
    vv = V - 128
    h = 1 << 19
    R = sat8((y + h + CVR * vv) >> SHIFT)          # (numpy's >> on signed integers is arithmetic)
    G = sat8((y + h + CVG * vv + CUG * uu) >> SHIFT)
    B = sat8((y + h + CUB * uu) >> SHIFT)
    return B, G, R


def bgr(y, u, v, rect=None):
    """BGR (..., Hr, Wr, 3) uint8 of 4:2:0 planes y (..., H, W), u and v (..., ceil(H/2), ceil(W/2)); rect = (x0, y0, Wr, Hr) or the
    whole frame."""
    H, W = y.shape[-2:]
    x0, y0, Wr, Hr = rect if rect is not None else (0, 0, W, H)
    rr = np.arange(y0, y0 + Hr)
    cc = np.arange(x0, x0 + Wr)
    Ys = y[..., rr[:, None], cc[None, :]]
    Us = u[..., (rr >> 1)[:, None], (cc >> 1)[None, :]]
    Vs = v[..., (rr >> 1)[:, None], (cc >> 1)[None, :]]
    return np.stack(pixels(Ys, Us, Vs), axis=-1).astype(np.uint8)


def bgr_to_yuv420(frames):
    """Any BGR -> 4:2:0 formula serves the tests that need YUV material (BT.601 limited range in float, chroma averaged over each
    2 x 2 cell, edge cells over what exists): (y, u, v) uint8 of BGR frames (F, H, W, 3)."""
    f = frames.astype(np.float64)
    B, G, R = f[..., 0], f[..., 1], f[..., 2]
    Y = 16 + (65.481 * R + 128.553 * G + 24.966 * B) / 255
    U = 128 + (-37.797 * R - 74.203 * G + 112.0 * B) / 255
    V = 128 + (112.0 * R - 93.786 * G - 18.214 * B) / 255
    F, H, W = Y.shape
    ch, cw = (H + 1) // 2, (W + 1) // 2

    def sub(P):
        pad = np.full((F, 2 * ch, 2 * cw), np.nan)
        pad[:, :H, :W] = P
        return np.nanmean(pad.reshape(F, ch, 2, cw, 2), axis=(2, 4))
    q = lambda a: np.clip(np.rint(a), 0, 255).astype(np.uint8)          # noqa: E731
    return q(Y), q(sub(U)), q(sub(V))
