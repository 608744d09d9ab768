"""Test-side restatement of the review video's definition (include/swk.h, swk_render_review / swk_bgr_to_yuv420): the blend, the four
overlay layers and BGR -> 4:2:0 YUV, as plain scalar formulas evaluated elementwise over int64 arrays.  Written from the
definition's text, not from the kernel.

    blend(p, col, a) = (p * (256 - a) + col * a + 128) >> 8          per channel
    layers, in order: mask tint (fill alpha), boxes in array order (edge pixels line alpha, inner pixels fill alpha), marks in array
    order (plus signs, line alpha), border (line alpha)
    Y = ( 269484 R + 528482 G + 102760 B + (1 << 19) + (16  << 20)) >> 20          every composed pixel
    U = (-155188 R - 305135 G + 460324 B + (1 << 19) + (128 << 20)) >> 20          composed pixel (2 i, 2 j) of chroma cell (i, j)
    V = ( 460324 R - 385875 G -  74448 B + (1 << 19) + (128 << 20)) >> 20
"""
import numpy as np

# (B, G, R) -> (Y, U, V), worked by hand
HAND_VECTORS = [
    ((0, 0, 0), (16, 128, 128)),
    ((255, 255, 255), (235, 128, 128)),
    ((0, 0, 255), (82, 90, 240)),
    ((0, 255, 0), (145, 54, 34)),
    ((255, 0, 0), (41, 240, 110)),
    ((130, 130, 130), (128, 128, 128)),
    ((1, 2, 3), (18, 127, 129)),
    ((200, 100, 50), (99, 179, 99)),
]


def blend(p, col, a):
    p, col, a = (np.asarray(x).astype(np.int64) for x in (p, col, a))
    return (p * (256 - a) + col * a + 128) >> 8


def yuv_pixels(B, G, R):
    """(Y, U, V) of equally shaped arrays of B, G, R values."""
    B, G, R = (np.asarray(x).astype(np.int64) for x in (B, G, R))
    h = 1 << 19
    Y = (269484 * R + 528482 * G + 102760 * B + h + (16 << 20)) >> 20          # (numpy's >> on signed integers is arithmetic)
    U = (-155188 * R - 305135 * G + 460324 * B + h + (128 << 20)) >> 20
    V = (460324 * R - 385875 * G - 74448 * B + h + (128 << 20)) >> 20
    return Y, U, V


def to_bgr3(frames):
    """(F, H, W, 3) int64 of BGR (F, H, W, 3) or gray (F, H, W) frames (gray is B = G = R)."""
    f = np.asarray(frames).astype(np.int64)
    return np.repeat(f[..., None], 3, axis=-1) if f.ndim == 3 else f


def yuv420(bgr):
    """(y, u, v) uint8 of composed frames (F, H, W, 3): y (F, H, W), u and v (F, ceil(H/2), ceil(W/2)) from the even pixels."""
    bgr = np.asarray(bgr)
    if bgr.ndim == 3:
        bgr = to_bgr3(bgr)
    Y, U, V = yuv_pixels(bgr[..., 0], bgr[..., 1], bgr[..., 2])
    assert Y.min() >= 16 and Y.max() <= 235 and min(U.min(), V.min()) >= 16 and max(U.max(), V.max()) <= 240
    return Y.astype(np.uint8), U[:, ::2, ::2].astype(np.uint8), V[:, ::2, ::2].astype(np.uint8)


def nv12(u, v):
    return np.stack([u, v], axis=-1)


def _style(styles, k):
    """((b, g, r), fill_alpha, line_alpha) of style k >= 1; styles: rows (b, g, r, fill_alpha, line_alpha)."""
    b, g, r, fill, line = (int(x) for x in styles[k - 1])
    return np.array([b, g, r], np.int64), fill, line


def compose(frames, boxes=(), marks=(), frame_style=None, mask=None, styles=(), mask_style=0, mark_arm=0, border=0):
    """The four layers over frames (F, H, W[, 3]) -> (F, H, W, 3) int64.  boxes: rows (frame, r0, c0, r1, c1, style); marks: rows
    (frame, r, c, style); styles: rows (b, g, r, fill_alpha, line_alpha); style 0 draws nothing."""
    out = to_bgr3(frames).copy()
    F, H, W = out.shape[:3]
    rr, cc = np.mgrid[0:H, 0:W]
    for f in range(F):
        img = out[f]
        # 1. mask
        if mask is not None and mask_style:
            col, fill, _ = _style(styles, mask_style)
            sel = np.asarray(mask) != 0
            img[sel] = blend(img[sel], col, fill)
        # 2. boxes
        for bf, r0, c0, r1, c1, st in boxes:
            if bf != f or st == 0:
                continue
            col, fill, line = _style(styles, st)
            inside = (rr >= r0) & (rr < r1) & (cc >= c0) & (cc < c1)
            edge = inside & ((rr == r0) | (rr == r1 - 1) | (cc == c0) | (cc == c1 - 1))
            inner = inside & ~edge
            img[edge] = blend(img[edge], col, line)
            img[inner] = blend(img[inner], col, fill)
        # 3. marks
        for mf, r, c, st in marks:
            if mf != f or st == 0:
                continue
            col, _, line = _style(styles, st)
            sel = ((cc == c) & (np.abs(rr - r) <= mark_arm)) | ((rr == r) & (np.abs(cc - c) <= mark_arm))
            img[sel] = blend(img[sel], col, line)
        # 4. border
        if frame_style is not None and frame_style[f]:
            col, _, line = _style(styles, int(frame_style[f]))
            sel = (rr < border) | (rr >= H - border) | (cc < border) | (cc >= W - border)
            img[sel] = blend(img[sel], col, line)
    return out


def render(frames, **kw):
    """(y, u, v) uint8 of the composed frames."""
    return yuv420(compose(frames, **kw))
