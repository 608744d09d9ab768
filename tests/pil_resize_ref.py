"""Pillow's antialiased bilinear resize of an 8-bit H x W x 3 image to 24 x 24, restated in numpy: libImaging/Resample.c as the
reference's pinned Pillow 8.1.1 runs it.  Coefficients in float64 (support = max(scale, 1), weights summed in index order, normalised,
rounded to 22-bit fixed point), the HORIZONTAL pass first, to uint8, then the vertical pass; each accumulates in integers from 2^21
and clips (x >> 22) to [0, 255].  A side that already is 24 skips its pass.

Horizontal first, always, is the definition the device code is held to.  Newer Pillows (seen with 12.2) run the vertical pass first
on some tall, narrow images (3000 x 25, 4096 x 40, 8000 x 30, ...), which moves some 300 of the 1728 output bytes by one; so tall
shapes are compared with tests/golden/pil_resize_large.npz (tools/make_pil_resize_goldens.py, Pillow 8.4.0), never with the
installed Pillow."""
import numpy as np

OUT = 24
PRECISION = 22
MAX_K = 343                      # coefficients per output sample at the largest input size of the device route, 4096


def formula_image(rows, cols, offset=0):
    """The test image of every large-crop test, from a closed formula (no RNG: every interpreter and the GPU tests build the same
    bytes): pixel (r, c, ch) = (131 r + 71 c + 37 ch + (r c mod 251) + offset) mod 256."""
    r = np.arange(rows, dtype=np.int64)[:, None, None]
    c = np.arange(cols, dtype=np.int64)[None, :, None]
    ch = np.arange(3, dtype=np.int64)[None, None, :]
    return ((131 * r + 71 * c + 37 * ch + (r * c) % 251 + offset) % 256).astype(np.uint8)


def coeffs(in_size, out_size=OUT):
    """precompute_coeffs + normalize_coeffs_8bpc: (bounds (out, 2) = first input sample and count, list of int64 coefficient arrays).
    Every operation is a float64 numpy operation rounded on its own, in the C code's order; the weights are summed by np.cumsum, which
    adds them one after the other in index order as the C loop does (np.sum adds pairwise and may differ in the last bit)."""
    scale = float(in_size) / float(out_size)
    filterscale = 1.0 if scale < 1.0 else scale
    support = 1.0 * filterscale
    ss = 1.0 / filterscale
    bounds = np.zeros((out_size, 2), np.int64)
    ks = []
    for xx in range(out_size):
        center = 0.0 + (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        v = np.abs(((np.arange(xmax) + xmin).astype(np.float64) - center + 0.5) * ss)
        w = np.where(v < 1.0, 1.0 - v, 0.0)
        ww = float(np.cumsum(w)[-1]) if xmax else 0.0
        c = w / ww if ww != 0.0 else w
        ks.append((0.5 + c * float(1 << PRECISION)).astype(np.int64))          # c >= 0: the C code's int() truncation
        bounds[xx] = (xmin, xmax)
    return bounds, ks


def coeff_table(in_size):
    """coeffs() in the layout of swk_debug_resize_table: (bounds (24, 2) int32, table (24, 343) int32, zeros behind each sample's last)."""
    bounds, ks = coeffs(in_size)
    table = np.zeros((OUT, MAX_K), np.int32)
    for xx, k in enumerate(ks):
        table[xx, :len(k)] = k
    return bounds.astype(np.int32), table


def _clip8(acc):
    return np.clip(acc >> PRECISION, 0, 255).astype(np.uint8)


def resize(image):
    """The 24 x 24 x 3 patch of an H x W x 3 uint8 image, horizontal pass first.  Returns (patch, (bounds_x, kx), (bounds_y, ky))."""
    image = np.ascontiguousarray(image, np.uint8)
    h, w = image.shape[:2]
    tx, ty = coeffs(w), coeffs(h)
    tmp = image
    if w != OUT:
        tmp = np.empty((h, OUT, 3), np.uint8)
        src = image.astype(np.int64)
        for xx in range(OUT):
            xmin, xmax = tx[0][xx]
            acc = (1 << (PRECISION - 1)) + np.tensordot(src[:, xmin:xmin + xmax, :], tx[1][xx], axes=([1], [0]))
            tmp[:, xx, :] = _clip8(acc)
    out = tmp
    if h != OUT:
        out = np.empty((OUT, OUT, 3), np.uint8)
        src = tmp.astype(np.int64)
        for yy in range(OUT):
            ymin, ymax = ty[0][yy]
            acc = (1 << (PRECISION - 1)) + np.tensordot(ty[1][yy], src[ymin:ymin + ymax], axes=([0], [0]))
            out[yy] = _clip8(acc)
    return np.ascontiguousarray(out), tx, ty


def patch(image):
    return resize(image)[0]
