"""Crops designed so that ONE tap of Pillow's 24 x 24 resize decides an output byte (numpy only; shared by test_resize_taps_cpu.py and
test_resize_taps_gpu.py).

The outermost coefficient of an output sample is small (about 1e-3 of the sum at input size 512), so on random content a loop that
loses it usually gives the right byte.  For an input size s the TARGETS are every output sample's first and last non-zero coefficient
(a zero outermost coefficient moves the target one tap inwards: no content can show a tap whose coefficient is 0).  The SIGNAL of a
target t holds 255 at tap t and a base value elsewhere, and one or two of the heaviest other taps are adjusted until the accumulator
without tap t lies less than 255 k_t below a multiple of 2^22: with the tap the byte is one more than without it.  The full accumulator
stays at or below 255 after the shift, so the clip never decides.  (Where one tap is both targets of a sample, at some sizes below 24,
the second signal holds 254 there, so that the crop's two signal channels differ.)

A crop isolates one pass.  Horizontal, 24 x s x 3: the vertical pass is skipped (24 rows); row r carries the signals of output column
r over that column's taps, channel 0 the first tap's, channel 1 the last tap's, channel 2 and every other byte pil_resize_ref's
formula image.  The designed byte of target (r, first / last) is patch[r, r, 0 / 1].  Vertical: the transpose, s x 24 x 3."""
import functools

import numpy as np

import pil_resize_ref as P

OUT = P.OUT
ONE = 1 << P.PRECISION
HALF = 1 << (P.PRECISION - 1)
BASES = (0, 128, 51, 204, 102, 153)                       # the value of the taps that are neither the target nor adjusted

SMALL_SIZES = [s for s in range(1, 513) if s != OUT]          # k_classifier_input / k_segment_inputs
# k_segment_inputs_large: the sizes at which a sample's tap count grows (ceil(s / 24) changes), the sizes just below them, and 4096
_GROW = [s for s in range(513, 4097) if -(-s // OUT) != -(-(s - 1) // OUT)]
LARGE_SIZES = sorted(set(_GROW) | {s - 1 for s in _GROW} | {4096})
assert len(LARGE_SIZES) == 299 and LARGE_SIZES[0] > 512

# shapes (rows, columns) on which both passes run; formula content at an offset chosen by combined()
COMBINED_SMALL = [(25, 25), (47, 48), (100, 37), (37, 100), (255, 256), (511, 512), (512, 512), (512, 25), (25, 512)]
COMBINED_LARGE = [(513, 600), (600, 513), (1031, 520), (4096, 30), (30, 4096)]


@functools.lru_cache(maxsize=None)
def coeffs(size):
    return P.coeffs(size)


# ------------------------------------------------------------------ the restatement, with the changes the tests ask of it
def _drop_index(drop, k):
    if drop is None:
        return -1
    if isinstance(drop, str):
        return {"first": 0, "last": len(k) - 1}[drop]
    return int(drop)


def _pass(src, table, drop, rounding, reverse, swap01):
    """One pass of pil_resize_ref.resize along axis 1 of src (rows, size, 3) int64 -> (rows, 24, 3) uint8.  drop: None, "first",
    "last" or 24 tap indices (-1: none), the tap left out of each output sample; reverse: coefficients applied in reverse order;
    swap01: channels 0 and 1 swapped in the accumulation."""
    bounds, ks = table
    out = np.empty((src.shape[0], OUT, 3), np.uint8)
    if swap01:
        src = src[:, :, [1, 0, 2]]
    for xx in range(OUT):
        xmin, xmax = bounds[xx]
        k = ks[xx][::-1] if reverse else ks[xx]
        d = _drop_index(drop if drop is None or isinstance(drop, str) else drop[xx], k)
        taps = src[:, xmin:xmin + xmax, :]
        if d >= 0:
            keep = np.arange(xmax) != d
            taps, k = taps[:, keep, :], k[keep]
        acc = rounding + np.tensordot(taps, k, axes=([1], [0]))
        out[:, xx, :] = np.clip(acc >> P.PRECISION, 0, 255).astype(np.uint8)
    return out


def resize(image, drop_x=None, drop_y=None, rounding=HALF, reverse=False, swap01=False):
    """pil_resize_ref.resize (horizontal pass first, to uint8, then the vertical pass; a side of 24 skips its pass) with optional
    changes.  With none it IS the restatement (asserted in test_resize_taps_cpu.py).  The vertical pass is the horizontal one on the
    transposed intermediate: the same integer sums."""
    image = np.ascontiguousarray(image, np.uint8)
    h, w = image.shape[:2]
    tmp = image
    if w != OUT:
        tmp = _pass(image.astype(np.int64), coeffs(w), drop_x, rounding, reverse, swap01)
    if h != OUT:
        tmp = _pass(tmp.transpose(1, 0, 2).astype(np.int64), coeffs(h), drop_y, rounding, reverse, swap01).transpose(1, 0, 2)
    return np.ascontiguousarray(tmp)


MUTANTS = {          # name -> keyword arguments of resize() for (horizontal crop, vertical crop)
    "first_tap_dropped": (dict(drop_x="first"), dict(drop_y="first")),
    "last_tap_dropped": (dict(drop_x="last"), dict(drop_y="last")),
    "no_rounding_term": (dict(rounding=0), dict(rounding=0)),
    "coefficients_reversed": (dict(reverse=True), dict(reverse=True)),
    "channels_0_1_swapped": (dict(swap01=True), dict(swap01=True)),
}


# ------------------------------------------------------------------ signals
PEAK = 255                                                # the value a signal holds at its target tap


def _flips(acc_without, d):
    """The byte with the target tap is not the byte without it, and the clip decides neither."""
    return ((acc_without % ONE) + d >= ONE) & (((acc_without + d) >> P.PRECISION) <= 255)


def signal(k, t, peak=PEAK):
    """uint8 values over the taps of coefficients k (int64) whose output byte changes when tap t (k[t] > 0) is dropped, or None.
    The heaviest other tap is searched alone over 0..255 at the six bases; only where that fails, it and a second heavy tap together."""
    d = peak * int(k[t])
    inner = [int(i) for i in np.argsort(-k, kind="stable") if i != t and k[i] > 0]
    # the second adjusted tap has another coefficient than the first where one exists: at 4096 the two heaviest are equal, and a pair
    # of equal coefficients reaches no accumulator that one of them does not
    inner = inner[:1] + ([i for i in inner[1:] if k[i] != k[inner[0]]] or inner[1:])[:1]
    bases = np.array(BASES, np.int64)
    rest = int(k.sum() - k[t])
    values = np.arange(256, dtype=np.int64)

    def build(base, adjusted):
        v = np.full(len(k), base, np.uint8)
        v[t] = peak
        for i, a in adjusted:
            v[i] = a
        return v

    acc0 = HALF + bases * rest                                          # every other tap at the base
    if not inner:
        good = np.flatnonzero(_flips(acc0, d))
        return build(BASES[good[0]], []) if len(good) else None
    h1 = inner[0]
    acc1 = acc0[:, None] + (values[None, :] - bases[:, None]) * int(k[h1])          # (base, value of the heaviest tap)
    good = np.argwhere(_flips(acc1, d))
    if len(good):
        b, a = good[0]
        return build(BASES[b], [(h1, a)])
    if len(inner) > 1:
        h2 = inner[1]
        for b, base in enumerate(BASES):
            acc2 = acc1[b][:, None] + (values[None, :] - base) * int(k[h2])
            good = np.argwhere(_flips(acc2, d))
            if len(good):
                a1, a2 = good[0]
                return build(base, [(h1, a1), (h2, a2)])
    return None


class Design:
    """The signals of one input size: target[xx, e] = tap index of output sample xx's first (e = 0) / last (e = 1) non-zero
    coefficient, moved[xx, e] = the outermost coefficient on that side is 0, signals[xx][e] = uint8 values over the sample's taps,
    missing = [(size, xx, e), ...] non-zero targets for which no signal was found (none expected)."""

    def __init__(self, size):
        self.size = size
        self.bounds, self.ks = coeffs(size)
        self.target = np.zeros((OUT, 2), np.int64)
        self.moved = np.zeros((OUT, 2), bool)
        self.signals = []
        self.missing = []
        for xx, k in enumerate(self.ks):
            nz = np.flatnonzero(k)
            pair = []
            for e, t in enumerate((int(nz[0]), int(nz[-1]))):
                self.target[xx, e] = t
                self.moved[xx, e] = t != (0, len(k) - 1)[e]
                v = signal(k, t)
                if v is not None and e == 1 and np.array_equal(v, pair[0]):
                    # one tap is both targets (size 1): channels 0 and 1 of the crop must still differ, so the second signal peaks lower
                    v = signal(k, t, peak=PEAK - 1)
                if v is None:
                    self.missing.append((size, xx, e))
                    v = np.full(len(k), BASES[0], np.uint8)
                    v[t] = 255
                pair.append(v)
            self.signals.append(pair)

    def horizontal(self):
        """The 24 x size x 3 crop."""
        s = self.size
        crop = P.formula_image(OUT, s, offset=s % 256)
        for r in range(OUT):
            xmin, xmax = self.bounds[r]
            crop[r, xmin:xmin + xmax, 0] = self.signals[r][0]
            crop[r, xmin:xmin + xmax, 1] = self.signals[r][1]
        return crop

    def vertical(self):
        """The size x 24 x 3 crop: the transpose."""
        return np.ascontiguousarray(self.horizontal().transpose(1, 0, 2))


@functools.lru_cache(maxsize=None)
def design(size):
    return Design(size)


def moved_share(sizes):
    """Share of the targets of `sizes` that a zero outermost coefficient moved one tap inwards."""
    moved = sum(int(design(s).moved.sum()) for s in sizes)
    return moved / float(len(sizes) * OUT * 2)


# ------------------------------------------------------------------ combined crops: both passes run
@functools.lru_cache(maxsize=None)
def combined(shape):
    """(image, offset): the formula image of `shape` at the first offset in 0..255 at which losing the last tap of the horizontal
    pass changes the patch, and losing the last tap of the vertical pass changes it too; (None, None) when no offset does."""
    h, w = shape
    for offset in range(256):
        image = P.formula_image(h, w, offset=offset)
        true = resize(image)
        if not np.array_equal(resize(image, drop_x="last"), true) and not np.array_equal(resize(image, drop_y="last"), true):
            return image, offset
    return None, None


# ------------------------------------------------------------------ the float32 statement of the network input
def net_lut(mean, std):
    """lut[c, b] = (float32(b) / float32(255) - mean[c]) / std[c], every operation rounded to float32 on its own (ToTensor, Normalize).
    lut[c, 0] is the padding's value."""
    b = np.arange(256, dtype=np.float32) / np.float32(255)
    m = np.asarray(mean, np.float32)[:, None]
    s = np.asarray(std, np.float32)[:, None]
    lut = (b[None, :] - m) / s
    assert lut.dtype == np.float32
    return lut


def net_interior(patches, mean, std):
    """(n, 24, 24, 3) uint8 patches -> (n, 3, 24, 24) float32: the part of the network input inside the padding."""
    lut = net_lut(mean, std)
    p = np.asarray(patches)
    return np.stack([lut[c][p[..., c]] for c in range(3)], axis=1)


def net_input(patch, mean, std, pad):
    """One patch -> (3, 24 + 2 pad, 24 + 2 pad) float32."""
    lut = net_lut(mean, std)
    side = OUT + 2 * pad
    out = np.empty((3, side, side), np.float32)
    out[:] = lut[:, 0][:, None, None]
    out[:, pad:pad + OUT, pad:pad + OUT] = net_interior(patch[None], mean, std)[0]
    return out
