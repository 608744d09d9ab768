"""Material shared by the deinterlacer's tests: sources of every format as they lie in memory beside their sample values, the designed
planes on which one direction of the edge search, its strict comparison, its search order or one side of the temporal clamp decides."""
import itertools
import zlib

import numpy as np

import deinterlace_ref as ref

# name -> (layout, (sx, sy), bits, msb_aligned, full_range)
FORMATS = {
    "420": ("planar", (1, 1), 8, False, False),
    "422": ("planar", (1, 0), 8, False, False),
    "444": ("planar", (0, 0), 8, False, False),
    "411": ("planar", (2, 0), 8, False, False),
    "mono": ("mono", (0, 0), 8, False, False),
    "420p10": ("planar", (1, 1), 10, False, False),
    "444p16": ("planar", (0, 0), 16, False, True),
    "nv12": ("semi", (1, 1), 8, False, False),
    "p010": ("semi", (1, 1), 10, True, False),
    "420full": ("planar", (1, 1), 8, False, True),
}


def rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


class Source:
    """`count` frames of one format: values = (Y, U, V) int64 sample values (U = V = None for mono), planes = what
    Context.yuv_deinterlace takes (the words as they lie in memory), kw = its format keywords."""

    def __init__(self, name, count, H, W, seed=0, pitch=0, coarse=False, still=False):
        layout, (sx, sy), bits, msb, full = FORMATS[name]
        r = rng("src", name, count, H, W, seed)
        dt = np.uint16 if bits > 8 else np.uint8
        CH, CW = ((H - 1) >> sy) + 1, ((W - 1) >> sx) + 1

        def values(h, w):
            v = r.integers(0, 1 << bits, size=(count, h, w), dtype=np.int64)
            if coarse:                                  # few levels: equal scores, so the strict comparisons decide
                v = (v >> (bits - 2)) << (bits - 2)
            if still:
                v[:] = v[0]
            return v
        Y = values(H, W)
        U, V = (None, None) if layout == "mono" else (values(CH, CW), values(CH, CW))
        self.name, self.count, self.H, self.W, self.layout = name, count, H, W, layout
        self.subsampling, self.bits, self.msb, self.full = (sx, sy), bits, msb, full
        self.values = (Y, U, V)
        shift = 16 - bits if msb else 0

        def words(v, inner=1):
            # (count, h, w[, 2]) words inside rows `pitch` samples longer than needed, the spare samples set to a value of their own
            shape = v.shape
            wide = np.full(shape[:2] + (shape[2] * inner + pitch,), (1 << bits) - 1 if not msb else 0xFFFF, dt)
            view = wide[:, :, :shape[2] * inner]
            view[...] = (v.reshape(shape[0], shape[1], -1) << shift).astype(dt)
            return view
        if layout == "mono":
            self.planes = (words(Y),)
        elif layout == "planar":
            self.planes = (words(Y), words(U), words(V))
        else:
            self.planes = (words(Y), words(np.stack([U, V], axis=-1), 2))
        self.kw = dict(subsampling=(sx, sy), bits=bits, msb_aligned=msb, full_range=full)

    def on_device(self, torch):
        """the same planes as tensors on the GPU (views of pitched tensors where the host planes are views)"""
        out = []
        for p in self.planes:
            base = p.base if p.base is not None else p
            t = torch.from_numpy(np.ascontiguousarray(base)).to("cuda:0")
            out.append(t[:, :, :p.shape[2]] if base.shape != p.shape else t)
        return tuple(out)

    def expected(self, rect=None, **params):
        """(BGR, (Y, U, V)) of the restatement for this source"""
        Y, U, V = self.values
        pl = ref.call(Y, U, V, subsampling=self.subsampling, rect=rect, **params)
        bgr = ref.call_bgr(Y, U, V, subsampling=self.subsampling, bits=self.bits, full_range=self.full, rect=rect, **params)
        return bgr, pl


def same(got, want):
    """got (an array of the call) equals want (sample values of the restatement), as integers"""
    if want is None:
        return got is None
    return got is not None and got.shape == want.shape and np.array_equal(np.asarray(got).astype(np.int64), np.asarray(want).astype(np.int64))


def param_cycle():
    """every combination of tff, rate, temporal, has_prev, has_next and a count from (1, 2, 3, 5) that leaves a frame, forever"""
    combos = []
    for tff, rate, temporal, hp, hn in itertools.product((1, 0), (2, 1), (1, 0), (0, 1), (0, 1)):
        for count in (1, 2, 3, 5):
            if count - hp - hn >= 1:
                combos.append((count, dict(tff=tff, rate=rate, temporal=temporal, has_prev=hp, has_next=hn)))
    order = rng("cycle").permutation(len(combos))
    return itertools.cycle([combos[k] for k in order]), len(combos)


# ------------------------------------------------------------------------------------------------ designed planes
def _edge_rows(W, j, lo=20, hi=200):
    """rows above and below a missing row on which a step edge runs in direction j: the row above shows it j columns further right
    than the missing row would, the row below j columns further left"""
    at = W // 2
    up = np.where(np.arange(W) < at + j, lo, hi)
    dn = np.where(np.arange(W) < at - j, lo, hi)
    return up, dn


def direction_plane(j, W=16):
    """One frame (1, 3, W): rows 0 and 2 are kept (tff, first field), row 1 is missing; at column W // 2 - 1 ... W // 2 the edge of
    direction j crosses it.  Returns (plane, x, expected direction at x)."""
    up, dn = _edge_rows(W, j)
    P = np.zeros((1, 3, W), np.int64)
    P[0, 0], P[0, 2] = up, dn
    P[0, 1] = 77          # (the missing row's stored samples: the second field, not read with temporal = 0)
    return P, W // 2, j


def tie_plane(W=16):
    """Rows on which score_{-1} == score at the probed column, so that direction -1 must not be taken (and its prediction would
    differ from the vertical one, so taking it would show); direction +1 scores worse.  Found by a seeded search.  Returns (plane, x)."""
    r = rng("tie")
    for _ in range(100000):
        up = r.integers(0, 8, W).astype(np.int64)
        dn = r.integers(0, 8, W).astype(np.int64)
        x = W // 2
        score = abs(up[x - 1] - dn[x - 1]) + abs(up[x] - dn[x]) + abs(up[x + 1] - dn[x + 1]) - 1
        sm1 = sum(abs(up[x + k - 1] - dn[x + k + 1]) for k in (-1, 0, 1))
        sp1 = sum(abs(up[x + k + 1] - dn[x + k - 1]) for k in (-1, 0, 1))
        pm1 = (up[x - 1] + dn[x + 1]) >> 1
        if sm1 == score and sp1 > score and pm1 != (up[x] + dn[x]) >> 1:
            P = np.zeros((1, 3, W), np.int64)
            P[0, 0], P[0, 2] = up, dn
            return P, x
    raise AssertionError("no tie found")


def unreached_plane(W=16):
    """j = -2 alone would beat the vertical score, j = -1 does not: -2 must not be reached (nor any other direction taken)"""
    r = rng("unreached")
    for _ in range(200000):
        up = r.integers(0, 16, W).astype(np.int64)
        dn = r.integers(0, 16, W).astype(np.int64)
        x = W // 2
        score = abs(up[x - 1] - dn[x - 1]) + abs(up[x] - dn[x]) + abs(up[x + 1] - dn[x + 1]) - 1
        s = {j: sum(abs(up[x + k + j] - dn[x + k - j]) for k in (-1, 0, 1)) for j in (-2, -1, 1, 2)}
        p2 = (up[x - 2] + dn[x + 2]) >> 1
        if s[-2] < score and s[-1] >= score and s[1] >= score and p2 != (up[x] + dn[x]) >> 1:
            P = np.zeros((1, 3, W), np.int64)
            P[0, 0], P[0, 2] = up, dn
            return P, x
    raise AssertionError("no such rows found")


def clamp_planes(side, W=12):
    """Three frames (3, 3, W), row 1 missing in the middle frame's first picture (tff): the rows above and below are equal in all three
    frames (td1 = td2 = 0) and give pred = 100; the missing row's own samples are b in the frame before and a in this frame, so the
    clamp is [dm - (|b - a| >> 1), dm + (|b - a| >> 1)].  side = "low": the whole interval lies above pred (out = its lower end);
    "high": below pred (out = its upper end).  Returns (planes, expected sample value of row 1)."""
    P = np.full((3, 3, W), 100, np.int64)
    b, a = (180, 160) if side == "low" else (30, 50)
    P[0, 1], P[1, 1], P[2, 1] = b, a, a
    dm, diff = (b + a) >> 1, abs(b - a) >> 1
    return P, (dm - diff if side == "low" else dm + diff)


DESIGNED = [("dir%+d" % j, direction_plane(j)[0]) for j in (-2, -1, 0, 1, 2)] + \
           [("tie", tie_plane()[0]), ("unreached", unreached_plane()[0]), ("clamp_low", clamp_planes("low")[0]), ("clamp_high", clamp_planes("high")[0])]
