"""Plain references of the classifier's convolutions for tests/test_cnn_accuracy*.py: float64 statements, float32 yardsticks in
plain sequential order (direct and Winograd F(2x2, 3x3)), the exact-integer input families with their < 2**24 precondition, the
error statistics and the 3 x criterion, and CPU simulations of split-bf16 products (correct and subtly wrong).  No GPU here.

Every convolution is taken as a matrix product over "patches": output pixel p, reduction index (ci, dy, dx) in the order of
Conv2d.weight.reshape(cout, -1).  A pool + squeeze is a 1 x 1 convolution of the (exact) max-pooled tensor."""
import numpy as np
import torch

LIMIT = float(2 ** 24)          # below it float32 holds every integer exactly
FACTOR = 3.0                    # layer 2 / 3: kernel error <= FACTOR x the plain float32 evaluation's, max and rms
FLOOR = 4e-7                    # layer 3: floor of the bound in units of max |score| (the one the split-bf16 tests use)

BT = np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], np.float64)
G = np.array([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], np.float64)
AT = np.array([[1, 1, 1, 0], [0, 1, -1, -1]], np.float64)


# ------------------------------------------------------------------ positions and patches
def sample_positions(rng, n, oh, ow, count):
    """`count` distinct output positions (segment, y, x) of an (n, oh, ow) block, or all of them when there are no more."""
    total = n * oh * ow
    idx = np.arange(total) if count >= total else np.sort(rng.choice(total, size=count, replace=False))
    return idx // (oh * ow), (idx // ow) % oh, idx % ow


def gather_patches(x, ni, yi, xi, k, stride=1):
    """x (n, c, h, w) array -> (P, c * k * k): the k x k patch whose top-left input is (stride * y, stride * x), reduction index
    (ci, dy, dx)."""
    d = np.arange(k)
    p = x[ni[:, None, None], :, (yi * stride)[:, None, None] + d[None, :, None], (xi * stride)[:, None, None] + d[None, None, :]]
    return np.ascontiguousarray(p.transpose(0, 3, 1, 2)).reshape(len(ni), -1)          # (P, k, k, c) -> (P, c, k, k)


def f64_product(a, w, b):
    """relu(a w^T + b) in float64: a (P, K), w (cout, K), b (cout,)."""
    return np.maximum(a.astype(np.float64) @ w.astype(np.float64).T + b.astype(np.float64), 0.0)


def seq_f32_product(a, w, b):
    """The same in float32, one multiply and one add (each rounded) per reduction index, in index order; bias last."""
    a, w = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(w, np.float32)
    acc = np.zeros((a.shape[0], w.shape[0]), np.float32)
    for k in range(a.shape[1]):
        acc += a[:, k:k + 1] * w[None, :, k]
    return np.maximum(acc + b.astype(np.float32)[None, :], np.float32(0))


# ------------------------------------------------------------------ Winograd F(2x2, 3x3)
def wino_filter_f32(w):
    """U = G g G^T in float64, rounded to float32 (what swk_winograd_f2x2_3x3_weights makes): (cout, cin, 3, 3) -> (cin, 4, 4, cout)."""
    u = np.einsum("ak,oikl,bl->iabo", G, np.asarray(w, np.float64), G)
    return u.astype(np.float32)


def _bt_rows(d, axis):
    d0, d1, d2, d3 = (np.take(d, i, axis=axis) for i in range(4))
    return np.stack([d0 - d2, d1 + d2, d2 - d1, d1 - d3], axis=axis)


def _at_rows(m, axis):
    m0, m1, m2, m3 = (np.take(m, i, axis=axis) for i in range(4))
    return np.stack([(m0 + m1) + m2, (m1 - m2) - m3], axis=axis)


def wino_tiles(x, ni, ty, tx):
    """x (n, c, t, t) -> the 4 x 4 input tiles (T, c, 4, 4) of output tiles (ty, tx); pixels past the tile edge (odd output sizes) read 0."""
    n, c, t, _ = x.shape
    xp = np.zeros((n, c, t + 1, t + 1), x.dtype)
    xp[:, :, :t, :t] = x
    d = np.arange(4)
    p = xp[ni[:, None, None], :, (2 * ty)[:, None, None] + d[None, :, None], (2 * tx)[:, None, None] + d[None, None, :]]
    return np.ascontiguousarray(p.transpose(0, 3, 1, 2))


def wino_f32_tiles(d, w, b):
    """Float32 F(2x2, 3x3) of input tiles d (T, cin, 4, 4): V = B^T d B, M = sum over channels (in order) of V * U with the float32
    U = G g G^T, Y = A^T M A, + bias, ReLU.  Every operation a rounded float32 one.  -> (T, cout, 2, 2)"""
    d = np.ascontiguousarray(d, np.float32)
    v = _bt_rows(_bt_rows(d, 2), 3)                              # (T, cin, 4, 4)
    u = wino_filter_f32(w)                                       # (cin, 4, 4, cout)
    m = np.zeros((d.shape[0], 4, 4, u.shape[3]), np.float32)
    for c in range(d.shape[1]):
        m += v[:, c, :, :, None] * u[c][None]
    y = _at_rows(_at_rows(m, 1), 2)                              # (T, 2, 2, cout)
    y = np.maximum(y + b.astype(np.float32)[None, None, None, :], np.float32(0))
    return y.transpose(0, 3, 1, 2)


def sample_wino(rng, n, o, count_tiles):
    """Output tiles of an (n, o, o) block of 3 x 3 outputs -> (segment, tile y, tile x) of the sampled tiles."""
    th = (o + 1) // 2
    return sample_positions(rng, n, th, th, count_tiles)


def wino_positions(ni, ty, tx, o):
    """The output positions of sampled tiles that lie in the o x o block: (tile index, a, b) and (segment, y, x)."""
    t, a, b = np.meshgrid(np.arange(len(ni)), np.arange(2), np.arange(2), indexing="ij")
    t, a, b = t.ravel(), a.ravel(), b.ravel()
    y, x = 2 * ty[t] + a, 2 * tx[t] + b
    ok = (y < o) & (x < o)
    return (t[ok], a[ok], b[ok]), (ni[t[ok]], y[ok], x[ok])


# ------------------------------------------------------------------ error statistics and the criterion
def err_stats(got, ref):
    """(max, rms) of got - ref relative to max |ref| (1 where the reference is all zero)."""
    ref = np.asarray(ref, np.float64)
    e = np.asarray(got, np.float64) - ref
    scale = float(np.abs(ref).max()) or 1.0
    return float(np.abs(e).max()) / scale, float(np.sqrt(np.mean(e * e))) / scale


def within(kernel, yard, factor=FACTOR):
    """The layer-2 criterion on two (max, rms) pairs."""
    return kernel[0] <= factor * yard[0] and kernel[1] <= factor * yard[1]


def ratios(kernel, yard):
    return tuple(k / y if y > 0 else (0.0 if k == 0 else float("inf")) for k, y in zip(kernel, yard))


# ------------------------------------------------------------------ exact-integer input families
INT_FAMILIES = ("narrow", "wide_act", "wide_both")


def int_weights(rng, family, cout, cin, k, wino=False):
    """narrow: |w| <= 8 dense, every (output, channel, tap) its own draw.  wide_act: {+-1, +-2} on three reduction indices per output, zero
    elsewhere.  wide_both: |w| < 2**11 on two.  wino: multiples of 4 (G g G^T integral); the wide families then sit on the centre tap,
    whose transform is +-w / 4 on four positions, so that the activations keep the width that tells the split variants apart."""
    K = cin * k * k
    if family == "narrow":
        w = rng.integers(-8, 9, size=(cout, K))
    else:
        nz = 3 if family == "wide_act" else 2
        w = np.zeros((cout, K), np.int64)
        slots = np.arange(cin) * k * k + (k * k) // 2 if wino else np.arange(K)
        for o in range(cout):
            at = rng.choice(slots, size=nz, replace=False)
            mag = rng.integers(1, 3, size=nz) if family == "wide_act" else rng.integers(2 ** 10, 2 ** 11, size=nz)
            w[o, at] = mag * rng.choice([-1, 1], size=nz)
    return ((4 if wino else 1) * w).reshape(cout, cin, k, k).astype(np.float32)


def int_activations(rng, family, shape, bits, signed):
    hi = start_bits(family) if bits is None else bits
    x = rng.integers(0, 2 ** hi, size=shape)
    if signed:
        x = x * rng.choice([-1, 1], size=shape)
    return x.astype(np.float32)


def start_bits(family):
    return {"narrow": 8, "wide_act": 21, "wide_both": 11}[family]


def int_case(rng, family, signed, x_shape, cout, k, bound, wino=False):
    """(x, w, b, bits, bound value): integer inputs of `family` whose activations were narrowed one bit at a time until bound(x, w, b) --
    an upper bound, computed in float64, of every partial sum a correct kernel can form -- is below 2**24."""
    w = int_weights(rng, family, cout, x_shape[1], k, wino)
    b = rng.integers(-100, 101, size=(cout,)).astype(np.float32)
    bits = start_bits(family)
    while True:
        x = int_activations(rng, family, x_shape, bits, signed)
        v = bound(x, w, b)
        if v < LIMIT:
            return x, w, b, bits, v
        bits -= 1
        assert bits >= 2, "no activation width satisfies the bound"


def direct_bound(xin, w, b, stride=1):
    """max over outputs of sum |x| |w| + |b|: every partial sum of the reduction, in any order and through any exact split of the
    operands, is an integer no larger."""
    y = torch.nn.functional.conv2d(torch.from_numpy(np.abs(xin)).double(), torch.from_numpy(np.abs(w)).double(), stride=stride)
    return float(y.max()) + float(np.abs(b).max())


def wino_bound(x, w, b):
    """The same for F(2x2, 3x3): max of |B^T| |d| |B| (input transform), of sum_c (|B^T| |d| |B|) |G g G^T| (products) and of
    |A^T| (sum_c ...) |A| + |b| (output transform); asserts G g G^T integral."""
    u = np.einsum("ak,oikl,bl->oiab", G, np.asarray(w, np.float64), G)
    assert np.array_equal(u, np.round(u)), "G g G^T is not integral: the weights must be multiples of 4"
    n, c, t, _ = x.shape
    xp = torch.zeros((n, c, t + 1, t + 1), dtype=torch.float64)
    xp[:, :, :t, :t] = torch.from_numpy(np.abs(x)).double()
    th = (t - 2 + 1) // 2
    d = torch.nn.functional.unfold(xp[:, :, :2 * th + 2, :2 * th + 2], 4, stride=2).reshape(n, c, 4, 4, -1)
    ab, aa = torch.from_numpy(np.abs(BT)), torch.from_numpy(np.abs(AT))
    v = torch.einsum("ai,ncijl,bj->ncabl", ab, d, ab)
    m = torch.einsum("ncabl,ocab->noabl", v, torch.from_numpy(np.abs(u)))
    y = torch.einsum("ya,noabl,xb->noyxl", aa, m, aa)
    return max(float(v.max()), float(y.max()) + float(np.abs(b).max()))


# ------------------------------------------------------------------ random input families (layer 2)
FAMILIES = ("normal", "relu3", "range1e4", "bias10", "zero_segment")


def random_case(g, family, x_shape, cout, k):
    """Seeded CPU inputs: x (n, cin, h, w), He-scaled w (cout, cin, k, k), b (cout,) as float32 torch tensors.
    normal: N(0, 1).  relu3: 3 relu(N(0, 1)) (no cancellation).  range1e4: every activation times 10**U(-2, 2).  bias10: the bias ten
    times the products' scale.  zero_segment: the middle segment all zero (its outputs are relu(bias) exactly)."""
    cin = x_shape[1]
    x = torch.randn(x_shape, generator=g)
    if family == "relu3":
        x = torch.relu(x) * 3.0
    if family == "range1e4":
        x = x * torch.pow(10.0, torch.rand(x_shape, generator=g) * 4.0 - 2.0)
    w = torch.randn((cout, cin, k, k), generator=g) * (2.0 / (cin * k * k)) ** 0.5
    b = torch.randn((cout,), generator=g) * 0.3
    if family == "bias10":
        b = torch.randn((cout,), generator=g) * 10.0 * float(x.abs().mean()) * 2.0 ** 0.5
    if family == "zero_segment":
        x[x_shape[0] // 2] = 0.0
    return x.contiguous(), w.contiguous(), b.contiguous()


# ------------------------------------------------------------------ split-bf16 products on the CPU ("the test tests")
def bf16_round(a):
    """float32 -> the nearest bf16 (ties to even), returned as float32."""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def bf16_split(a, parts):
    out, rest = [], np.ascontiguousarray(a, np.float32)
    for _ in range(parts):
        p = bf16_round(rest)
        out.append(p)
        rest = rest - p                     # exact: the remainder of a round-to-nearest part fits float32
    return out


def split_accumulate(a, w, parts=3, keep=lambda i, j: i + j < 3):
    """a w^T as a split-bf16 kernel forms it: both operands split into `parts` bf16 parts, the part products (i, j) that `keep`
    admits (each exact in float32) accumulated in float32 in reduction order.  parts = 3 with i + j < 3 is the correct kernel (six
    products); parts = 3 with i + j < 2 drops three of them; parts = 2 is the two-way split with its four products."""
    ap, wp = bf16_split(a, parts), bf16_split(w, parts)
    pairs = [(i, j) for i in range(parts) for j in range(parts) if keep(i, j)]
    acc = np.zeros((a.shape[0], w.shape[0]), np.float32)
    for k in range(a.shape[1]):
        for i, j in pairs:
            acc += ap[i][:, k:k + 1] * wp[j][None, :, k]
    return acc


def split_product(a, w, b, **variant):
    """relu(a w^T + b) on split_accumulate."""
    return np.maximum(split_accumulate(a, w, **variant) + b.astype(np.float32)[None, :], np.float32(0))


def split_wino_tiles(d, w, b, **variant):
    """wino_f32_tiles with the sixteen per-position products V U formed by split_accumulate: what the split-bf16 Winograd kernel
    computes (V = B^T d B in float32, then split; U = G g G^T rounded to float32, then split)."""
    d = np.ascontiguousarray(d, np.float32)
    v = _bt_rows(_bt_rows(d, 2), 3)                              # (T, cin, 4, 4)
    u = wino_filter_f32(w)                                       # (cin, 4, 4, cout)
    m = np.zeros((d.shape[0], 4, 4, u.shape[3]), np.float32)
    for p in range(4):
        for q in range(4):
            m[:, p, q, :] = split_accumulate(np.ascontiguousarray(v[:, :, p, q]), np.ascontiguousarray(u[:, p, q, :].T), **variant)
    y = _at_rows(_at_rows(m, 1), 2)
    y = np.maximum(y + b.astype(np.float32)[None, None, None, :], np.float32(0))
    return y.transpose(0, 3, 1, 2)


SPLIT_VARIANTS = {
    "correct": dict(parts=3, keep=lambda i, j: i + j < 3),
    "dropped": dict(parts=3, keep=lambda i, j: i + j < 2),
    "two_way": dict(parts=2, keep=lambda i, j: True),
}

# reduction length -> outputs of the Fire modules' convolutions (squeezes, expand1x1s, 3 x 3 expands as 9 cin) and of conv1
FIRE_SHAPES = [(96, 16), (128, 16), (128, 32), (256, 32), (256, 48), (384, 48), (384, 64), (512, 64), (16, 64), (32, 128), (48, 192), (64, 256),
               (144, 64), (288, 128), (432, 192), (576, 256), (147, 96)]
