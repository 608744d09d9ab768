"""numpy restatement of the dropout head of include/swk.h (swk_nhwc_head2_dropout_relu_mean), written from the header's text:

    Philox4x32-10, standard constants;  key = (seed & 0xffffffff, seed >> 32);
    counter = (p * (c / 4) + ch / 4, s >> 5, segment key & 0xffffffff, segment key >> 32);
    m(s, p, ch) = bit (s & 31) of output word (ch & 3); kept when the bit is 1;
    out[n][s][k] = (sum_p max(sum_ch 2 m f w[k][ch] + bias[k], 0)) / n_pos,  f = x at the live positions, bg elsewhere.

tests/test_dropout_mask_cpu.py checks the generator against the published known-answer vectors; the GPU tests use head_reference."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """counter: four broadcastable integer arrays (each < 2**32), key: two ints -> four uint32 arrays."""
    c0, c1, c2, c3 = np.broadcast_arrays(*[np.asarray(c, dtype=np.uint64) for c in counter])
    k0, k1 = int(key[0]) & MASK32, int(key[1]) & MASK32
    for _ in range(10):
        p0 = c0 * np.uint64(M0)
        p1 = c2 * np.uint64(M1)
        h0, l0 = p0 >> np.uint64(32), p0 & np.uint64(MASK32)
        h1, l1 = p1 >> np.uint64(32), p1 & np.uint64(MASK32)
        c0, c1, c2, c3 = h1 ^ c1 ^ np.uint64(k0), l1, h0 ^ c3 ^ np.uint64(k1), l0
        k0, k1 = (k0 + W0) & MASK32, (k1 + W1) & MASK32
    return tuple(c.astype(np.uint32) for c in (c0, c1, c2, c3))


def mask_words(seed, key, n_pos, c, blocks):
    """uint32 [blocks][n_pos][c]: the word whose bit (s & 31) is the mask of sample s = 32 * block + (s & 31) at (position, channel)."""
    seed, key = int(seed) & (2 ** 64 - 1), int(key) & (2 ** 64 - 1)
    quad = np.arange(n_pos, dtype=np.uint64)[:, None] * np.uint64(c // 4) + np.arange(c // 4, dtype=np.uint64)[None, :]
    blk = np.arange(blocks, dtype=np.uint64)[:, None, None]
    words = philox4x32_10((quad[None], blk, key & MASK32, key >> 32), (seed & MASK32, seed >> 32))
    return np.stack(words, axis=-1).reshape(blocks, n_pos, c)


def mask(seed, key, samples, n_pos, c):
    """bool [samples][n_pos][c]: True = kept."""
    words = mask_words(seed, key, n_pos, c, (samples + 31) // 32)
    s = np.arange(samples)
    return ((words[s >> 5] >> (s & 31).astype(np.uint32)[:, None, None]) & np.uint32(1)).astype(bool)


def features(x, pos, bg, n_pos):
    """x [n][px][c] at positions pos, bg [n_pos][c] (or None) elsewhere -> float64 [n][n_pos][c]."""
    x = np.asarray(x, dtype=np.float64)
    n, px, c = x.shape
    f = np.zeros((n, n_pos, c)) if bg is None else np.broadcast_to(np.asarray(bg, dtype=np.float64), (n, n_pos, c)).copy()
    f[:, np.asarray(pos, dtype=np.int64)] = x
    return f


def head_reference(x, pos, bg, n_pos, w, bias, keys, seed, samples):
    """The header's formula in float64 -> [n][samples][2]."""
    f = features(x, pos, bg, n_pos)
    w2 = 2.0 * np.asarray(w, dtype=np.float64).reshape(2, -1)
    b = np.asarray(bias, dtype=np.float64).reshape(2)
    out = np.empty((f.shape[0], samples, 2))
    for i in range(f.shape[0]):
        m = mask(seed, keys[i], samples, n_pos, f.shape[2])
        for k in range(2):
            pre = np.where(m, (f[i] * w2[k])[None], 0.0).sum(axis=2) + b[k]          # [samples][n_pos]
            out[i, :, k] = np.maximum(pre, 0.0).sum(axis=1) / n_pos
    return out
