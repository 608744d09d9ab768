"""The dropout mask of swk_nhwc_head2_dropout_relu_mean as include/swk.h defines it, restated in numpy (tests/dropout_ref.py): the
generator against the published Philox4x32-10 known-answer vectors, and the mask's statistics on the network's own 169 x 512 map.
No GPU: the GPU tests (tests/test_dropout_head_gpu.py) hold the kernel to this restatement."""
import numpy as np

import dropout_ref as D

N_POS, C = 169, 512
_POP = np.array([bin(v).count("1") for v in range(256)], dtype=np.uint8)


def _bits(words):
    return int(_POP[np.ascontiguousarray(words).view(np.uint8)].sum(dtype=np.int64))


def _within(ones, n, what):
    """The share of ones among n fair bits: 0.5 +- 5 sigma of the binomial (sigma = 0.5 / sqrt(n)), worked out here."""
    bound = 5.0 * 0.5 / np.sqrt(float(n))
    share = ones / float(n)
    print("%s: share %.6f of %d bits, bound 0.5 +- %.2e" % (what, share, n, bound))
    assert abs(share - 0.5) <= bound, (what, share, bound)


def test_philox4x32_10_known_answers():
    """Random123's kat_vectors for philox4x32 with 10 rounds (Salmon, Moraes, Dror, Shaw: Parallel Random Numbers: As Easy as 1, 2, 3,
    SC'11): counter and key all zero, all ones, and the digits of pi."""
    kat = (((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)))
    for ctr, key, want in kat:
        assert tuple(int(v) for v in D.philox4x32_10(ctr, key)) == want, (ctr, key)
    # vectorised over counters: the same words as one call each
    c0 = np.array([0, 0x243f6a88, 7], dtype=np.uint64)
    got = D.philox4x32_10((c0, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0))
    assert tuple(int(g[1]) for g in got) == kat[2][2]
    assert tuple(int(g[0]) for g in got) != tuple(int(g[2]) for g in got)


def test_mask_layout_follows_the_header():
    """mask(s, p, ch) = bit (s & 31) of word (ch & 3) of the call with counter (p c/4 + ch/4, s >> 5, key lo, key hi), key = the seed."""
    seed, key = 0x0123456789abcdef, 0xfedcba9876543210
    m = D.mask(seed, key, 70, N_POS, C)
    assert m.shape == (70, N_POS, C) and m.dtype == bool
    for s, p, ch in ((0, 0, 0), (31, 168, 511), (32, 5, 6), (69, 100, 257), (33, 1, 3)):
        words = D.philox4x32_10((p * (C // 4) + ch // 4, s >> 5, key & 0xffffffff, key >> 32), (seed & 0xffffffff, seed >> 32))
        assert bool(m[s, p, ch]) == bool((int(words[ch & 3]) >> (s & 31)) & 1), (s, p, ch)
    # the mask of a sample does not depend on how many samples are taken
    assert np.array_equal(D.mask(seed, key, 33, N_POS, C), m[:33])


def test_kept_share_and_independence_of_keys_seeds_and_samples():
    """Seed 0, 64 keys of the form (frame << 8) | label, 64 samples, the 169 x 512 map: half the values are kept, and the masks of two
    keys, of two seeds and of two samples differ in half their bits -- each within 5 sigma of the binomial for its number of bits."""
    keys = [((1000 + 3 * i) << 8) | (1 + i % 5) for i in range(63)] + [(-1 << 8 | 2) & (2 ** 64 - 1)]         # a null frame's among them
    words = np.stack([D.mask_words(0, k, N_POS, C, 2) for k in keys])                # [64][2][169][512]: 64 samples in two words
    per_key = words[0].size * 32
    _within(_bits(words), len(keys) * per_key, "kept share, seed 0")
    for a, b in ((0, 1), (5, 6), (62, 63)):
        _within(_bits(words[a] ^ words[b]), per_key, "keys %d and %d" % (a, b))
    other = np.stack([D.mask_words(1, k, N_POS, C, 2) for k in keys[:4]])
    _within(_bits(words[:4] ^ other), 4 * per_key, "seeds 0 and 1")
    far = D.mask_words(1 << 32, keys[0], N_POS, C, 2)
    _within(_bits(words[0] ^ far), per_key, "seeds 0 and 2**32")
    w = words[:, 0]                                                                   # samples 0..31
    n = w.size
    for s, t in ((0, 1), (7, 31), (0, 16)):
        diff = ((w >> np.uint32(s)) ^ (w >> np.uint32(t))) & np.uint32(1)
        _within(int(diff.sum(dtype=np.int64)), n, "samples %d and %d" % (s, t))
    diff = (words[:, 0] ^ words[:, 1]) & np.uint32(1)                                  # samples 0 and 32: two generator calls
    _within(int(diff.sum(dtype=np.int64)), n, "samples 0 and 32")


def test_segment_keys():
    """(parent frame number << 8) | label as uint64, two's complement for null frames."""
    from swiftwatcher_amd.data_structures import segment_keys
    k = segment_keys([0, 5, 123456, -1], [1, 2, 255, 3])
    assert k.dtype == np.uint64
    assert [int(v) for v in k] == [1, (5 << 8) | 2, (123456 << 8) | 255, (2 ** 64 - 256) | 3]


def test_batch_keys_follow_the_batch_order():
    """batch_keys: frames in the batch's order, per frame the live records' labels ascending; records beyond nseg do not count."""
    from swiftwatcher_amd import _lib
    from swiftwatcher_amd.data_structures import batch_keys, segment_keys
    segs = np.zeros((3, 4), _lib.SEGMENT_DTYPE)
    segs["label"] = [[1, 2, 3, 9], [1, 9, 9, 9], [9, 9, 9, 9]]
    nseg = np.array([3, 1, 0], np.int32)
    k = batch_keys(segs, nseg, (20, 19, -1))
    assert np.array_equal(k, segment_keys([20, 20, 20, 19], [1, 2, 3, 1]))
    assert batch_keys(segs, np.zeros(3, np.int32), (20, 19, -1)).shape == (0,)
