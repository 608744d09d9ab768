"""BGR -> grey on every (B, G, R) triple, through every copy of the arithmetic and every load branch an entry point reaches, in both
grey modes, against numpy in int64:  (1868 B + 9617 G + 4899 R + 2^13) >> 14  and  (3735 B + 19235 G + 9798 R + 2^14) >> 15.

All 2^24 triples, each once, in a seeded permutation (neighbouring pixels are unrelated), laid out as the case needs them:

  filters.hip k_gray4, dword loads   swk_bgr2gray on 64 x 512 x 512 (dense rows of a width that is a multiple of 4: every quad of
                                     a row starts on a dword); the batch call on an already-cut ROI
  filters.hip k_gray4, byte loads    NOT reachable through swk_bgr2gray: it uploads the pixels densely, so with W % 4 == 0 every
                                     quad is 12 W r + 12 q bytes from a dword-aligned base.  Reached by the batch call that reads
                                     full frames on the device in place with an odd x0 and a row stride of 777 bytes: the first
                                     byte of a row's ROI takes every residue mod 4 (the rows on residue 0 take the dword loads at
                                     an offset)
  filters.hip k_gray4g               swk_bgr2gray at width 511: a partial last quad of three pixels, rows (and their stores) on
                                     every alignment in turn, the aligned full quads by dwords, the others by bytes.  2^24 is no
                                     multiple of 511: the last row is filled with zeros, which are compared as well
  groups.hip k_gray_groups           one groups call of two groups of different geometry, one half of the triples each: device
                                     frames with an odd origin and an odd row stride, and a dense host ROI
  stabilize.hip k_stab_gray          swk_stabilize_u8 with S = 0, the rectangle the whole frame and the anchor the numpy grey of
                                     that frame: sad == sad_unshifted == 0, and a sum of absolute differences is zero only if
                                     every pixel agrees.  Dense device rows (dword loads) and a row stride of 1537 bytes (byte
                                     loads wherever the row does not start on a dword).  Control: one anchor pixel off by one
                                     gives a sum of exactly 1
  filters.hip k_gray (3 channels)    not reachable: launch_gray sends every three-channel call to k_gray4 or k_gray4g

and the anchor that stabilize.StabilizingReader makes with bgr2gray matches its own frame at shift (0, 0) with a sum of 0."""
import numpy as np
import pytest

import stabilize_ref as ref

pytestmark = pytest.mark.gpu

COUNT = 1 << 24
F, H, W = 64, 512, 512                   # the stack of the dense cases
FB, HB, WB, NB = 256, 256, 256, 16       # the batch calls: 16 windows of 16 frames of 256 x 256
W_ODD, H_ODD, F_ODD = 511, 4691, 7       # 7 x 4691 x 511 = 16 779 707 >= 2^24
MODES = [0, 1]


@pytest.fixture(scope="module")
def ctx():
    from swiftwatcher_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def triples():
    """(2^24, 3) uint8: every triple once"""
    v = np.random.default_rng(20240607).permutation(COUNT).astype(np.uint32)
    t = np.empty((COUNT, 3), np.uint8)
    t[:, 0], t[:, 1], t[:, 2] = v & 255, (v >> 8) & 255, v >> 16
    t.setflags(write=False)
    return t


def numpy_gray(t, mode):
    b, g, r = (t[..., k].astype(np.int64) for k in range(3))
    y = (1868 * b + 9617 * g + 4899 * r + (1 << 13)) >> 14 if mode == 0 else (3735 * b + 19235 * g + 9798 * r + (1 << 14)) >> 15
    assert y.min() >= 0 and y.max() <= 255
    return y.astype(np.uint8)


@pytest.fixture(scope="module")
def gray(triples):
    out = {mode: numpy_gray(triples, mode) for mode in MODES}
    for a in out.values():
        a.setflags(write=False)
    return out


def params(mode):
    from swiftwatcher_amd import _lib
    return _lib.default_params(gray_mode=mode, maxiter=1)


def assert_gray(got, want, label):
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    assert got.shape == want.shape, label
    bad = np.nonzero(got != want)[0]
    assert not len(bad), "%s: %d pixels differ, first at %d: %d, expected %d" % (label, len(bad), bad[0], got[bad[0]], want[bad[0]])


def test_the_reference(triples, gray):
    packed = triples[:, 0].astype(np.int64) | (triples[:, 1].astype(np.int64) << 8) | (triples[:, 2].astype(np.int64) << 16)
    assert np.array_equal(np.sort(packed), np.arange(COUNT))                                  # every triple, once
    assert (packed[1:] - packed[:-1] == 1).mean() < 1e-3                                      # and not in order
    b, g, r = (triples[:, k].astype(np.float64) for k in range(3))
    # floor(x / 2^k + 0.5) in float64: the sums are integers below 2^23 and the division is by a power of two, so this is exact
    assert np.array_equal(np.floor((1868 * b + 9617 * g + 4899 * r) / 2.0 ** 14 + 0.5), gray[0].astype(np.float64))
    assert np.array_equal(np.floor((3735 * b + 19235 * g + 9798 * r) / 2.0 ** 15 + 0.5), gray[1].astype(np.float64))
    assert 1868 + 9617 + 4899 == 1 << 14 and 3735 + 19235 + 9798 == 1 << 15
    for mode in MODES:
        assert np.array_equal(ref.gray(triples[:4096], mode), gray[mode][:4096])              # the restatement the stabilization tests use
    assert (gray[0] != gray[1]).sum() > 1000                                                   # the modes are two functions


# ---- swk_bgr2gray -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_bgr2gray_dense_rows_of_a_multiple_of_four(ctx, triples, gray, mode):
    """k_gray4, dword loads (its byte loads are out of this entry point's reach: see the module's text)"""
    assert W % 4 == 0
    assert_gray(ctx.bgr2gray(triples.reshape(F, H, W, 3), mode), gray[mode], "k_gray4")


@pytest.mark.parametrize("mode", MODES)
def test_bgr2gray_odd_width(ctx, triples, gray, mode):
    """k_gray4g: W = 511"""
    total = F_ODD * H_ODD * W_ODD
    assert W_ODD % 4 == 3 and COUNT <= total < COUNT + W_ODD * F_ODD
    src = np.zeros((total, 3), np.uint8)
    src[:COUNT] = triples
    want = np.zeros(total, np.uint8)
    want[:COUNT] = gray[mode]
    assert_gray(ctx.bgr2gray(src.reshape(F_ODD, H_ODD, W_ODD, 3), mode), want, "k_gray4g")


# ---- the batch calls ----------------------------------------------------------------------------------------------------------------
def framed(pixels, frames, top, left, bottom, right):
    """(frames, HB, WB, 3) pixels inside larger frames whose other bytes are 255 -> (the larger array, crop (x0, y0, Wc, Hc))"""
    h, w = pixels.shape[1:3]
    big = np.full((frames, top + h + bottom, left + w + right, 3), 255, np.uint8)
    big[:, top:top + h, left:left + w] = pixels
    return big, (left, top, w, h)


@pytest.mark.parametrize("mode", MODES)
def test_batch_call_from_full_frames_with_an_odd_origin(ctx, triples, gray, mode):
    """device frames read in place: x0 = 1, rows 777 bytes apart -- k_gray4's byte loads, and its dword loads on every fourth row"""
    import torch
    big, crop = framed(triples.reshape(FB, HB, WB, 3), FB, 1, 1, 1, 2)
    assert big.strides[1] == 777 and {(3 * crop[0] + r * 777) % 4 for r in range(4)} == {0, 1, 2, 3}
    dev = torch.from_numpy(big).cuda()
    assert dev.data_ptr() % 4 == 0
    res = ctx.batch_run(dev, FB // NB, NB, crop=crop, params=params(mode), stages=("gray",))
    assert_gray(res["gray"], gray[mode], "batch call, full frames")


@pytest.mark.parametrize("mode", MODES)
def test_batch_call_from_a_cut_roi(ctx, triples, gray, mode):
    res = ctx.batch_run(triples.reshape(FB, HB, WB, 3), FB // NB, NB, params=params(mode), stages=("gray",))
    assert_gray(res["gray"], gray[mode], "batch call, cut ROI")


@pytest.mark.parametrize("mode", MODES)
def test_groups_call(ctx, triples, gray, mode):
    """k_gray_groups: group 0 = the first half as 128 device frames of 256 x 256 inside 258 x 259 (odd origin, odd row stride), group 1
    = the second half as 256 dense host frames of 128 x 256"""
    import torch
    half = COUNT // 2
    big, crop = framed(triples[:half].reshape(FB // 2, HB, WB, 3), FB // 2, 1, 1, 1, 2)
    dev = torch.from_numpy(big).cuda()
    groups = [dict(frames=dev, nwin=FB // 2 // NB, n=NB, crop=crop),
              dict(frames=triples[half:].reshape(FB, HB // 2, WB, 3), nwin=FB // NB, n=NB)]
    got = ctx.batch_run_groups(groups, params=params(mode), stages=("gray",))
    assert got[0]["gray"].shape == (FB // 2, HB, WB) and got[1]["gray"].shape == (FB, HB // 2, WB)
    assert_gray(got[0]["gray"], gray[mode][:half], "groups call, group 0")
    assert_gray(got[1]["gray"], gray[mode][half:], "groups call, group 1")


# ---- swk_stabilize_u8 -----------------------------------------------------------------------------------------------------------------
def stab_sads(ctx, dev, anchors, mode):
    """sad and sad_unshifted of every frame of the device tensor (F, H, W, 3) against its own anchor, S = 0, the whole frame"""
    out = []
    for f in range(dev.shape[0]):
        shifts, _, pixels = ctx.stabilize(dev[f:f + 1], (0, 0, H, W), 0, anchors[f], gray_mode=mode, device_out=True)
        s = shifts[0]
        assert (int(s["dy"]), int(s["dx"])) == (0, 0)
        out.append((int(s["sad"]), int(s["sad_unshifted"])))
    return out


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("rows", ["dword_rows", "odd_row_stride"])
def test_stab_gray_through_the_shift_search(ctx, triples, gray, mode, rows):
    import torch
    stack = triples.reshape(F, H, W, 3)
    if rows == "dword_rows":
        dev = torch.from_numpy(stack.copy()).cuda()          # (a copy: torch takes no read-only array)
        assert dev.stride(1) % 4 == 0 and dev.data_ptr() % 4 == 0
    else:
        wide = np.full((F, H, 3 * W + 1), 255, np.uint8)
        wide[:, :, :3 * W] = stack.reshape(F, H, 3 * W)
        dev = torch.from_numpy(wide).cuda().as_strided((F, H, W, 3), (H * (3 * W + 1), 3 * W + 1, 3, 1))
        assert dev.stride(1) == 1537
    anchors = gray[mode].reshape(F, H, W)
    assert stab_sads(ctx, dev, anchors, mode) == [(0, 0)] * F
    # control: one pixel of one anchor off by one
    f, r, c = 37, 129, 258
    off = anchors[f].copy()
    off[r, c] += 1 if off[r, c] < 255 else -1
    assert stab_sads(ctx, dev[f:f + 1], [off], mode) == [(1, 1)]


@pytest.mark.parametrize("mode", MODES)
def test_the_readers_anchor_matches_its_own_frame(ctx, triples, mode):
    """StabilizingReader makes its anchor with bgr2gray (k_gray4 or k_gray4g) and matches it against planes of k_stab_gray: on the
    first frame itself the best shift is (0, 0) with a sum of 0, at a search range of 8 (every other candidate is another noise
    picture)"""
    from swiftwatcher_amd.io_frames import ArrayReader
    from swiftwatcher_amd.stabilize import StabilizingReader
    frame = triples.reshape(F, H, W, 3)[5 + mode]
    for crop_region in ([(101, 75), (101 + 95, 75 + 63)], [(64, 64), (64 + 96, 64 + 64)]):          # margin rectangles 119 and 120 wide
        reader = StabilizingReader(ArrayReader([frame], fps=30.0), crop_region, 8, (24, 24), gray_mode=mode, backend=ctx)
        frames, numbers, _ = reader.get_n_frames(2)
        assert list(numbers) == [0, 1] and reader.shifts[0] == (0, 0, 0, 0) and reader.shifts[1] == (0, 0, 0, 0)
        (x0, y0), (x1, y1) = crop_region
        assert np.array_equal(frames[0][y0:y1, x0:x1], frame[y0:y1, x0:x1])
