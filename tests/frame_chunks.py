"""Frames, windows and the inventory for the size-edge tests: tests/test_frame_chunks_cpu.py, tests/test_frame_chunks_gpu.py and
tests/test_far_offsets_gpu.py.  No GPU in here.

Periodic stacks.  Every launcher of the image stages splits its frames into launches of CHUNK = 32768 (a grid's y / z extent is
limited) and advances its per-frame arrays by f0 per launch.  A forgotten advance gives right results for frames 0..32767 and frame
0's results again from frame 32768 on.  The tests therefore run F1 = 32768 + 37 frames (two launches, the second ragged) or F2 =
2 * 32768 + 5 frames (three launches: the middle one has f0 > 0 and a full count) in which frame f is distinct frame f % K, K = 37: 37
is coprime to 32768 and to every window length used, so launch and window boundaries fall at every phase of the period.  The
expected output is the K distinct results tiled -- first the entry point's own results on the K frames in a lone call, then the CPU
restatement of the stage on those K.  A stale f0 can only go unseen where two frames' OUTPUTS are equal: assert_distinct() refuses a
generator whose K expected outputs are not pairwise different.

Sizing rule.  No call of these tests moves more than 64 MB between host and device (SIZES below gives every call's larger
direction at its frame count), with one exception that is device-only and accepted: the shape-sum table of swk_segment_shapes_u8,
F x 256 x 17 x 8 bytes = 1.1 GB at F1, which the library allocates and never copies.  seg_cap is 4 wherever records come back: 32805
x 255 records of 48 bytes would be 400 MB."""
import os
import re

import numpy as np

K = 37
CHUNK = 32768
F1 = CHUNK + 37
F2 = 2 * CHUNK + 5
SEG_CAP = 4
MB64 = 64 * 1000 * 1000

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "swiftwatcher_amd", "csrc")


# ------------------------------------------------------------------ periodic stacks
def periodic(stack_K, F):
    """frame f = distinct frame f % K"""
    a = np.asarray(stack_K)
    assert len(a) == K
    return np.ascontiguousarray(a[np.arange(F) % K])


def tile(expected_K, F):
    """the expected output of a periodic stack from the K distinct results (any array whose first axis is the frame)"""
    return periodic(expected_K, F)


def assert_distinct(expected_K, what=""):
    """the K results differ pairwise (as bytes): no frame's output could stand in for another's"""
    a = np.ascontiguousarray(expected_K)
    assert len(a) == K, what
    seen = {}
    for k in range(K):
        key = a[k].tobytes()
        assert key not in seen, "%s: distinct frames %d and %d have the same output" % (what, seen[key], k)
        seen[key] = k


def assert_differs_across_launches(expected_K, what=""):
    """The weaker rule for outputs of a few bytes a frame (a count cannot take 37 values everywhere): a launch c = 1, 2 that read the
    first launch's slice would hand frame f the result of frame f - c * 32768; that one, at least, differs from frame f's own."""
    a = np.ascontiguousarray(expected_K)
    assert len(a) == K, what
    for c in (1, 2):
        for k in range(K):
            j = (k - c * CHUNK) % K
            assert a[k].tobytes() != a[j].tobytes(), "%s: distinct frames %d and %d (launch %d's stale twin) have the same output" % (what, k, j, c)


def assert_outputs_tell_frames_apart(expected_K, what=""):
    """assert_distinct for an output of 8 bytes a frame and more, assert_differs_across_launches below that"""
    a = np.ascontiguousarray(expected_K)
    if a[0].nbytes >= 8:
        assert_distinct(a, what)
    else:
        assert_differs_across_launches(a, what)


def assert_periodic(got, expected_K, what=""):
    """got[f] == expected_K[f % K] for every frame, bit for bit; names the first frame that differs and its launch"""
    got = np.asarray(got)
    want = np.asarray(expected_K)
    assert got.shape[1:] == want.shape[1:] and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    F = len(got)
    full = tile(want, F)
    if got.dtype.names:
        bad = np.nonzero((got != full).reshape(F, -1).any(axis=1))[0]
    else:
        bad = np.nonzero((got.reshape(F, -1) != full.reshape(F, -1)).any(axis=1))[0]
    assert not len(bad), "%s: %d of %d frames differ, the first is frame %d (launch %d, f0 = %d, distinct frame %d)" % (
        what, len(bad), F, bad[0], bad[0] // CHUNK, bad[0] // CHUNK * CHUNK, bad[0] % K)


def stale_second_chunk(expected_K, F):
    """host stand-in for a launcher that forgot `+ f0` on a per-frame array: from frame 32768 on, every launch reads what the
    first launch read"""
    idx = np.arange(F)
    return np.ascontiguousarray(np.asarray(expected_K)[(idx % CHUNK) % K])


# ------------------------------------------------------------------ the K distinct frames of each stage
SHAPES_ODD = [(5, 7), (9, 13)]          # odd pixel counts: every vector-width fallback
SHAPE_ALIGNED = (8, 12)                 # the k_gray4 / 4-byte routes
SHAPE_BATCH = (12, 20)


def _rng(*key):
    import zlib
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def bgr_frames(H, W, seed=0):
    """(K, H, W, 3) noise"""
    return _rng("bgr", H, W, seed).integers(0, 256, size=(K, H, W, 3), dtype=np.uint8)


def gray_planes(H, W, seed=0):
    """(K, H, W) planes as the RPCA leaves them: a dark ground, bright smooth blobs of a level of the frame's own, noise of a few
    levels -- the bilateral filter, the threshold and the openings all leave something, and something else on every frame"""
    rng = _rng("gray", H, W, seed)
    out = np.empty((K, H, W), np.uint8)
    r, c = np.indices((H, W))
    for k in range(K):
        img = rng.integers(0, 12, size=(H, W)).astype(np.int64)
        for _ in range(2):
            cy, cx = rng.integers(0, H), rng.integers(0, W)
            hh, ww = rng.integers(2, max(3, H // 2 + 1)), rng.integers(2, max(3, W // 2 + 1))
            blob = (np.abs(r - cy) <= hh) & (np.abs(c - cx) <= ww)
            img[blob] += 40 + 5 * k + rng.integers(0, 6, size=int(blob.sum()))
        out[k] = np.clip(img, 0, 255)
    return out


def label_planes(H, W, seed=0):
    """(K, H, W) u8 label planes: distinct frame k holds the labels 1 .. k + 1, every one of them, scattered -- so the label COUNT of a
    frame is its own as well"""
    rng = _rng("labels", H, W, seed)
    assert H * W >= 2 * K
    out = np.zeros((K, H, W), np.uint8)
    for k in range(K):
        img = rng.integers(0, k + 2, size=(H, W)).astype(np.uint8)
        flat = img.reshape(-1)
        flat[rng.permutation(flat.size)[:k + 1]] = np.arange(1, k + 2)
        out[k] = img
    return out


def binary_planes(H, W, seed=0):
    """(K, H, W) foreground masks (0 / 255), density between a fifth and four fifths.  Each frame is drawn again until its component
    counts, 8- and 4-way (scipy), differ from those of the frames a launch's stale read would confuse it with (the frames 32768 and
    65536 places away in the period): assert_differs_across_launches holds for the counts."""
    from scipy import ndimage
    rng = _rng("binary", H, W, seed)
    out = np.zeros((K, H, W), np.uint8)
    counts = {}
    twins = sorted({(c * CHUNK) % K for c in (1, 2)} | {(-c * CHUNK) % K for c in (1, 2)})
    for k in range(K):
        for _ in range(1000):
            img = rng.random((H, W)) < 0.2 + 0.6 * k / (K - 1)
            n8, n4 = ndimage.label(img, np.ones((3, 3)))[1], ndimage.label(img)[1]
            if all(counts.get((k + t) % K, (None, None))[0] != n8 and counts.get((k + t) % K, (None, None))[1] != n4 for t in twins):
                break
        else:
            raise AssertionError("no mask for frame %d" % k)
        counts[k] = (n8, n4)
        out[k] = img * 255
    return out


# the 25 shifts of search 2, from the centre outwards: distinct frame k is moved by STAB_SHIFTS[k % 25]
STAB_S = 2
STAB_SHIFTS = sorted(((dy, dx) for dy in range(-STAB_S, STAB_S + 1) for dx in range(-STAB_S, STAB_S + 1)),
                     key=lambda s: (s[0] * s[0] + s[1] * s[1], s))


def stabilize_case(Ho=5, Wo=7, seed=0, margin=3):
    """(frames (K, Hs, Ws, 3), rect, anchor (Ho, Wo), shifts [(dy, dx)] * K): one textured scene; distinct frame k shows it moved by
    STAB_SHIFTS[k % 25] -- every shift of the search range is taken, twelve of them twice -- under noise and a brightness of its own, so
    that frames of equal shift still differ in every output.  The anchor is the grey of the unmoved scene."""
    import stabilize_ref
    rng = _rng("stab", Ho, Wo, seed)
    Hs, Ws = Ho + 2 * margin, Wo + 2 * margin
    M = STAB_S + 1
    scene = rng.integers(0, 256, size=(Hs + 2 * M, Ws + 2 * M, 3)).astype(np.float64)
    frames = np.empty((K, Hs, Ws, 3), np.uint8)
    shifts = []
    for k in range(K):
        dy, dx = STAB_SHIFTS[k % len(STAB_SHIFTS)]
        # the picture's rectangle at (y0 + dy, x0 + dx) shows what the unmoved picture shows at (y0, x0)
        pic = scene[M - dy:M - dy + Hs, M - dx:M - dx + Ws] * (0.9 + 0.005 * (k // len(STAB_SHIFTS))) + rng.normal(0.0, 1.0, size=(Hs, Ws, 3))
        frames[k] = np.clip(np.rint(pic), 0, 255)
        shifts.append((dy, dx))
    still = np.clip(np.rint(scene[M:M + Hs, M:M + Ws] * 0.9), 0, 255).astype(np.uint8)
    rect = (margin, margin, Ho, Wo)
    anchor = stabilize_ref.gray(still[margin:margin + Ho, margin:margin + Wo], 0)
    return frames, rect, anchor, shifts


def yuv420_planes(H, W, seed=0):
    """(y (K, H, W), u, v (K, ceil(H/2), ceil(W/2))) noise over the whole byte range"""
    rng = _rng("yuv", H, W, seed)
    ch, cw = (H + 1) // 2, (W + 1) // 2
    return (rng.integers(0, 256, size=(K, H, W), dtype=np.uint8), rng.integers(0, 256, size=(K, ch, cw), dtype=np.uint8),
            rng.integers(0, 256, size=(K, ch, cw), dtype=np.uint8))


# ---- windows of the batch calls: n = 3, 12 x 20 (and a second geometry for the groups call) ----
BATCH_N = 3
BATCH_NWIN = 10935                      # 10935 x 3 = 32805 = F1: frame 32768 is the third frame of window 10922
# At the reference's lmbda = 0.01 a window this small has an all-zero sparse image on every frame, whatever it shows: the shrinkage
# threshold lmbda / mu is so low against 1 / sqrt(pixels) that E takes the whole window, ground included, with a positive sign, and
# the u8 image keeps -E.  That holds up to ROIs of some 1 / lmbda^2 = 10^4 pixels, which 32805 frames cannot have under the 64 MB
# rule.  The batch tests therefore run at lmbda = 0.1 (1 / sqrt(240) = 0.065), where a dark bird on one frame of three stays in
# the sparse image and through the filters.
BATCH_LMBDA = 0.1
# seeds found by the search at the bottom of this file (python tests/frame_chunks.py): the K windows of each meet window_conditions()
WINDOW_SEEDS = {(12, 20): 0, (9, 14): 0}


def batch_windows(H, W, seed):
    """(K, 3, H, W, 3) BGR windows: a smooth ground that stays, noise of a level or two, and on most windows a dark bird on one of
    the three frames (position, size, depth and frame of the window's own), which the RPCA's sparse term keeps"""
    rng = _rng("window", H, W, seed)
    out = np.empty((K, BATCH_N, H, W, 3), np.uint8)
    r, c = np.indices((H, W))
    for k in range(K):
        ground = 150.0 + 20.0 * np.sin(r / (2.0 + k % 5) + k) * np.cos(c / (3.0 + k % 3))
        ground = ground[..., None] + rng.normal(0, 3.0, size=(H, W, 3))
        for j in range(BATCH_N):
            out[k, j] = np.clip(np.rint(ground + rng.normal(0, 1.0, size=(H, W, 3))), 0, 255)
        if k % 4 != 3:
            j = k % BATCH_N
            cy, cx = rng.integers(3, H - 3), rng.integers(3, W - 3)
            hh, ww = rng.integers(1, 3), rng.integers(2, 4)          # 3..5 rows by 5..7 columns
            bird = (np.abs(r - cy) <= hh) & (np.abs(c - cx) <= ww)
            out[k, j][bird] = np.clip(out[k, j][bird].astype(np.int64) - (70 + rng.integers(0, 40)), 0, 255)
    return out


def window_conditions(orc, windows):
    """The oracle's results of the K distinct windows and the two conditions on them: at least a third have a non-empty opened frame
    with a segment; no element of any window's E lies within ialm_trajectory_cases.BAND of a value where the u8 sparse image changes
    (cap: zero masked elements), so that a different Gram-slab count -- nblk depends on nwin -- cannot move a byte.
    Returns (refs, windows with segments, masked elements)."""
    import ialm_trajectory_cases as tc
    refs, with_segs, masked = [], 0, 0
    for w in windows:
        ref = orc.window(np.ascontiguousarray(w), lmbda=BATCH_LMBDA)
        n, H, Wd = ref["gray"].shape
        cols = np.transpose(ref["gray"].reshape(n, H * Wd))
        _, E = orc.ialm_defined(cols, lmbda=BATCH_LMBDA)
        masked += int(tc.boundary_mask(E, tc.BAND).sum())
        with_segs += bool(ref["opened"].any() and any(len(s) for s in ref["segments"]))
        refs.append(ref)
    return refs, with_segs, masked


# ------------------------------------------------------------------ sizing rule
# call: (frames, bytes per frame host -> device, bytes per frame device -> host)
SIZES = {
    "bgr2gray 8x12": (F2, 8 * 12 * 3, 8 * 12),
    "bgr2gray 9x13": (F2, 9 * 13 * 3, 9 * 13),
    "bilateral_u8 9x13": (F1, 9 * 13, 9 * 13),
    "grey_open3x3_u8 9x13": (F2, 9 * 13, 9 * 13),
    "grey_open_u8 9x13": (F1, 9 * 13, 9 * 13),
    "regionprops_u8 9x13": (F1, 9 * 13, SEG_CAP * 48 + 4),
    "segment_shapes_u8 9x13": (F1, 9 * 13, SEG_CAP * 144 + 4),
    "ccl_u8 9x13": (F1, 9 * 13, 9 * 13 * 4 + 4),
    "stabilize 5x7 in 11x13": (F1, 11 * 13 * 3, 5 * 7 * 3 + 24 + 25 * 8),
    "stabilize_subpel 5x7 in 11x13": (F1, 11 * 13 * 3, 5 * 7 * 3 + 40 + 25 * 8 + 25 * 8),
    "yuv420_to_bgr 10x14": (F1, 10 * 14 * 3 // 2, 9 * 11 * 3),
    "yuv_to_bgr 10x14 16-bit": (F1, 10 * 14 * 2 * 3 // 2, 9 * 11 * 3),
    "render_review 9x13": (F1, 9 * 13 * 3, 9 * 13 + 2 * 5 * 7),
    "render_review_panels 9x13, 3 cells": (F1, 9 * 13 * (3 + 2), 3 * (10 * 14) * 3 // 2),
    "debug_filter_fused 9x13": (F1, 9 * 13, 3 * 9 * 13),
    "batch_run 12x20": (F1, 12 * 20 * 3, 6 * 12 * 20 + SEG_CAP * 48 + 8),
    "batch_run single-channel 12x20, gray alone": (F2, 12 * 20, 12 * 20 + 48 + 8),
    "batch_run n = 1, 5x7": (70000, 5 * 7 * 3, 6 * 5 * 7 + SEG_CAP * 48 + 8),
}


# ------------------------------------------------------------------ the inventory
LOOP_RE = re.compile(r"for \(int f0 = 0; f0 < F; f0 \+= 32768\)")
FUNC_RE = re.compile(r"^(?:static |inline )*(?:void|int|bool|size_t|int32_t)\s+(\w+)\(", re.M)
COUNT_NAMES = {"F", "nwin", "b.nwin", "count", "Fg"}          # a grid extent of these names is a frame or window count


def _dim3_args(text, start):
    """the top-level arguments of the parenthesis that opens at text[start]"""
    depth, args, cur = 0, [], ""
    for ch in text[start:]:
        if ch == "(":
            depth += 1
            if depth == 1:
                continue
        elif ch == ")":
            depth -= 1
            if depth == 0:
                args.append(cur.strip())
                return args
        elif ch == "," and depth == 1:
            args.append(cur.strip())
            cur = ""
            continue
        cur += ch
    return args


def sweep_sources(csrc=CSRC):
    """Every place in csrc/*.hip where a frame or window count meets a grid's y / z extent:
    ("loop", file, function, ordinal within the function) for each `f0 += 32768` loop, and ("grid", file, function, count name) for each
    dim3 whose second or third extent is a frame or window count that no loop splits."""
    hits = []
    for name in sorted(os.listdir(csrc)):
        if not name.endswith(".hip"):
            continue
        text = open(os.path.join(csrc, name)).read()
        funcs = [(m.start(), m.group(1)) for m in FUNC_RE.finditer(text)]

        def enclosing(pos):
            inside = [f for p, f in funcs if p <= pos]
            return inside[-1] if inside else "?"
        seen = {}
        for m in LOOP_RE.finditer(text):
            fn = enclosing(m.start())
            seen[fn] = seen.get(fn, 0) + 1
            hits.append(("loop", name, fn, seen[fn]))
        for m in re.finditer(r"\bdim3\s*(?:\w+)?\(", text):
            args = _dim3_args(text, m.end() - 1)
            for a in args[1:]:
                if a in COUNT_NAMES:
                    hits.append(("grid", name, enclosing(m.start()), a))
    return hits


GPU = "tests/test_frame_chunks_gpu.py::"
WINDOWS = GPU + "test_more_windows_than_65535"
NOT_REACHED = "run only under a switch or for outputs the window-count test does not ask for; the refusal covers its launch: " + WINDOWS
# hit of sweep_sources() -> the test that crosses it (a frame loop: its second launch; a window grid: a window count above 65535), or
# the reason it has none
INVENTORY = {
    ("loop", "filters.hip", "launch_gray", 1): GPU + "test_bgr2gray[8x12",                       # k_gray4
    ("loop", "filters.hip", "launch_gray", 2): GPU + "test_bgr2gray[9x13",                       # k_gray4g
    ("loop", "filters.hip", "launch_gray", 3): GPU + "test_batch_run_single_channel_three_launches",          # k_gray (and test_batch_run[gray_forced])
    ("loop", "filters.hip", "launch_bilateral", 1): GPU + "test_bilateral_u8",
    ("loop", "filters.hip", "launch_grey_open", 1): GPU + "test_grey_open_u8",
    ("loop", "filters.hip", "launch_open3x3", 1): GPU + "test_grey_open3x3_u8",
    ("loop", "filters.hip", "launch_filter_fused", 1): GPU + "test_debug_filter_fused_dense",
    ("loop", "filters.hip", "launch_filter_fused_geom", 1): GPU + "test_debug_filter_fused_geom",
    ("loop", "ccl.hip", "launch_ccl", 1): GPU + "test_ccl_u8_multi_kernel",
    ("loop", "ccl.hip", "launch_regionprops", 1): GPU + "test_regionprops_u8",
    ("loop", "shape_props.hip", "launch_segment_shapes", 1): GPU + "test_segment_shapes_u8",
    ("loop", "stabilize.hip", "launch_stabilize", 1): GPU + "test_stabilize",
    ("loop", "stabilize.hip", "launch_stabilize_subpel", 1): GPU + "test_stabilize_subpel",
    ("loop", "yuv.hip", "launch_yuv420_to_bgr", 1): GPU + "test_yuv420_to_bgr",
    ("loop", "yuv.hip", "launch_yuv_to_bgr", 1): GPU + "test_yuv_to_bgr",
    ("loop", "review.hip", "launch_review", 1): GPU + "test_render_review",
    ("loop", "review.hip", "launch_review_panels", 1): GPU + "test_render_review_panels",
    ("loop", "groups.hip", "launch_gray_groups", 1): GPU + "test_batch_run_groups",
    # ---- window counts in grid y, not split: swk_batch_run refuses above the device's extent (include/swk.h, "Windows per call")
    ("grid", "ialm.hip", "launch_ialm_stats", "b.nwin"): WINDOWS,
    ("grid", "ialm_gram8.hip", "launch_gram_nb", "b.nwin"): WINDOWS,
    ("grid", "ialm_mstate.hip", "launch_m_one", "b.nwin"): WINDOWS,
    ("grid", "ialm_mfma.hip", "launch_select_sparse", "b.nwin"): WINDOWS,
    ("grid", "ialm.hip", "launch_lds", "b.nwin"): WINDOWS + "[variant1]",
    ("grid", "ialm_mfma.hip", "launch_full", "b.nwin"): WINDOWS + "[want_AE]",
    ("grid", "ialm.hip", "launch_planes_to_pn", "nwin"): WINDOWS + "[want_AE]",
    ("grid", "ialm_small.hip", "launch_gram_reduce", "b.nwin"): ("none", "runs for windows of more than 4 Gram slabs; 65536 such windows "
                                                                 "are gigabytes of frames.  " + NOT_REACHED),
    ("grid", "groups.hip", "launch_planes_to_pn_groups", "nwin"): ("none", "A / E of a groups call of more than 65535 windows.  " + NOT_REACHED),
    ("grid", "filters.hip", "launch_resize_linear", "F"): GPU + "test_resize_refuses_more_frames_than_grid_z",
}


def check_inventory(hits=None):
    """every hit of the sweep has an entry, and no entry is left without a hit"""
    hits = sweep_sources() if hits is None else hits
    missing = [h for h in hits if h not in INVENTORY]
    stale = [k for k in INVENTORY if k not in hits]
    assert not missing, "no test named for %s: add it to frame_chunks.INVENTORY" % (missing,)
    assert not stale, "inventory entries without a place in the sources: %s" % (stale,)
    return hits


# ------------------------------------------------------------------ CPU restatements of the stages on K frames
def orc_gray(orc, bgr, mode):
    return np.stack([orc.bgr2gray(np.ascontiguousarray(f), mode) for f in bgr])


def orc_bilateral(orc, planes, d):
    return np.stack([orc.bilateral_u8(p, d) for p in planes])


def orc_open(orc, planes, size):
    return np.stack([orc.grey_open_u8(p, size) for p in planes])


def orc_ccl(orc, planes, conn, order):
    res = [orc.ccl_u8(p, conn, order) for p in planes]
    return np.array([r[0] for r in res], np.int32), np.stack([r[1] for r in res])


def orc_regionprops(orc, labels, cap):
    """(segs (K, cap) SEGMENT_DTYPE with zeros behind the last record, nseg (K,))"""
    from swiftwatcher_amd import _lib
    segs = np.zeros((len(labels), cap), _lib.SEGMENT_DTYPE)
    nseg = np.zeros(len(labels), np.int32)
    for k, lab in enumerate(labels):
        recs = orc.regionprops_u8(lab)
        nseg[k] = len(recs)
        for i, s in enumerate(recs[:cap]):
            segs[k, i] = (s["label"],) + s["bbox"] + (0, s["area"], s["sum_r"], s["sum_c"])
    return segs, nseg


def ref_shapes(labels, cap):
    """(shapes (K, cap) SHAPE_DTYPE, nseg (K,)) by tests/shape_props_ref.py"""
    import shape_props_ref
    from swiftwatcher_amd import _lib
    out = np.zeros((len(labels), cap), _lib.SHAPE_DTYPE)
    nseg = np.zeros(len(labels), np.int32)
    for k, lab in enumerate(labels):
        recs = shape_props_ref.records(lab)
        nseg[k] = len(recs)
        for i, r in enumerate(recs[:cap]):
            out[k, i]["label"] = r["label"]
            out[k, i]["m"] = r["m"]
            out[k, i]["border"] = r["border"]
            out[k, i]["perim"] = r["perim"]
            out[k, i]["quads"] = r["quads"]
    return out, nseg


def find_window_seeds(shapes=((12, 20), (9, 14)), tries=200):
    """the search the committed WINDOW_SEEDS come from"""
    from oracle import reference_path as orc
    found = {}
    for H, W in shapes:
        for seed in range(tries):
            _, with_segs, masked = window_conditions(orc, batch_windows(H, W, seed))
            print("%dx%d seed %d: %d windows with segments, %d masked elements" % (H, W, seed, with_segs, masked))
            if 3 * with_segs >= K and masked == 0:
                found[(H, W)] = seed
                break
    return found


if __name__ == "__main__":
    import sys
    sys.path.insert(0, ROOT)
    print(find_window_seeds())
