"""Victims, dirtiers and the slot inventory of the history-independence tests: tests/test_history_independence_cpu.py and
tests/test_history_independence_gpu.py.  No GPU in here.

The property: a call's outputs are a function of its arguments and the context's switches, not of the calls made before it.  A
swk_ctx keeps its device buffers (enum Slot, csrc/swk_api.hip) for its lifetime, grows them, never clears them as a whole, and
hands them to the next call as they lie; it also keeps the bilateral tables, the two backoff counters and the record of the last
batch.  The protocol of every GPU case:

    fresh = victim(new Context)                   after = victim(Context that first ran the dirtier sequence)
    after == fresh byte for byte in every output, and fresh meets the assertion its host reference already has in the suite

A VICTIM is a small call whose expected result is proven on the host by a module the suite already has (named with each victim).
A DIRTIER is a valid, larger call that leaves the most in the buffers the victim will use: stale contents are what real calls
leave -- finite numbers, indices and counts within the slot's allocation -- never a poison fill.  SLOTS maps every slot to the
dirtier that fills it and a victim that reads or overwrites it; the CPU test holds the table to the sources and the geometry of
every pair to "the dirtier's footprint covers the victim's padding".

Geometry restated from the sources (the functions are file-local there; the CPU test holds the restatements to their text):
    fpad     planes per window in A / Y / E: n rounded up to 4 on the M-state route (ialm_mstate_fpad), to 16 otherwise (ialm_fpad)
    pstride  plane pitch in elements: P rounded up to 128 (ialm_pstride)
    nblk     Gram slabs per window (ialm_pass_nblk)
plan_batch is not restated: tests/history_plan_check.cpp runs the library's own on the groups below."""
import functools
import os
import re
from collections import namedtuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "swiftwatcher_amd", "csrc")


# ------------------------------------------------------------------ the protocol's comparison
def as_bytes(a):
    if hasattr(a, "cpu"):
        a = a.cpu().numpy()
    a = np.ascontiguousarray(a)
    if a.dtype.names:          # records: their fields, not the bytes between them
        return (str(a.dtype), a.shape, b"".join(np.ascontiguousarray(a[k]).tobytes() for k in a.dtype.names))
    return (str(a.dtype), a.shape, a.tobytes())


def assert_same(fresh, after, what):
    """every output of the two runs: the same names, types, shapes and bytes (float64 as raw bytes: -0.0 is not 0.0)"""
    assert sorted(fresh) == sorted(after), (what, sorted(fresh), sorted(after))
    for key in sorted(fresh):
        f, a = as_bytes(fresh[key]), as_bytes(after[key])
        assert f[:2] == a[:2], "%s: output %s changed its type or shape: %s -> %s" % (what, key, f[:2], a[:2])
        if f[2] != a[2]:
            x, y = np.frombuffer(f[2], np.uint8), np.frombuffer(a[2], np.uint8)
            bad = np.nonzero(x != y)[0]
            raise AssertionError("%s: output %s depends on the calls made before: %d of %d bytes differ, the first at byte %d"
                                 % (what, key, len(bad), len(x), bad[0]))


# ------------------------------------------------------------------ IALM geometry, restated
KMAXN = 64          # frames per window of the MFMA / LDS passes; above it the plain f64 kernels (variant 6)


def ialm_fpad(mstate, n):
    return (n + 3) & ~3 if mstate else (n + 15) & ~15


def ialm_pstride(P):
    return (P + 127) & ~127


def ialm_variant(ctx_variant, n, want_AE):
    """plan_ialm's choice of the pass"""
    v = ctx_variant or 4
    if v >= 4 and v != 6 and want_AE:
        v = 2
    if n > KMAXN:
        v = 6
    return v


def ialm_pass_nblk(variant, n, P, nwin):
    if variant >= 2 and variant != 6:
        per_win = (256 * 2 * 3 + nwin - 1) // nwin
        per_win = min(per_win, ((P + 15) // 16 + 7) // 8, 512)
        return max(per_win, 1)
    per_win = (256 * 8 + nwin - 1) // nwin
    return min(max(per_win, 4), 128, (P + 63) // 64)


IalmGeom = namedtuple("IalmGeom", "nwin n P variant mstate fpad pstride nblk")


def ialm_geom(nwin, n, P, ctx_variant=0, want_AE=False):
    v = ialm_variant(ctx_variant, n, want_AE)
    mstate = v in (4, 5)
    return IalmGeom(nwin, n, P, v, mstate, ialm_fpad(mstate, n), ialm_pstride(P), ialm_pass_nblk(v, n, P, nwin))


def ialm_slot_bytes(g, want_E=False):
    """bytes of every slot ialm_start reserves (the NEED lines of swk_api.hip, restated)"""
    felems = g.nwin * g.fpad * g.pstride
    out = {"SL_A": felems * 8, "SL_Y": felems * 8, "SL_BM": g.nwin * g.n * g.n * 8, "SL_VPREV": g.nwin * g.n * g.n * 8,
           "SL_GPART": g.nwin * g.nblk * g.n * g.n * 8, "SL_ZZPART": 2 * g.nwin * g.nblk * 8, "SL_X": g.nwin * g.n * g.P,
           "SL_S": g.nwin * g.n * g.P}
    if g.mstate:
        out["SL_SALT"] = g.nwin * g.n * g.P
    if want_E:
        out["SL_E"] = felems * 8
    return out


def written_granules(g, elem_bytes, granules):
    """Which 2-byte granules of a plane slot (A, Y / U, E) a call of geometry g writes: plane j < n of every window, pixels p < P of
    it.  (What a kernel writes beyond that -- whole tiles, padded planes -- is not counted: the statement is the conservative one.)"""
    out = np.zeros(granules, bool)
    per = elem_bytes // 2
    for w in range(g.nwin):
        for j in range(g.n):
            a = (w * g.fpad + j) * g.pstride * per
            out[a:min(a + g.P * per, granules)] = True
    return out


def padding_granules(g, elem_bytes):
    """The 2-byte granules of a plane slot that are the call's padding: planes n .. fpad - 1, and pixels P .. pstride - 1 of every
    plane.  (extent in granules, mask)"""
    per = elem_bytes // 2
    total = g.nwin * g.fpad * g.pstride * per
    out = np.zeros(total, bool)
    for w in range(g.nwin):
        for j in range(g.fpad):
            a = (w * g.fpad + j) * g.pstride * per
            if j >= g.n:
                out[a:a + g.pstride * per] = True
            else:
                out[a + g.P * per:a + g.pstride * per] = True
    return total, out


def plane_elem_bytes(slot, g):
    """A and E hold float64 on every route (M on the M-state route); the Y slot holds binary16 U there"""
    return 2 if (slot == "SL_Y" and g.mstate) else 8


# ------------------------------------------------------------------ IALM dirtiers
IalmDirtier = namedtuple("IalmDirtier", "name nwin n H W seed")
# 64 and 70 frames, more windows than any victim, pixel counts with another residue mod 16 than every victim's (all victims: 0 or
# 2 or 13), within 70 x 130.  D64 takes the M-state pass (A / E not wanted) or the A/Y-state MFMA pass (wanted); D70 the plain f64
# kernels and k_ialm_small_wide (SL_WIDE) either way.
D64 = IalmDirtier("d64", 3, 64, 70, 129, 64001)          # P = 9030 = 6 mod 16
D70 = IalmDirtier("d70", 2, 70, 69, 130, 70001)          # P = 8970 = 10 mod 16
IALM_DIRTIERS = (D64, D70)


@functools.lru_cache(maxsize=None)
def saturated_frames(nwin, n, H, W, seed):
    """(nwin * n, H, W) u8: checkerboards of 0 / 255 with cells of 1..4 pixels and a phase of the frame's own, every fifth frame all
    255, two pixels in a hundred inverted (no two frames equal, the window has full rank): M, Y, U and the Gram slabs get large"""
    rng = np.random.default_rng(seed)
    r, c = np.indices((H, W))
    out = np.empty((nwin * n, H, W), np.uint8)
    for f in range(nwin * n):
        cell = 1 + f % 4
        img = (((r // cell + c // cell + f) & 1) * 255).astype(np.uint8)
        if f % 5 == 4:
            img[:] = 255
        flip = rng.random((H, W)) < 0.02
        out[f] = np.where(flip, 255 - img, img)
    out.setflags(write=False)
    return out


def dirtier_frames(d):
    return saturated_frames(d.nwin, d.n, d.H, d.W, d.seed)


# ------------------------------------------------------------------ IALM victims
# the trajectory windows (tests/ialm_trajectory_cases.py, proven by tests/test_ialm_trajectory_cpu.py): n = 5, 21, 37 are no
# multiple of 4 or 16, so every route pads their frames; their pixel counts are multiples of 128, so their planes have no padded
# columns.  The two scenes of tests/ccl_patterns.py (proven against the CPU oracle by tests/test_ccl_patterns_gpu.py's cases) have:
# 63 x 94 = 5922 = 2 mod 16 (2 mod 4), 67 x 95 = 6365 = 13 mod 16 (odd).
TRAJECTORY_VICTIMS = ("short5", "plain21", "n37", "dup", "null21")
SCENE_VICTIMS = ("sparse_63x94", "sparse_67x95")
WIDE_VICTIMS = ("wide70", "plain21")          # under variant 6


def victim_geometry(name):
    """(n, H, W) of an IALM victim"""
    if name in SCENE_VICTIMS:
        import ccl_patterns as cp
        s = cp.SCENES[name]
        return 21, s["H"], s["W"]
    import ialm_trajectory_cases as tc
    c = tc.CASES[name]
    return c.n, c.Hc, c.Wc


@functools.lru_cache(maxsize=None)
def scene_roi(name):
    import ccl_patterns as cp
    roi = cp.block_scene(**cp.SCENES[name])
    roi.setflags(write=False)
    return roi


@functools.lru_cache(maxsize=None)
def scene_oracle(name, **overrides):
    from oracle import reference_path as orc
    return orc.window(np.ascontiguousarray(scene_roi(name)), **overrides)


@functools.lru_cache(maxsize=None)
def scene_trajectory(name, maxiter=100):
    """ialm_trajectory_cases.trajectory of a scene's grey window: [(A_k, E_k, ratio_k)]"""
    import ialm_trajectory_cases as tc
    from oracle import reference_path as orc
    g = np.stack([orc.bgr2gray(np.ascontiguousarray(f)) for f in scene_roi(name)])
    return tc.trajectory(g.reshape(g.shape[0], -1).T, maxiter=maxiter)


# ------------------------------------------------------------------ the other families' shapes (victim smaller than its dirtier)
Shape = namedtuple("Shape", "count H W")
# family: (dirtier, victims); counts are frames (planes, crops), H x W the plane the kernel works on.  A dirtier has at least the
# victim's frame count as well: a slot sized per frame (records, counts, sum tables) that the victim had to grow would be a new
# allocation, and the stale records gone with the old one.
PLANE_PAIRS = {
    "filter_fused": (Shape(40, 70, 130), [Shape(9, 67, 95), Shape(9, 33, 65), Shape(21, 70, 61), Shape(21, 33, 130), Shape(21, 9, 13)]),
    "ccl_u8": (Shape(24, 70, 130), [Shape(1, 64, 96), Shape(1, 33, 70), Shape(1, 46, 65), Shape(1, 14, 5), Shape(21, 9, 13)]),
    "regionprops_u8": (Shape(24, 70, 130), [Shape(21, 9, 13)]),
    "segment_shapes_u8": (Shape(24, 70, 130), [Shape(21, 9, 13)]),
    "grey_open_u8": (Shape(40, 70, 130), [Shape(21, 9, 13)]),
    "resize_linear_u8": (Shape(1, 70, 130), [Shape(1, 9, 13)]),
    "bgr_to_yuv420": (Shape(30, 70, 130), [Shape(21, 11, 16)]),
    "render_review": (Shape(30, 70, 130), [Shape(21, 11, 16)]),
    "render_review_panels": (Shape(30, 70, 130), [Shape(21, 11, 16)]),
    "yuv420_to_bgr": (Shape(30, 70, 130), [Shape(21, 10, 14)]),
    "yuv_to_bgr": (Shape(30, 70, 130), [Shape(21, 10, 14)]),
}
# stabilizer: (frames, Ho, Wo, search); the source pictures are designed_case's (rectangle + pad)
STAB_DIRTIER, STAB_VICTIM = (21, 26, 52, 16), (9, 20, 28, 4)
# classifier inputs: (crops, largest side)
CROPS_DIRTIER, CROPS_VICTIM = (40, 300), (10, 80)


def plane_bytes(s):
    return s.count * s.H * s.W


# ------------------------------------------------------------------ the groups calls (plan_batch runs on these: history_plan_check.cpp)
GROUPS_N = 21
# victim: a P < n group (4 x 5, a sub-batch of its own at its true P), the 63 x 94 scene, and a 47 x 94 group padded to the scene's
# pitch.  dirtier: one dense group of three brighter, larger windows.
GROUPS_VICTIM = [(1, 4, 5), (1, 63, 94), (1, 47, 94)]          # (nwin, Hc, Wc) per group
GROUPS_DIRTIER = [(3, 70, 129)]
GROUPS_SINGLE_VICTIM = [(1, 67, 95)]                           # a one-group call after the groups call


# ------------------------------------------------------------------ the slot inventory
Filled = namedtuple("Filled", "dirtier victim")
GPU = "tests/test_history_independence_gpu.py::"
_IALM = "swk_batch_run / swk_ialm of d64 (3 x 64 frames of 70 x 129) and d70 (2 x 70 frames of 69 x 130), saturated checkerboards"
_IALM_AE = _IALM + ", A and E wanted"
_BATCH = "swk_batch_run of ccl_patterns' dense_212x424 scene (255 records on every patterned frame) and of d64"
_FORCED = "the multi-kernel labeller forced on 24 planes of 70 x 130 with more than 255 components"
SLOTS = {
    "SL_ROI": Filled(_BATCH, GPU + "test_batch_scene_after_ialm_dirtiers"),
    "SL_X": Filled(_IALM, GPU + "test_mstate_window_after_ialm_dirtiers"),
    "SL_S": Filled(_IALM, GPU + "test_mstate_window_after_ialm_dirtiers"),
    "SL_BIL": Filled(_BATCH, GPU + "test_batch_scene_after_ialm_dirtiers"),
    "SL_THR": Filled(_BATCH, GPU + "test_batch_scene_after_ialm_dirtiers"),
    "SL_OPEN": Filled(_BATCH, GPU + "test_batch_scene_after_ialm_dirtiers"),
    "SL_LAB8": Filled(_BATCH, GPU + "test_batch_scene_after_ialm_dirtiers"),
    "SL_LAB32": Filled(_FORCED + " (swk_ccl_u8)", GPU + "test_labeller_routes_after_each_other"),
    "SL_A": Filled(_IALM_AE + " and not wanted (M)", GPU + "test_ialm_factors_after_ialm_dirtiers"),
    "SL_Y": Filled(_IALM_AE + " and not wanted (binary16 U)", GPU + "test_ialm_factors_after_ialm_dirtiers"),
    "SL_E": Filled(_IALM_AE, GPU + "test_ialm_factors_after_ialm_dirtiers"),
    "SL_PN": Filled(_IALM_AE + " through swk_batch_run (host A / E staging)", GPU + "test_batch_scene_after_ialm_dirtiers[sparse_63x94-factors]"),
    "SL_BM": Filled(_IALM, GPU + "test_ialm_factors_after_ialm_dirtiers"),
    "SL_VPREV": Filled(_IALM + " (Newton-Schulz warm start)", GPU + "test_ialm_factors_after_ialm_dirtiers"),
    "SL_GPART": Filled(_IALM + " (only frame-block pairs ib <= jb are written)", GPU + "test_mstate_window_after_ialm_dirtiers"),
    "SL_ZZPART": Filled(_IALM + " (second half: max |U|)", GPU + "test_mstate_window_after_ialm_dirtiers"),
    "SL_WIN": Filled(_IALM, GPU + "test_mstate_window_after_ialm_dirtiers"),
    "SL_ACTIVE": Filled(_IALM, GPU + "test_mstate_window_after_ialm_dirtiers"),
    "SL_PARENT": Filled(_FORCED, GPU + "test_labeller_routes_after_each_other"),
    "SL_ROOTBITS": Filled(_FORCED, GPU + "test_labeller_routes_after_each_other"),
    "SL_WORDPREFIX": Filled(_FORCED, GPU + "test_labeller_routes_after_each_other"),
    "SL_NCOMP": Filled(_FORCED, GPU + "test_labeller_routes_after_each_other"),
    "SL_TABLE": Filled(_FORCED + " (swk_regionprops_u8, 255 labels)", GPU + "test_records_with_fewer_labels"),
    "SL_SUMS": Filled(_FORCED + " (swk_regionprops_u8, 255 labels)", GPU + "test_records_with_fewer_labels"),
    "SL_SEGS": Filled(_BATCH, GPU + "test_records_with_fewer_labels"),
    "SL_NSEG": Filled(_BATCH, GPU + "test_records_with_fewer_labels"),
    "SL_TMP_IN": Filled("every stand-alone call's larger twin (30 to 40 planes of 70 x 130)", GPU + "test_stand_alone_calls"),
    "SL_TMP_OUT": Filled("every stand-alone call's larger twin", GPU + "test_stand_alone_calls"),
    "SL_TMP_AUX": Filled("swk_render_review_panels and swk_grey_open_u8 on 30 to 40 planes of 70 x 130", GPU + "test_stand_alone_calls"),
    "SL_COLORW": Filled("the fused filter at d = 9, sigmas (40, 3): 81 taps", GPU + "test_bilateral_tables_are_rebuilt_and_restored"),
    "SL_SPACEW": Filled("the fused filter at d = 9, sigmas (40, 3)", GPU + "test_bilateral_tables_are_rebuilt_and_restored"),
    "SL_TAPDR": Filled("the fused filter at d = 9, sigmas (40, 3)", GPU + "test_bilateral_tables_are_rebuilt_and_restored"),
    "SL_TAPDC": Filled("the fused filter at d = 9, sigmas (40, 3)", GPU + "test_bilateral_tables_are_rebuilt_and_restored"),
    "SL_SALT": Filled(_IALM + " (M-state pass: the alternate sparse image)", GPU + "test_mstate_window_after_ialm_dirtiers"),
    "SL_WIDE": Filled("d70 (k_ialm_small_wide's workspace)", GPU + "test_ialm_factors_after_ialm_dirtiers[plain_f64+wide_jacobi-d64_then_d70]"),
    "SL_REDO_X": Filled("d64 stopped at maxiter = 2: its guess fails, three windows run again", GPU + "test_backoff_after_a_failed_guess"),
    "SL_REDO_S": Filled("d64 stopped at maxiter = 2", GPU + "test_backoff_after_a_failed_guess"),
    "SL_REDO_P": Filled("a groups call of d64-sized windows stopped at maxiter = 2", GPU + "test_groups_call_after_a_dense_call[truncated]"),
    "SL_SEGOFFS": Filled("swk_segment_inputs with boxes of 513 px and above and skipped boxes", GPU + "test_segment_inputs_counts_are_the_calls_own"),
    "SL_SEGLARGE": Filled("swk_segment_inputs with boxes of 513 px and above", GPU + "test_segment_inputs_counts_are_the_calls_own"),
    "SL_CL_CROPS": Filled("swk_classifier_input_window of 40 crops of up to 300 px", GPU + "test_classifier_input_with_fewer_and_smaller_crops"),
    "SL_CL_OFFS": Filled("swk_classifier_input_window of 40 crops", GPU + "test_classifier_input_with_fewer_and_smaller_crops"),
    "SL_CL_HW": Filled("swk_classifier_input_window of 40 crops", GPU + "test_classifier_input_with_fewer_and_smaller_crops"),
    "SL_CL_PATCH": Filled("swk_classifier_input_window of 40 crops, patches wanted", GPU + "test_classifier_input_with_fewer_and_smaller_crops"),
    "SL_CL_NET": Filled("swk_classifier_input_window of 40 crops, host network input", GPU + "test_classifier_input_with_fewer_and_smaller_crops"),
    "SL_GRP": Filled("a groups call of more windows", GPU + "test_groups_call_after_a_dense_call"),
    "SL_REVIEW": Filled("swk_render_review_labels with boxes, marks and labels on 30 frames", GPU + "test_stand_alone_calls[render_review_text]"),
    "SL_SHAPE_TAB": Filled("swk_segment_shapes_u8 of 24 planes of 70 x 130 with 255 labels", GPU + "test_records_with_fewer_labels"),
    "SL_SHAPE_REC": Filled("swk_segment_shapes_u8 of 24 planes with 255 labels", GPU + "test_records_with_fewer_labels"),
    "SL_SHAPE_NSEG": Filled("swk_segment_shapes_u8 of 24 planes with 255 labels", GPU + "test_records_with_fewer_labels"),
    "SL_STAB_PLANE": Filled("swk_stabilize_u8 at S = 16 on 21 frames", GPU + "test_stand_alone_calls[stabilize]"),
    "SL_STAB_TAB": Filled("swk_stabilize_u8 at S = 16 (33 x 33 candidates a frame)", GPU + "test_stand_alone_calls[stabilize]"),
    "SL_STAB_REC": Filled("swk_stabilize_u8 at S = 16 on 21 frames", GPU + "test_stand_alone_calls[stabilize]"),
    "SL_SUBPEL_PLANE": Filled("swk_stabilize_subpel_u8 at S = 16 on 21 frames", GPU + "test_stand_alone_calls[stabilize_subpel]"),
    "SL_SUBPEL_TAB": Filled("swk_stabilize_subpel_u8 at S = 16", GPU + "test_stand_alone_calls[stabilize_subpel]"),
    "SL_SUBPEL_REC": Filled("swk_stabilize_subpel_u8 at S = 16 on 21 frames", GPU + "test_stand_alone_calls[stabilize_subpel]"),
    "SL_SUBPEL_SUBTAB": Filled("swk_stabilize_subpel_u8 at S = 16 on 21 frames", GPU + "test_stand_alone_calls[stabilize_subpel]"),
}
# Marks a slot may carry instead of a Filled entry (none does today): ("constant tables", why) or ("host-visible output only", why)
EXEMPT_KINDS = ("constant tables", "host-visible output only")


def parse_slots(path=None):
    """(names of enum Slot in order, SL_COUNT left out; {slot: number of NEED / need sites}) of csrc/swk_api.hip"""
    text = open(path or os.path.join(CSRC, "swk_api.hip")).read()
    m = re.search(r"enum Slot \{(.*?)\};", text, re.S)
    assert m, "enum Slot not found"
    names = [t.split("=")[0].strip() for t in m.group(1).replace("\n", " ").split(",") if t.strip()]
    assert names[-1] == "SL_COUNT"
    sites = {}
    for s in re.findall(r"\b(?:NEED|need)\(ctx, (SL_[A-Z0-9_]+)", text):
        sites[s] = sites.get(s, 0) + 1
    return names[:-1], sites


def check_slots(names=None, sites=None, table=None):
    if names is None:
        names, sites = parse_slots()
    table = SLOTS if table is None else table
    missing = [s for s in names if s not in table]
    stale = [s for s in table if s not in names]
    assert not missing, "no history case named for %s: add it to history_cases.SLOTS" % (missing,)
    assert not stale, "history_cases.SLOTS names slots the library does not have: %s" % (stale,)
    unknown = [s for s in sites if s not in names]
    assert not unknown, "NEED sites name slots outside enum Slot: %s" % (unknown,)
    for s, entry in table.items():
        if isinstance(entry, Filled):
            assert entry.dirtier and entry.victim.startswith(GPU), s
        else:
            assert entry[0] in EXEMPT_KINDS and entry[1], s
