"""The labeller of the batch calls, k_ccl_frame<VEC, PROPS = true> (csrc/ccl.hip: u8 labels and region records in one workgroup per
frame), on every pattern family of tests/ccl_patterns.py, handed to it by swk_debug_ccl_frame_props (include/swk_debug.h) through the
launcher swk_batch_run takes.  tests/test_ccl_patterns_gpu.py reaches this instantiation only through six RPCA scenes built so
that the opened frames come out structured; here the frames are the patterns themselves.

Frames of one shape go together in one call, at all four (connectivity, order) pairs: the shapes put the frames on the 4-, 2- and
1-byte loads (VEC) and on both sides of the run cap.  Labels, nseg and every record equal the CPU oracle's, the recount of the
oracle's int32 labels (label k and k + 256 j united, multiples of 256 gone) and the GPU stage functions swk_ccl_u8 +
swk_regionprops_u8, at seg_cap 255, 17 and 1; the reversed batch gives the reversed result; a frame size the one-workgroup kernel does
not take is refused.  tests/test_ccl_patterns_cpu.py holds the oracle to scipy and numpy on the same frames."""
import functools

import numpy as np
import pytest

import ccl_patterns as cp
from helpers import orc_seg_tuples

pytestmark = pytest.mark.gpu

PAIRS = [(8, 1), (8, 0), (4, 0), (4, 1)]
PAIR_IDS = ["8way_block", "8way_raster", "4way_raster", "4way_block"]
CAPS = (255, 17, 1)


def _groups():
    """{shape: [Case]}: every frame of the small families and of the three batch mixes, by shape"""
    by = {}
    for case in cp.small_families() + [c for shape in cp.K_RUN_SHAPES for c in cp.batch_mix(*shape)]:
        by.setdefault(case.img.shape, []).append(case)
    return by


GROUPS = _groups()
SHAPES = sorted(GROUPS)


@pytest.fixture(scope="module")
def orc():
    from oracle import reference_path
    return reference_path


@pytest.fixture(scope="module")
def ctx():
    from swiftwatcher_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def _records(segs):
    return [(int(s["label"]), int(s["r0"]), int(s["c0"]), int(s["r1"]), int(s["c1"]), int(s["area"]), int(s["sum_r"]), int(s["sum_c"]))
            for s in segs]


@functools.lru_cache(maxsize=None)
def _oracle(shape, conn, order):
    """per frame of the group: (u8 labels, records of those labels, records recounted from the int32 labels)"""
    from oracle import reference_path as orc
    out = []
    for case in GROUPS[shape]:
        _, lab32 = orc.ccl_u8(case.img, conn, order)
        lab8 = orc.labels_to_u8(lab32)
        out.append((lab8, orc_seg_tuples(orc.regionprops_u8(lab8)), cp.merged_records(lab32)))
    return out


def test_the_groups_cover_every_load_width_and_both_sides_of_the_run_cap():
    assert all(cp.frame_kernel_takes(*s) for s in SHAPES)
    assert {0, 2} <= {(s[0] * s[1]) % 4 for s in SHAPES} and any((s[0] * s[1]) % 2 for s in SHAPES)          # VEC 4, 2 and 1
    for shape in cp.K_RUN_SHAPES:
        runs = [cp.count_runs(c.img) for c in GROUPS[shape]]
        assert {1023, 1024, 1025} <= set(runs) and min(runs) == 0 and len(runs) >= 13
    assert max(len(g) for g in GROUPS.values()) >= 20 and len(SHAPES) >= 30


@pytest.mark.parametrize("conn,order", PAIRS, ids=PAIR_IDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_labels_and_records_of_every_pattern(ctx, orc, shape, conn, order):
    cases = GROUPS[shape]
    ims = np.stack([c.img for c in cases])
    want = _oracle(shape, conn, order)
    nc, lab32 = ctx.ccl_u8(ims, conn, order)
    gpu_lab8 = orc.labels_to_u8(lab32)
    first = None
    for cap in CAPS:
        lab, segs, nseg = ctx.debug_ccl_frame_props(ims, conn, order, seg_cap=cap)
        assert segs.shape == (len(cases), cap)
        gsegs, gnseg = ctx.regionprops_u8(gpu_lab8, seg_cap=cap)
        for f, (case, (lab8, recs, merged)) in enumerate(zip(cases, want)):
            what = (case.name, shape, conn, order, cap)
            np.testing.assert_array_equal(lab[f], lab8, err_msg=str(what))
            assert recs == merged, what                            # (the oracle's own records are the united ones)
            assert int(nseg[f]) == len(recs) == min(int(nc[f]), 255), what
            kept = min(len(recs), cap)
            assert _records(segs[f, :kept]) == recs[:cap], what
            assert not segs[f, kept:].tobytes().strip(b"\0"), what          # zeros behind a frame's last record
            # ... and the stage functions on the GPU
            np.testing.assert_array_equal(lab[f], gpu_lab8[f], err_msg=str(what))
            assert int(gnseg[f]) == int(nseg[f]) and _records(gsegs[f, :kept]) == _records(segs[f, :kept]), what
        if first is None:
            first = (lab, segs, nseg)
    # the same frames in the opposite order: no frame's labels or records depend on its neighbours'
    lab_r, segs_r, nseg_r = ctx.debug_ccl_frame_props(ims[::-1].copy(), conn, order, seg_cap=CAPS[0])
    assert np.array_equal(lab_r[::-1], first[0]) and np.array_equal(segs_r[::-1], first[1]) and np.array_equal(nseg_r[::-1], first[2])


def test_a_size_the_one_workgroup_kernel_does_not_take_is_refused(ctx, orc):
    from swiftwatcher_amd import _lib
    assert not cp.frame_kernel_takes(800, 808)
    with pytest.raises(_lib.SwkError):
        ctx.debug_ccl_frame_props(np.zeros((1, 800, 808), np.uint8))
    for bad in (dict(connectivity=6), dict(seg_cap=0), dict(seg_cap=256)):
        with pytest.raises(_lib.SwkError):
            ctx.debug_ccl_frame_props(cp.u_shape().img[None], **bad)
    case = cp.u_shape()
    lab, segs, nseg = ctx.debug_ccl_frame_props(case.img[None])
    np.testing.assert_array_equal(lab[0], orc.labels_to_u8(orc.ccl_u8(case.img)[1]))
    assert int(nseg[0]) == 2 and _records(segs[0, :2]) == orc_seg_tuples(orc.regionprops_u8(lab[0]))
