"""swk_segment_shapes_u8 (csrc/shape_props.hip) against tests/shape_props_ref.py, field by field and for exact equality: the records
are integer sums, so nothing depends on scheduling.  Then the feature end to end: FrameQueue(shape_props=True), count_swifts(...,
shape_props=True).

The kernel's tile is 16 rows (a band) by 256 columns; BAND and TILE_COLS restate kShapeRows and kShapeCols.  Heights straddle the
band, widths the 4-, 2- and 1-byte loads (a dense host plane's row pitch is its width) and the tile's column edge."""
import ctypes

import numpy as np
import pytest
from scipy import ndimage

import ccl_patterns as cp
import shape_props_ref as ref

pytestmark = pytest.mark.gpu

BAND, TILE_COLS = 16, 256
VALUES = (1, 254, 255, 7, 128, 2)
WIDTHS = (1, 2, 3, 5, 31, 32, 33, 63, 64, 65, 127, 130, 255, 256, 257, 260)
HEIGHTS = (1, 2, BAND - 1, BAND, BAND + 1, 2 * BAND + 1)
ERR_ARG = -1


@pytest.fixture(scope="module")
def ctx():
    from swiftwatcher_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def check(ctx, planes, seg_cap=255, got=None):
    """every frame's records equal the helper's; returns the records"""
    planes = np.asarray(planes)
    recs, nseg = got if got is not None else ctx.segment_shapes_u8(planes, seg_cap=seg_cap)
    assert recs.shape == (len(planes), seg_cap) and nseg.shape == (len(planes),)
    for f, plane in enumerate(planes):
        want = ref.records(plane)
        assert int(nseg[f]) == len(want), f
        k = min(len(want), seg_cap)
        assert ref.as_dicts(recs[f, :k]) == want[:k], f
        assert not recs[f, k:].tobytes().strip(b"\0"), "slots past nseg are zero"
        assert not np.any(recs[f]["reserved_"])
    return recs, nseg


def by_component(mask, values=VALUES):
    """the mask's 8-connected components painted with `values` in turn: with more components than values, separate blobs share one"""
    lab, n = ndimage.label(mask, np.ones((3, 3), bool))
    table = np.array([0] + [values[i % len(values)] for i in range(n)], np.uint8)
    return table[lab]


def family_cases():
    cases = [c for c in cp.small_families() if max(c.img.shape) <= 32768]          # (a side above 32768 is refused: the extreme rows)
    cases += [cp.spiral(50, 70), cp.rings(40, 56, 1), cp.comb(), cp.checkerboard(36, 50, 3), cp.diagonal_contacts(33)]
    return cases


def grouped(planes):
    by = {}
    for p in planes:
        by.setdefault(p.shape, []).append(p)
    return [np.stack(v) for _, v in sorted(by.items())]


def test_pattern_families_painted_pixel_by_pixel(ctx):
    """ccl_patterns' own paint: up to 255 values per plane, every region scattered over the whole plane (the planes of up to 2,500
    pixels: the helper works value by value)"""
    planes = [c.img for c in family_cases() if c.img.size <= 2500]
    assert len(planes) > 20
    for stack in grouped(planes):
        check(ctx, stack)


def test_pattern_families_painted_by_component(ctx):
    planes = [by_component(c.img > 0) for c in family_cases()]
    assert any(ndimage.label(p == 1, np.ones((3, 3), bool))[1] > 1 for p in planes), "one plane has two blobs of one value"
    present = set(np.unique(np.concatenate([p.ravel() for p in planes])))
    assert {1, 254, 255} <= present
    for stack in grouped(planes):
        check(ctx, stack)


def test_two_separate_blobs_of_one_value_are_one_region(ctx):
    plane = np.zeros((40, 300), np.uint8)
    plane[3:9, 4:11] = 9
    plane[25:38, 250:290] = 9          # in another band and another column tile
    plane[20:23, 100:104] = 3
    recs, nseg = check(ctx, plane[None])
    assert nseg[0] == 2 and recs[0, 1]["m"][0] == 6 * 7 + 13 * 40


def blobs(seed, H, W):
    rng = np.random.default_rng(seed)
    coarse = rng.choice(np.array([0, 0, 1, 2, 254, 255], np.uint8), size=((H + 2) // 3, (W + 2) // 3))
    plane = np.kron(coarse, np.ones((3, 3), np.uint8))[:H, :W].copy()
    noise = rng.random((H, W))
    plane[noise < 0.06] = 0
    plane[noise > 0.95] = 77
    return plane


@pytest.mark.parametrize("W", WIDTHS)
def test_widths_and_heights(ctx, W):
    for H in HEIGHTS:
        check(ctx, np.stack([blobs(1000 * H + W, H, W), blobs(77 + 1000 * H + W, H, W)]))


def test_full_planes_of_one_value_touch_every_edge_and_corner(ctx):
    for H, W in ((1, 1), (1, 7), (7, 1), (2, 2), (BAND, TILE_COLS), (BAND + 1, TILE_COLS + 1), (3 * BAND, 40)):
        check(ctx, np.full((1, H, W), 200, np.uint8))


def edge_planes():
    H, W = 3 * BAND + 2, TILE_COLS + 44
    out = []
    p = np.zeros((H, W), np.uint8)          # a region crossing two bands, one crossing three, both crossing the column tiles' edge
    p[BAND - 3:BAND + 4, 10:20] = 5
    p[BAND - 2:2 * BAND + 5, TILE_COLS - 6:TILE_COLS + 9] = 6
    out.append(p)
    p = np.zeros((H, W), np.uint8)          # the four edges and the four corners
    p[0, 5:30] = 1
    p[H - 1, 40:W - 3] = 2
    p[4:H - 4, 0] = 3
    p[9:30, W - 1] = 4
    p[0:2, 0:2] = 5
    p[0:3, W - 2:W] = 6
    p[H - 2:H, 0:3] = 7
    p[H - 1, W - 1] = 8
    out.append(p)
    p = np.zeros((H, W), np.uint8)          # classes decided by pixels in the neighbouring band's / tile's halo
    for k in range(12):                     # diagonal lines through a band boundary and through the tile's column edge
        p[BAND - 6 + k, 20 + k] = 1
        p[BAND + 5 - k, 60 + k] = 2
        p[5 + k, TILE_COLS - 6 + k] = 3
    p[2:H - 2, 100] = 4                     # a one-pixel-wide vertical line over three bands
    p[3, 110:W - 2] = 5                     # ... and a horizontal one over both tiles
    p[BAND - 8:BAND, 130] = 6               # an L whose corner sits on the band's last row
    p[BAND - 1, 130:140] = 6
    p[BAND:BAND + 8, 150] = 7               # ... and one on the next band's first row
    p[BAND, 150:160] = 7
    p[2 * BAND - 2:2 * BAND + 2, 170:174] = 8          # a 4x4 block on the boundary, with a hole on it
    p[2 * BAND - 1:2 * BAND + 1, 171:173] = 0
    p[2 * BAND:2 * BAND + 3, TILE_COLS - 2:TILE_COLS + 1] = 9          # a plus sign on the crossing of a band and a tile edge
    p[2 * BAND + 1, TILE_COLS - 2] = p[2 * BAND + 1, TILE_COLS] = 9
    p[2 * BAND, TILE_COLS - 2] = p[2 * BAND, TILE_COLS] = p[2 * BAND + 2, TILE_COLS - 2] = p[2 * BAND + 2, TILE_COLS] = 0
    out.append(p)
    p = np.zeros((H, W), np.uint8)          # two values interleaved across the boundaries: windows that count for both
    p[BAND - 1::2, :] = 11
    p[:, TILE_COLS - 1::2] = 12
    out.append(p)
    return np.stack(out)


def test_regions_on_band_and_tile_boundaries(ctx):
    check(ctx, edge_planes())


@pytest.mark.parametrize("count", [1, 3, 70])
def test_frame_indexing(ctx, count):
    check(ctx, np.stack([blobs(31 * f + count, 21, 37) for f in range(count)]))


def all_values_plane():
    plane = np.zeros((34, 48), np.uint8)
    v = 1
    for r in range(0, 34, 2):
        for c in range(0, 48, 3):
            if v <= 255:
                plane[r:r + 1 + (v % 2), c:c + 2] = v
                v += 1
    assert len(np.unique(plane)) == 256
    return plane


@pytest.mark.parametrize("seg_cap", [255, 7, 1])
def test_truncation_and_an_empty_frame(ctx, seg_cap):
    planes = np.stack([all_values_plane(), np.zeros((34, 48), np.uint8), blobs(3, 34, 48)])
    recs, nseg = check(ctx, planes, seg_cap=seg_cap)
    assert nseg.tolist()[:2] == [255, 0]
    assert not recs[1].tobytes().strip(b"\0")


def test_device_planes_are_read_where_they_lie(ctx):
    import torch
    F, H, W = 5, 2 * BAND + 3, 67
    planes = np.stack([blobs(900 + f, H, W) for f in range(F)])
    want = ctx.segment_shapes_u8(planes)
    check(ctx, planes, got=want)
    wide = np.full((F, H, W + 13), 99, np.uint8)          # what lies between the rows is another value: it must not be read
    wide[:, :, :W] = planes
    dev = torch.from_numpy(wide).cuda()
    got = ctx.segment_shapes_u8(dev[:, :, :W])
    assert got[0].tobytes() == want[0].tobytes() and np.array_equal(got[1], want[1])
    # frames backwards: a negative frame stride from the last frame
    got = ctx.segment_shapes_u8(dict(ptr=dev[F - 1].data_ptr(), shape=(F, H, W), frame_stride=-dev.stride(0), row_stride=dev.stride(1)))
    assert got[0].tobytes() == want[0][::-1].tobytes() and np.array_equal(got[1], want[1][::-1])
    # an odd base address and an odd pitch: the 1-byte loads on the same data
    got = ctx.segment_shapes_u8(dev[:, 1:, 1:W])
    check(ctx, planes[:, 1:, 1:], got=got)
    # the same strides from host memory
    got = ctx.segment_shapes_u8(wide[::-1, :, :W])
    assert got[0].tobytes() == want[0][::-1].tobytes()
    dense = torch.from_numpy(planes).cuda()
    got = ctx.segment_shapes_u8(dense)
    assert got[0].tobytes() == want[0].tobytes()


def power(n, k):
    return sum(i ** k for i in range(n))


def full_plane_record(H, W, v):
    m = [power(H, p) * power(W, q) for p, q in ref.ORDER]
    border = H * W if min(H, W) <= 2 else 2 * H + 2 * W - 4
    return m, border


def test_the_largest_square_plane_does_not_overflow(ctx):
    H = W = 4096
    assert H * W * max(H - 1, W - 1) ** 3 < 2 ** 63
    small = ref.records(np.full((9, 11), 3, np.uint8))[0]
    m, border = full_plane_record(9, 11, 3)
    assert small["m"] == m and small["border"] == border and small["perim"] == [border, 0, 0] and small["quads"] == [4, 0, 0]
    recs, nseg = ctx.segment_shapes_u8(np.full((1, H, W), 3, np.uint8), seg_cap=2)
    m, border = full_plane_record(H, W, 3)
    assert nseg[0] == 1 and recs[0, 0]["label"] == 3
    assert [int(x) for x in recs[0, 0]["m"]] == m
    assert m[6] == (H * (H - 1) // 2) ** 2 * W and 2 ** 57 < m[6] < 2 ** 63          # the largest of the sums: far beyond 32 bits, within 63
    assert int(recs[0, 0]["border"]) == border and recs[0, 0]["perim"].tolist() == [border, 0, 0] and recs[0, 0]["quads"].tolist() == [4, 0, 0]
    assert not recs[0, 1].tobytes().strip(b"\0")


def raw_call(ctx, planes, H, W, seg_cap=4, count=1, mem=0, row_stride=None, labels="planes", shapes="shapes", nseg="nseg"):
    """swk_segment_shapes_u8 as it is, with outputs prefilled: (rc, outputs untouched)"""
    from swiftwatcher_amd import _lib
    out = {"planes": planes, "shapes": np.full((max(count, 1), max(seg_cap, 1)), 0, _lib.SHAPE_DTYPE), "nseg": np.full(max(count, 1), -7, np.int32)}
    out["shapes"].view(np.uint8)[...] = 0xA5
    before = out["shapes"].tobytes()
    ptr = lambda key: ctypes.c_void_p(out[key].ctypes.data) if key is not None else None          # noqa: E731
    rs = W if row_stride is None else row_stride
    rc = ctx._lib.swk_segment_shapes_u8(ctx._h, ptr(labels), mem, count, H, W, H * rs, rs, seg_cap, ptr(shapes), ptr(nseg))
    return rc, out["shapes"].tobytes() == before and np.all(out["nseg"] == -7)


@pytest.mark.parametrize("H,W", [(1, 32768), (8, 32768), (9, 32768), (32768, 9), (32768, 8)])
def test_the_overflow_bound_is_the_stated_inequality(ctx, H, W):
    planes = np.full((H, W), 17, np.uint8)
    refused = H * W * max(H - 1, W - 1) ** 3 >= 2 ** 63
    rc, untouched = raw_call(ctx, planes, H, W)
    if refused:
        assert rc == ERR_ARG and untouched
    else:
        assert rc == 0
        recs, nseg = ctx.segment_shapes_u8(planes[None], seg_cap=1)
        m, border = full_plane_record(H, W, 17)
        assert nseg[0] == 1 and [int(x) for x in recs[0, 0]["m"]] == m and int(recs[0, 0]["border"]) == border


@pytest.mark.parametrize("kw", [dict(labels=None), dict(shapes=None), dict(nseg=None), dict(count=0), dict(count=-1), dict(H=0), dict(H=32769),
                                dict(W=0), dict(W=32769), dict(seg_cap=0), dict(seg_cap=256), dict(row_stride=5), dict(mem=2), dict(mem=-1)],
                         ids=lambda kw: "%s_%s" % next(iter(kw.items())))
def test_every_refusal_leaves_the_outputs_alone(ctx, kw):
    args = dict(H=6, W=6)
    args.update(kw)
    # (a buffer as large as the refused geometry claims: nothing is read, and nothing could be read past an end either)
    planes = np.full((max(args["H"], 1) * max(args["W"], 1) + 64,), 1, np.uint8)
    rc, untouched = raw_call(ctx, planes, **args)
    assert rc == ERR_ARG and untouched
    rc, _ = raw_call(ctx, planes, H=6, W=6)
    assert rc == 0, "the same call without the fault is accepted"


# ---- with the existing path, and end to end ----------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def golden_window(golden_dir, ctx):
    import os
    frames = np.load(os.path.join(golden_dir, "ialm_47x94x21.npz"))["frames"]
    return ctx.batch_run(np.ascontiguousarray(frames), 1, 21, stages=("labels",))


def test_records_match_the_batch_calls_region_records(ctx, golden_window):
    res = golden_window
    recs, nseg = check(ctx, res["labels"])
    assert np.array_equal(nseg, res["nseg"]) and nseg.sum() > 0
    for f in range(21):
        k = int(nseg[f])
        assert np.array_equal(recs[f, :k]["label"], res["segs"][f, :k]["label"])
        assert np.array_equal(recs[f, :k]["m"][:, 0], res["segs"][f, :k]["area"])
        assert np.array_equal(recs[f, :k]["m"][:, 1], res["segs"][f, :k]["sum_r"])
        assert np.array_equal(recs[f, :k]["m"][:, 2], res["segs"][f, :k]["sum_c"])


CROP = [(30, 20), (30 + 96, 20 + 64)]


@pytest.fixture(scope="module")
def clip():
    from swiftwatcher_amd import synthetic
    return synthetic.full_frames(500, 52, CROP, frame_hw=(110, 160), birds=4, bird_len=(8, 12), bird_wid=(3, 5))[::-1].copy()


def _shape_values(obj):
    from swiftwatcher_amd import image_filtering as img
    return [np.asarray(getattr(obj, name), dtype=np.float64).tobytes() for name in img.SHAPE_PROPERTIES]


def _window(clip, **kw):
    from swiftwatcher_amd.data_structures import FrameQueue
    queue = FrameQueue(21, **kw)
    queue.push_list_of_frames(list(clip[:21]), list(range(21)), ["t%d" % k for k in range(21)])
    queue.preprocess_queue(CROP, None)
    queue.segment_queue((24, 24), CROP)
    return queue


@pytest.mark.parametrize("keep_stages", [True, False])
def test_framequeue_segments_carry_the_shape_attributes(ctx, clip, keep_stages):
    from swiftwatcher_amd import _lib, image_filtering as img
    default = _lib.default_context(0)
    calls = []
    real = default.segment_shapes_u8
    default.segment_shapes_u8 = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
    try:
        plain = _window(clip, keep_stages=True)
        assert not calls, "without the flag no shape call is made"
        queue = _window(clip, keep_stages=keep_stages, shape_props=True)
        assert len(calls) == 1, "one call per window"
    finally:
        del default.segment_shapes_u8
    total = 0
    for slot, ref_slot in zip(queue, plain):
        labels = ref_slot.processed_frames["cc_labeling"]
        want = img.get_segment_properties(labels, shape=True)
        assert [s.label for s in slot.segments] == [p.label for p in want] == [s.label for s in ref_slot.segments]
        for seg, props, bare in zip(slot.segments, want, ref_slot.segments):
            assert _shape_values(seg) == _shape_values(props)
            assert (seg.bbox, seg.centroid, seg.area) == (props.bbox, props.centroid, props.area) == (bare.bbox, bare.centroid, bare.area)
            assert "_shape" not in bare.__dict__ and not hasattr(bare, "orientation")
            total += 1
        if not keep_stages:
            assert "cc_labeling" not in slot.processed_frames and "RPCA" not in slot.processed_frames and slot.stage_planes is None
    assert total > 10


def _event_records(events, shape):
    return [[(s.parent_frame_number, s.label, tuple(s.bbox), tuple(s.centroid), s.area) + (tuple(_shape_values(s)) if shape else ())
             for s in ev] for ev in events]


@pytest.mark.parametrize("wpc", [1, 4])
def test_count_swifts_is_unchanged_and_its_events_carry_the_attributes(clip, wpc):
    import copy
    from swiftwatcher_amd import pipeline
    roi_mask = np.zeros((64, 96), np.uint8)
    roi_mask[51:, :] = 255
    want_count, want = pipeline.count_swifts(list(clip), CROP, roi_mask, fps=30.0, windows_per_call=wpc)
    count, events = pipeline.count_swifts(list(clip), CROP, roi_mask, fps=30.0, windows_per_call=wpc, shape_props=True)
    assert count == want_count and _event_records(events, False) == _event_records(want, False)
    assert sum(len(ev) for ev in events) > 0
    for ev in events:
        for s in ev:
            assert math_ok(s)
    assert _event_records(copy.deepcopy(events), True) == _event_records(events, True)
    for ev in want:
        for s in ev:
            assert not hasattr(s, "eccentricity")


def math_ok(s):
    return (0.0 <= s.eccentricity <= 1.0 and -np.pi / 2 <= s.orientation <= np.pi / 2 and s.major_axis_length >= s.minor_axis_length >= 0
            and s.perimeter >= 0 and 0 < s.extent <= 1 and isinstance(s.euler_number, int) and s.moments[0, 0] == s.area)


def test_groups_and_the_reader_that_segments_ahead(clip):
    """count_swifts_videos (one shape call per group) and PresegmentingReader give the segments of the serial loop, attributes included"""
    from swiftwatcher_amd import pipeline
    from swiftwatcher_amd.io_frames import ArrayReader, PresegmentingReader
    roi_mask = np.zeros((64, 96), np.uint8)
    roi_mask[51:, :] = 255
    crop2 = [(20, 10), (20 + 80, 10 + 60)]
    mask2 = np.zeros((60, 80), np.uint8)
    mask2[48:, :] = 255
    lone = [pipeline.count_swifts(list(clip), CROP, roi_mask, shape_props=True), pipeline.count_swifts(list(clip[:30]), crop2, mask2, shape_props=True)]
    both = pipeline.count_swifts_videos([list(clip), list(clip[:30])], regions=[(CROP, roi_mask), (crop2, mask2)], shape_props=True)
    for (c0, e0), (c1, e1) in zip(lone, both):
        assert c0 == c1 and _event_records(e0, True) == _event_records(e1, True)
    reader = PresegmentingReader(ArrayReader(list(clip), fps=30.0), CROP, queue_size=21, windows=2)
    try:
        count, events = pipeline.count_swifts(reader, CROP, roi_mask, shape_props=True)
        assert reader.shape_props
    finally:
        reader.close()
    assert count == lone[0][0] and _event_records(events, True) == _event_records(lone[0][1], True)
