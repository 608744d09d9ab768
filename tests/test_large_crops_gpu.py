"""Segment boxes with a side of 513..4096 on the device route (swk_segment_inputs / swk_segment_inputs_last and the groups call's
path): the second kernel of csrc/classify_input.hip must produce Pillow's horizontal-pass-first resize bit for bit.

Expected network inputs are made without a second normaliser: the 24 x 24 patches of the restatement (tests/pil_resize_ref.py, held
to Pillow in tests/test_large_crops_cpu.py) are fed as 24 x 24 crops to swk_classifier_input_window, where a 24 x 24 crop passes
through the resize, and `net` is compared bit for bit."""
import os

import numpy as np
import pytest
import torch

import pil_resize_ref as P

pytestmark = pytest.mark.gpu

# rows x columns of the hand-written boxes: the ten with a side above 512, interleaved with three the <= 512 kernel serves
LARGE = [(513, 24), (24, 513), (512, 513), (513, 513), (3, 1299), (700, 1300), (600, 700), (1, 1025), (528, 528), (24, 1296)]
SMALL = [(24, 24), (37, 61), (512, 300)]
FH, FW = 700, 1300


def _grown(shape):
    """extract_segment_images grows a box to at least 24 x 24 (image_filtering.py:349-358)."""
    return max(shape[0], 24), max(shape[1], 24)


def _records():
    """Two frames' region records (rows x columns boxes placed where the grown box stays inside the 700 x 1300 frame) and, per segment
    of the batch, (frame, r0, r1, c0, c1) of the box extract_segment_images cuts."""
    from swiftwatcher_amd import _lib
    order = [LARGE[0], SMALL[0], LARGE[1], LARGE[2], SMALL[1], LARGE[3], LARGE[4], SMALL[2], LARGE[5], LARGE[6], LARGE[7], SMALL[0],
             LARGE[8], LARGE[9]]
    per_frame = [order[:7], order[7:]]
    cap = 8
    records = np.zeros((2, cap), _lib.SEGMENT_DTYPE)
    counts = np.zeros(2, np.int32)
    boxes = []
    for f, shapes in enumerate(per_frame):
        counts[f] = len(shapes)
        for i, (h, w) in enumerate(shapes):
            gh, gw = _grown((h, w))
            r0 = min(13 * i + 5 * f, FH - gh) + (gh - h) // 2          # a different place per record; the grown box stays in the frame
            c0 = min(29 * i + 3 * f, FW - gw) + (gw - w) // 2
            records[f, i] = (i + 1, r0, c0, r0 + h, c0 + w, 0, h * w, 0, 0)
            boxes.append((f, r0 - (gh - h) // 2, r0 - (gh - h) // 2 + gh, c0 - (gw - w) // 2, c0 - (gw - w) // 2 + gw))
    return records, counts, cap, boxes


@pytest.fixture(scope="module")
def hand_written():
    """Frames, records and the restated patches of the hand-written boxes, made once."""
    from swiftwatcher_amd import image_filtering as img
    frames = np.stack([P.formula_image(FH, FW, offset=0), P.formula_image(FH, FW, offset=101)])
    records, counts, cap, boxes = _records()
    crops = []
    for f in range(2):          # the product's own host statement of the boxes must agree with the ones written down above
        rps = img.regionprops_from_records(records[f, :counts[f]])
        crops += img.extract_segment_images(rps, frames[f], (24, 24), [(0, 0), (FW, FH)])
    assert [c.shape[:2] for c in crops] == [(b[2] - b[1], b[4] - b[3]) for b in boxes]
    for c, (f, r0, r1, c0, c1) in zip(crops, boxes):
        assert np.array_equal(c, frames[f, r0:r1, c0:c1])
    assert sorted(c.shape[:2] for c in crops if max(c.shape[:2]) > 512) == sorted(_grown(s) for s in LARGE)
    patches = [P.patch(c) for c in crops]
    frame_of = [b[0] for b in boxes]
    return frames, records, counts, cap, patches, frame_of


def _device_batch(frames, records, counts, cap):
    from swiftwatcher_amd import _lib
    dev = torch.device("cuda", 0)
    F, fh, fw = frames.shape[:3]
    dframes = torch.from_numpy(frames).to(dev)
    segs = torch.from_numpy(records.view(np.uint8).reshape(F, cap, 48)).to(dev)
    nseg = torch.from_numpy(counts).to(dev)
    torch.cuda.synchronize()
    inp = _lib.Input(frames=dframes.data_ptr(), mem=_lib.MEM_DEVICE, channels=3, nwin=1, n=F, Hc=fh, Wc=fw, x0=0, y0=0,
                     frame_stride=fh * fw * 3, row_stride=fw * 3)
    return inp, (dframes, segs, nseg)


def _expected(ctx, patches, pad):
    """(n, 3, S, S) logical network inputs of 24 x 24 patches, from the library's own <= 512 kernel (a 24 x 24 crop passes through)."""
    from swiftwatcher_amd.segment_classification import IMAGENET_MEAN, IMAGENET_STD
    _, net = ctx.classifier_input(patches, IMAGENET_MEAN, IMAGENET_STD, pad=pad)
    return net


SENTINEL = -7.25


def _cut(ctx, inp, hw, keep, cap, net_cap, pad, nhwc, first=0, guard=0):
    """swk_segment_inputs into rows guard .. guard + net_cap - 1 of a sentinel-filled (net_cap + 2 guard, 3, S, S) tensor ->
    (total, skipped, the whole tensor as logical NCHW numpy, the whole seg_frame array)."""
    from swiftwatcher_amd.segment_classification import IMAGENET_MEAN, IMAGENET_STD
    dev = torch.device("cuda", 0)
    side = 24 + 2 * pad
    fmt = torch.channels_last if nhwc else torch.contiguous_format
    x = torch.full((net_cap + 2 * guard, 3, side, side), SENTINEL, dtype=torch.float32, device=dev).contiguous(memory_format=fmt)
    fidx = torch.full((net_cap + 2 * guard,), -99, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    _, segs, nseg = keep
    total, skipped = ctx.segment_inputs(inp, hw, segs.data_ptr(), nseg.data_ptr(), cap, IMAGENET_MEAN, IMAGENET_STD,
                                        x[guard:].data_ptr(), net_cap, first=first, pad=pad, seg_frame_ptr=fidx[guard:].data_ptr(),
                                        channels_last=nhwc)
    return total, skipped, x.cpu().numpy(), fidx.cpu().numpy()


@pytest.mark.parametrize("pad,nhwc", [(100, False), (100, True), (8, False), (8, True)])
def test_boxes_with_a_side_above_512_are_resampled_on_the_device(hand_written, pad, nhwc):
    """Hand-written records giving the ten large boxes between boxes of the <= 512 route.  Before the large-crop route existed this
    reported the large boxes as skipped and left the blank image in their rows."""
    from swiftwatcher_amd import _lib
    frames, records, counts, cap, patches, frame_of = hand_written
    ctx = _lib.Context(0)
    inp, keep = _device_batch(frames, records, counts, cap)
    total, skipped, net, fidx = _cut(ctx, inp, (FH, FW), keep, cap, len(patches), pad, nhwc)
    assert total == len(patches) == 14 and skipped == 0
    assert fidx.tolist() == frame_of
    exp = _expected(ctx, patches, pad)
    for k in range(total):
        np.testing.assert_array_equal(net[k], exp[k], err_msg="segment %d" % k)
    ctx.close()


@pytest.mark.parametrize("first", [0, 2, 3, 6, 12])
def test_chunks_place_large_boxes_and_touch_nothing_else(hand_written, first):
    """net_cap = 3 at several `first`.  The batch is L s L L s L L | s L L L s L L (L = a large box): a large box is the first row of
    the chunk at first = 0, 2, 3, 6 and 12, the middle row at first = 2 and the last at first = 0, 3 and 6; first = 12 is the ragged
    end.  The chunk is written into rows 1..3 of a sentinel-filled buffer of five: row 0, row 4 and the rows past a ragged chunk
    keep the sentinel, in net and in seg_frame."""
    from swiftwatcher_amd import _lib
    frames, records, counts, cap, patches, frame_of = hand_written
    ctx = _lib.Context(0)
    inp, keep = _device_batch(frames, records, counts, cap)
    exp = _expected(ctx, patches, 8)
    total, skipped, net, fidx = _cut(ctx, inp, (FH, FW), keep, cap, 3, 8, True, first=first, guard=1)
    assert total == 14 and skipped == 0
    k = min(3, total - first)
    for j in range(k):
        np.testing.assert_array_equal(net[1 + j], exp[first + j], err_msg="row %d" % j)
    assert fidx[1:1 + k].tolist() == frame_of[first:first + k]
    assert (net[0] == SENTINEL).all() and (net[1 + k:] == SENTINEL).all() and fidx[0] == -99 and (fidx[1 + k:] == -99).all()
    ctx.close()


def test_chunk_positions_cover_first_middle_and_last():
    """The claim of the chunking test's docstring, checked: with net_cap = 3 the chosen `first` values put a large box on the first, the
    middle and the last row of a chunk."""
    _, _, _, boxes = _records()
    large = [max(b[2] - b[1], b[4] - b[3]) > 512 for b in boxes]
    assert large == [c == "L" for c in "LsLLsLLsLLLsLL"]
    seen = {j for first in (0, 2, 3, 6, 12) for j in range(min(3, len(large) - first)) if large[first + j]}
    assert seen == {0, 1, 2}


def test_tall_and_wide_boxes_match_the_pillow_8_fixture(golden_dir):
    """4096 x 25, 4096 x 40 and 3000 x 25 out of a 4096 x 40 frame, 30 x 4096 out of a 30 x 4096 frame, against the fixture written by
    a horizontal-pass-first Pillow (a newer Pillow installed beside the tests runs the vertical pass first on the tall ones)."""
    from swiftwatcher_amd import _lib
    g = np.load(os.path.join(golden_dir, "pil_resize_large.npz"))
    fixture = {tuple(int(v) for v in s): p for s, p in zip(g["shapes"], g["patches"])}
    ctx = _lib.Context(0)
    for (fh, fw), shapes in (((4096, 40), [(4096, 25), (4096, 40), (3000, 25)]), ((30, 4096), [(30, 4096)])):
        frames = P.formula_image(fh, fw)[None]          # boxes anchored at the origin: the fixture's images are the formula's corner
        records = np.zeros((1, 4), _lib.SEGMENT_DTYPE)
        for i, (h, w) in enumerate(shapes):
            records[0, i] = (i + 1, 0, 0, h, w, 0, h * w, 0, 0)
        counts = np.array([len(shapes)], np.int32)
        inp, keep = _device_batch(frames, records, counts, 4)
        patches = [fixture[s] for s in shapes]
        for s, p in zip(shapes, patches):          # the formula image of a smaller shape is the corner of the larger one's
            assert np.array_equal(P.formula_image(*s), frames[0, :s[0], :s[1]])
            np.testing.assert_array_equal(P.patch(frames[0, :s[0], :s[1]]), p)
        for pad, nhwc in ((8, True), (100, False)):
            total, skipped, net, fidx = _cut(ctx, inp, (fh, fw), keep, 4, len(shapes), pad, nhwc)
            assert total == len(shapes) and skipped == 0 and fidx.tolist() == [0] * len(shapes)
            np.testing.assert_array_equal(net, _expected(ctx, patches, pad))
    ctx.close()


def test_a_side_above_4096_is_skipped_and_left_blank():
    from swiftwatcher_amd import _lib
    from swiftwatcher_amd.segment_classification import IMAGENET_MEAN, IMAGENET_STD
    ctx = _lib.Context(0)
    frames = P.formula_image(4097, 24)[None]
    records = np.zeros((1, 2), _lib.SEGMENT_DTYPE)
    records[0, 0] = (1, 0, 0, 4097, 24, 0, 4097 * 24, 0, 0)
    records[0, 1] = (2, 1, 0, 4097, 24, 0, 4096 * 24, 0, 0)          # one row less: served
    inp, keep = _device_batch(frames, records, np.array([2], np.int32), 2)
    total, skipped, net, fidx = _cut(ctx, inp, (4097, 24), keep, 2, 2, 8, False)
    assert total == 2 and skipped == 1 and fidx.tolist() == [0, 0]
    blank = ((0.0 - np.asarray(IMAGENET_MEAN, np.float32)) / np.asarray(IMAGENET_STD, np.float32)).astype(np.float32)
    np.testing.assert_array_equal(net[0], np.broadcast_to(blank[:, None, None], net[0].shape))
    np.testing.assert_array_equal(net[1], _expected(ctx, [P.patch(frames[0, 1:])], 8)[0])
    ctx.close()


def test_device_coefficient_tables_equal_the_float64_restatement_at_every_size():
    """Bounds and 22-bit coefficients of the 24 output samples for every input size 1..4096, as the large-crop kernel forms them (two
    sweeps, no per-thread array), and for 1..512 as the kernels of the smaller crops form them: integer for integer the restatement's.
    A fused multiply-add or a changed summation order in the device code moves int(0.5 + c * 2^22) somewhere in these 4096 tables;
    image comparisons would notice only by luck."""
    from swiftwatcher_amd import _lib
    ctx = _lib.Context(0)
    ref = [P.coeff_table(size) for size in range(1, 4097)]
    for route, last in ((1, 4096), (0, 512)):
        for first in range(1, last + 1, 512):
            bounds, table = ctx.debug_resize_table(first, 512, route=route)
            for j in range(512):
                eb, et = ref[first - 1 + j]
                assert np.array_equal(bounds[j], eb) and np.array_equal(table[j], et), "input size %d, route %d" % (first + j, route)
    with pytest.raises(_lib.SwkError):
        ctx.debug_resize_table(4000, 100, route=1)
    with pytest.raises(_lib.SwkError):
        ctx.debug_resize_table(512, 2, route=0)
    ctx.close()


# ------------------------------------------------------------------ the counting loop
ROI_H, ROI_W, N = 24, 640, 5
CROP_REGION = [(30, 24), (30 + ROI_W, 24 + ROI_H)]
FRAME_HW = (72, 700)


def _bar_clip(windows=1, seed=3):
    """Windows of 5 BGR frames (oldest first): bright sky with sigma = 2.5 noise; the middle frame of every window carries a dark bar
    (contrast -80) of 5 rows x 560 columns across the 24 x 640 ROI, the others a small dark blob on either side of the bar's columns.  Every region is placed
    so that its box, grown to 24 x 24, stays inside the ROI: the ROI is so thin that the library uploads it without the margin the
    boxes could otherwise grow into (the staged buffer would be more than twice the ROI), and a box that leaves the ROI is then cut
    at its edge on the device but not on the host."""
    rng = np.random.default_rng(seed)
    (x0, y0), _ = CROP_REGION
    frames = np.empty((windows * N,) + FRAME_HW + (3,), np.uint8)
    for t in range(windows * N):
        f = np.empty(FRAME_HW + (3,), np.float64)
        f[...] = np.array([210.0, 200.0, 190.0])
        if t % N == 2:
            f[y0 + 9:y0 + 14, x0 + 40:x0 + 600] -= 80.0
        else:          # left and right of the bar's columns, at other columns in every frame
            i = (t % N) - (t % N > 2)
            f[y0 + 8:y0 + 15, x0 + 8 + 8 * i:x0 + 16 + 8 * i] -= 70.0
            f[y0 + 9:y0 + 15, x0 + 624 - 8 * i:x0 + 632 - 8 * i] -= 45.0
        f += rng.normal(0.0, 2.5, size=f.shape)
        frames[t] = np.clip(np.rint(f), 0, 255).astype(np.uint8)
    return frames


@pytest.fixture(scope="module")
def bar_scene(tmp_path_factory):
    """The clip, the CPU oracle's view of it (which proves the test is not vacuous: a region whose grown crop box is at least 513
    columns wide) and a classifier whose head is calibrated on the clip's crops with the boundary moved into a gap."""
    from helpers import oracle_frames
    from oracle import classifier_ref as ref
    from swiftwatcher_amd.segment_classification import SegmentClassifier
    clip = _bar_clip(windows=2)
    info = oracle_frames(clip, CROP_REGION, queue_size=N)
    crops = [c for fr in info for c in fr["crops"]]
    widths = [c.shape[1] for c in crops]
    assert max(widths) >= 513 and len(crops) >= 8, widths          # the oracle finds the bar as ONE region: its crop is a large box
    from oracle import reference_path as orc
    (x0, y0), (x1, y1) = CROP_REGION
    for fr in info:          # the premise of _bar_clip: no grown box leaves the ROI
        for s in fr["segments"]:
            r0, c0, r1, c1 = orc.segment_crop_box(s["bbox"], (24, 24), CROP_REGION)
            assert y0 <= r0 and r1 <= y1 and x0 <= c0 and c1 <= x1, s["bbox"]
    sd = ref.calibrate_head(ref.random_state_dict(21), crops)
    scores, _ = ref.classify(sd, crops)
    d = np.sort((scores[:, 1] - scores[:, 0]).astype(np.float64))
    gap = int(np.argmax(np.diff(d)))
    sd["classifier.1.bias"] = sd["classifier.1.bias"] - torch.tensor([0.0, float(0.5 * (d[gap] + d[gap + 1]))])
    scores, keep = ref.classify(sd, crops)
    assert np.abs(scores[:, 1] - scores[:, 0]).min() > 2e-4 and 0 < keep.sum() < len(crops)
    path = tmp_path_factory.mktemp("bar") / "w.pt"
    torch.save(sd, path)
    return clip, info, SegmentClassifier(str(path))


def _device_scores(clf, batch):
    """Scores of a window batch over the device route (what predict_last_batch runs, before its argmax)."""
    from swiftwatcher_amd.segment_classification import IMAGENET_MEAN, IMAGENET_STD

    def cut(net_ptr, frame_ptr, cap, first, pad, nhwc):
        return batch.ctx.segment_inputs_last(batch.generation, IMAGENET_MEAN, IMAGENET_STD, net_ptr, cap, first=first, pad=pad,
                                             min_seg_size=batch.min_seg_size, seg_frame_ptr=frame_ptr, channels_last=nhwc,
                                             known_total=batch.total)
    return clf._scores_device(cut)[0].cpu().numpy()


def test_frame_queue_window_with_a_wide_segment_is_classified(bar_scene):
    """FrameQueue.segment_queue + classifier(frame.segments): before the large-crop route the first classifier call of the window
    raised RuntimeError (the bar's box was counted as skipped)."""
    from swiftwatcher_amd.data_structures import FrameQueue
    clip, info, clf = bar_scene
    frames = list(clip[:N])
    q = FrameQueue(queue_size=N)
    q.push_list_of_frames(frames, list(range(N)), ["t"] * N)
    q.preprocess_queue(CROP_REGION, None)
    q.segment_queue((24, 24), CROP_REGION)
    segs = [s for f in q for s in f.segments]
    imgs = [s.segment_image for s in segs]
    assert max(im.shape[1] for im in imgs) >= 513
    batch = segs[0]._batch
    s_dev = _device_scores(clf, batch)
    s_host = clf.scores(imgs).cpu().numpy()
    np.testing.assert_allclose(s_dev, s_host, atol=1e-5, rtol=1e-5)
    want = {id(s) for s, sc in zip(segs, s_host) if sc[1] > sc[0]}
    kept = set()
    while not q.is_empty():
        f = q.pop_frame()
        kept |= {id(s) for s in clf(f.segments)}          # raised before
    assert batch.used and kept == want and 0 < len(kept) < len(segs)


def test_groups_call_with_a_wide_segment_is_classified(bar_scene):
    """The same window beside a group of another geometry (60 x 120) in one swk_batch_run_groups call: k_segment_inputs_groups lists
    the wide box and the large kernel reads its frame through the call's frame descriptors."""
    from swiftwatcher_amd import synthetic
    from swiftwatcher_amd.data_structures import segment_window_groups
    clip, info, clf = bar_scene
    other_region = [(20, 10), (20 + 120, 10 + 60)]
    other = synthetic.full_frames(5, N, other_region, frame_hw=(90, 170), birds=3, bird_len=(14, 22), bird_wid=(6, 10))[::-1].copy()
    groups = [([(list(other), list(range(N)), ["t"] * N)], other_region),
              ([(list(clip[:N]), list(range(N)), ["t"] * N)], CROP_REGION)]
    out = segment_window_groups(groups, (24, 24), classifier=clf)
    frames = [fr for g in out for popped in g for fr in popped]
    segs = [s for fr in frames for s in fr.segments]
    assert len({id(s._batch) for s in segs}) == 1
    by_index = sorted(segs, key=lambda s: s._index)
    imgs = [s.segment_image for s in by_index]
    assert max(im.shape[1] for im in imgs) >= 513 and any(fr.segments for fr in out[0][0])
    s_dev = _device_scores(clf, by_index[0]._batch)
    s_host = clf.scores(imgs).cpu().numpy()
    np.testing.assert_allclose(s_dev, s_host, atol=1e-5, rtol=1e-5)
    want = {id(s) for s, sc in zip(by_index, s_host) if sc[1] > sc[0]}
    clf.classify_frames(frames)
    assert {id(s) for fr in frames for s in fr.segments} == want


class _HostCrops:
    """A classifier that scores the segments' images: the link to the window's device state is removed first."""

    def __init__(self, clf):
        self.clf = clf

    def __call__(self, segments):
        for s in segments:
            s.__dict__.pop("_batch", None)
        return self.clf(segments)


def test_counting_loop_runs_through_a_wide_segment(bar_scene):
    """pipeline.count_swifts with the classifier on over two windows that each hold the bar: runs to the end (it raised before), with
    the events of a run that scores host crops (Pillow resize) instead."""
    from helpers import event_signature
    from swiftwatcher_amd import pipeline
    clip, info, clf = bar_scene
    roi_mask = np.zeros((ROI_H, ROI_W), np.uint8)
    roi_mask[ROI_H // 2:, 64:576] = 255
    count, events = pipeline.count_swifts(list(clip), CROP_REGION, roi_mask, classifier=clf, queue_size=N)
    count_h, events_h = pipeline.count_swifts(list(clip), CROP_REGION, roi_mask, classifier=_HostCrops(clf), queue_size=N)
    assert count == count_h and event_signature(events) == event_signature(events_h)
