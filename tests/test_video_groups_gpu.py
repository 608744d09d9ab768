"""swk_batch_run_groups: several videos' windows, each at its own geometry, in one library call.  Every group must come out as
swk_batch_run gives it on that group alone (u8 stages, iterations, region records; A / E to float64 summation order, and bit for
bit when the call has one group), and as the CPU oracle segments it; segment_window_groups / count_swifts_videos must count every video as count_swifts does."""
import os

import numpy as np
import pytest

from helpers import STAGES, roi_stack
from helpers import gray_u8 as _gray, lone_run as _lone, check_against_lone_and_oracle as _check_against_lone_and_oracle

pytestmark = pytest.mark.gpu

N = 21


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


def _rois(seed, nwin, Hc, Wc, null_tail=()):
    return roi_stack(seed, nwin, Hc, Wc, n=N, null_tail=null_tail)


def _mixed_groups(small=False, null_tails=False):
    """(spec for batch_run_groups, BGR ROI stack per group in queue order) of the issue's four geometries (+ a 4 x 4 one)"""
    import torch
    specs, rois = [], []
    # 64 x 96 BGR, host memory, two windows
    r0 = _rois(11, 2, 64, 96, null_tail=(0, 9) if null_tails else ())
    specs.append(dict(frames=r0, nwin=2, n=N))
    rois.append(r0)
    # 47 x 94 cropped out of full frames (x0, y0 != 0)
    r1 = _rois(23, 1, 47, 94, null_tail=(5,) if null_tails else ())
    full = np.full((N, 70, 130, 3), 200, np.uint8)
    full[:, 9:56, 13:107] = r1
    specs.append(dict(frames=full, nwin=1, n=N, crop=(13, 9, 94, 47)))
    rois.append(r1)
    # 107 x 214 gray, device memory
    r2 = _rois(37, 1, 107, 214)
    specs.append(dict(frames=torch.from_numpy(_gray(r2)).cuda(), nwin=1, n=N))
    rois.append(r2)
    # 30 x 40, negative frame stride (the window lies oldest first in memory)
    r3 = _rois(41, 1, 30, 40, null_tail=(12,) if null_tails else ())
    specs.append(dict(frames=np.ascontiguousarray(r3[::-1]), nwin=1, n=N, reverse_frames=True))
    rois.append(r3)
    if small:
        r4 = _rois(53, 1, 4, 4)
        specs.insert(1, dict(frames=r4, nwin=1, n=N))
        rois.insert(1, r4)
    return specs, rois


@pytest.mark.parametrize("ae", [False, True], ids=["mstate", "with_A_E"])
def test_mixed_geometries_match_lone_runs_and_oracle(ctx, orc, ae):
    specs, rois = _mixed_groups()
    got = _check_against_lone_and_oracle(ctx, orc, specs, rois, ae)
    assert sum(int(r["nseg"].sum()) for r in got) > 20
    for g in (0, 2):          # one group alone: host BGR frames, device gray frames
        _check_against_lone_and_oracle(ctx, orc, specs[g:g + 1], rois[g:g + 1], ae)


def test_windows_smaller_than_n_pixels_run_at_their_own_size(ctx, orc):
    specs, rois = _mixed_groups(small=True)
    _check_against_lone_and_oracle(ctx, orc, specs, rois, ae=True)


def test_windows_that_end_in_null_frames(ctx, orc):
    specs, rois = _mixed_groups(null_tails=True)
    _check_against_lone_and_oracle(ctx, orc, specs, rois, ae=False)


def _model_pt_classifier(golden_dir):
    import tempfile
    import torch
    from swiftwatcher_amd.segment_classification import SegmentClassifier
    g = np.load(os.path.join(golden_dir, "classifier_model_pt.npz"))
    sd = {k[2:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("w:")}
    with tempfile.TemporaryDirectory() as d:
        torch.save(sd, os.path.join(d, "model.pt"))
        return SegmentClassifier(os.path.join(d, "model.pt"))


def test_segment_inputs_and_scores_after_a_groups_call(ctx, golden_dir):
    """swk_segment_inputs_last after a groups call = every group's inputs, concatenated; model.pt's scores bit-identical to
    scoring each group's batch alone (the head kernel is batch-independent)."""
    import torch
    from swiftwatcher_amd import _lib
    from swiftwatcher_amd.segment_classification import IMAGENET_MEAN, IMAGENET_STD
    clf = _model_pt_classifier(golden_dir)
    specs, _ = _mixed_groups()
    specs = [s for s in specs if not hasattr(s["frames"], "cpu")]          # BGR groups: the classifier cuts colour crops
    side = 24 + 2 * 8

    def inputs(generation, total):
        net = torch.zeros((max(total, 1), 3, side, side), dtype=torch.float32, device="cuda")
        fr = torch.zeros((max(total, 1),), dtype=torch.int32, device="cuda")
        t, skipped = ctx.segment_inputs_last(generation, IMAGENET_MEAN, IMAGENET_STD, net.data_ptr(), max(total, 1), pad=8,
                                             seg_frame_ptr=fr.data_ptr(), known_total=total)
        assert t == total and skipped == 0
        return net[:total].cpu(), fr[:total].cpu()

    def scores(generation, total):
        def cut(net_ptr, frame_ptr, cap, first, pad, nhwc):
            return ctx.segment_inputs_last(generation, IMAGENET_MEAN, IMAGENET_STD, net_ptr, cap, first=first, pad=pad,
                                           seg_frame_ptr=frame_ptr, channels_last=nhwc, known_total=total)
        return clf._scores_device(cut)[0].cpu()

    got = ctx.batch_run_groups(specs)
    total = sum(int(np.minimum(r["nseg"], 255).sum()) for r in got)
    assert total > 10
    net_g, fr_g = inputs(got[0]["generation"], total)
    sc_g = scores(got[0]["generation"], total)
    nets, frs, scs, f0 = [], [], [], 0
    for spec in specs:
        lone = _lone(ctx, spec)
        t = int(lone["nseg"].sum())
        net, fr = inputs(lone["generation"], t)
        nets.append(net)
        frs.append(fr + f0)
        scs.append(scores(lone["generation"], t))
        f0 += spec["nwin"] * N
    assert torch.equal(net_g, torch.cat(nets))
    assert torch.equal(fr_g, torch.cat(frs))
    assert torch.equal(sc_g, torch.cat(scs)), "scores of a groups call differ from per-group scoring"
    # the context has moved on: the groups call's batch is stale now
    with pytest.raises(_lib.StaleBatch):
        inputs(got[0]["generation"], total)


def _clips():
    """five synthetic clips with different chimney geometries, lengths not multiples of 21: (frames oldest first, crop, mask)"""
    from swiftwatcher_amd import synthetic
    out = []
    for k, (x0, y0, w, h, total, hw) in enumerate([(30, 20, 160, 96, 52, (140, 230)), (12, 30, 120, 64, 47, (110, 150)),
                                                    (40, 10, 200, 110, 65, (150, 260)), (8, 8, 96, 48, 30, (70, 120)),
                                                    (25, 15, 140, 80, 44, (120, 200))]):
        crop_region = [(x0, y0), (x0 + w, y0 + h)]
        clip = synthetic.full_frames(77 + k, total, crop_region, frame_hw=hw, birds=4, bird_len=(10, 14), bird_wid=(4, 6))[::-1].copy()
        mask = np.zeros((h, w), np.uint8)
        mask[h * 2 // 5:, :] = 255
        out.append((clip, crop_region, mask))
    return out


def _events_key(events):
    return [[(s.parent_frame_number, s.label, s.bbox, s.centroid) for s in e] for e in events]


def test_count_swifts_videos_equals_count_swifts_per_video(orc):
    from swiftwatcher_amd import pipeline
    from swiftwatcher_amd import event_classification as ec
    from swiftwatcher_amd.segment_tracking import SegmentTracker
    from swiftwatcher_amd.data_structures import Frame, Segment
    from swiftwatcher_amd.image_filtering import RegionProps
    from swiftwatcher_amd.io_frames import ArrayReader
    clips = _clips()
    alone = [pipeline.count_swifts(list(c), cr, m) for c, cr, m in clips]
    assert sum(len(ev) for _, ev in alone) >= 3
    for in_flight in (1, 2, 4):
        for wpc in (1, 8):
            got = pipeline.count_swifts_videos([list(c) for c, _, _ in clips], regions=[(cr, m) for _, cr, m in clips],
                                               in_flight=in_flight, windows_per_call=wpc)
            assert len(got) == len(clips)
            for v, ((cnt, ev), (cnt0, ev0)) in enumerate(zip(got, alone)):
                assert cnt == cnt0, (in_flight, wpc, v)
                assert _events_key(ev) == _events_key(ev0), (in_flight, wpc, v)
    # the CPU restatement's pipeline on the first clip: oracle windows -> the same tracker
    clip, crop_region, mask = clips[0]
    (x0, y0), (x1, y1) = crop_region
    reader = ArrayReader(list(clip))
    tracker = SegmentTracker(mask)
    processed = 0
    while processed < reader.total_frames:
        frames, numbers, stamps = reader.get_n_frames(N)
        ref = orc.window(np.ascontiguousarray(np.stack([f[y0:y1, x0:x1] for f in frames][::-1])))
        for pos in range(N - 1, -1, -1):
            k = N - 1 - pos
            fr = Frame(None, numbers[k], stamps[k])
            fr.segments = [Segment(RegionProps(s["label"], s["bbox"], s["centroid"], s["area"]), fr.frame_number, fr.timestamp, None)
                           for s in ref["segments"][pos]]
            tracker.step(fr)
            processed += 0 if fr.null else 1
    cnt0, ev0 = alone[0]
    assert [(e[-1].parent_frame_number, len(e)) for e in ev0] == [(e[-1].parent_frame_number, len(e)) for e in tracker.detected_events]
    assert cnt0 == ec.count_swifts(tracker.detected_events)


def test_errors_leave_the_context_usable(ctx, orc):
    from swiftwatcher_amd import _lib
    specs, rois = _mixed_groups()
    host = [s for s in specs if isinstance(s["frames"], np.ndarray)]
    lone = _lone(ctx, host[0])
    # mismatched n
    odd = dict(frames=host[0]["frames"][:2 * 20], nwin=2, n=20)
    with pytest.raises(_lib.SwkError):
        ctx.batch_run_groups([host[0], odd])
    again = _lone(ctx, host[0])
    for key in STAGES + ("nseg", "iters"):
        assert np.array_equal(again[key], lone[key]), key
    # one group below 4 x 4 among valid ones: refused before anything is written
    tiny = dict(frames=np.zeros((N, 3, 8, 3), np.uint8), nwin=1, n=N)
    params = _lib.default_params()
    ins = (_lib.Input * 2)()
    outs = (_lib.Output * 2)()
    opened = np.full((N, 64, 96), 7, np.uint8)
    f0 = host[0]["frames"][:N]
    ins[0] = _lib.Input(frames=f0.ctypes.data, mem=_lib.MEM_HOST, channels=3, nwin=1, n=N, Hc=64, Wc=96, x0=0, y0=0,
                        frame_stride=f0.strides[0], row_stride=f0.strides[1])
    ins[1] = _lib.Input(frames=tiny["frames"].ctypes.data, mem=_lib.MEM_HOST, channels=3, nwin=1, n=N, Hc=3, Wc=8, x0=0, y0=0,
                        frame_stride=tiny["frames"].strides[0], row_stride=tiny["frames"].strides[1])
    outs[0] = _lib.Output(mem=_lib.MEM_HOST, seg_cap=255, opened=opened.ctypes.data)
    outs[1] = _lib.Output(mem=_lib.MEM_HOST, seg_cap=255)
    lib = _lib.load()
    import ctypes
    assert lib.swk_batch_run_groups(ctx._h, ins, 2, ctypes.byref(params), outs) == -1          # SWK_ERR_ARG
    assert (opened == 7).all(), "a refused call wrote output"
    # swk_batch_run runs the same checks, the call-level limits included, before anything is launched or written
    big = _lib.Input.from_buffer_copy(ins[0])
    big.nwin, big.frame_stride = (1 << 24) // N + 1, 0          # more than 2^24 frames (all the same one)
    assert lib.swk_batch_run(ctx._h, ctypes.byref(big), ctypes.byref(params), ctypes.byref(outs[0])) == -1
    assert (opened == 7).all(), "a refused swk_batch_run wrote output"
    ins[1].n = 20
    ins[1].Hc = 8
    assert lib.swk_batch_run_groups(ctx._h, ins, 2, ctypes.byref(params), outs) == -1          # mismatched n, raw
    assert (opened == 7).all()
    again = _lone(ctx, host[0])
    for key in STAGES + ("nseg", "iters"):
        assert np.array_equal(again[key], lone[key]), key
    ref = orc.window(np.ascontiguousarray(rois[0][:N]))
    assert np.array_equal(again["labels"][:N], ref["labels"])
