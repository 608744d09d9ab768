"""The counting loops with the tracker stepped a window per call (track_by_window=True, SegmentTracker.step_window) against the same
loops stepping it per frame (False): equal counts and equal events, on small synthetic clips whose last window is padded with null
frames, with and without the reference's classifier between segmentation and tracker."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# (x0, y0, ROI width, ROI height, frames, frame size): three or four 21-frame windows each, none a multiple of 21
GEOMETRY = [(30, 20, 96, 48, 72, (90, 160)), (12, 30, 120, 64, 47, (110, 150)), (8, 8, 80, 40, 58, (60, 100))]


@pytest.fixture(scope="module")
def clips():
    """(frames oldest first, crop region, ROI mask) per clip.  Small faint birds: the kind of synthetic blob of which the reference's
    trained weights keep a fair share (tests/test_baseline_configs.py), so that the tracker behind the classifier still sees tracks."""
    from swiftwatcher_amd import synthetic
    out = []
    for k, (x0, y0, w, h, total, hw) in enumerate(GEOMETRY):
        crop_region = [(x0, y0), (x0 + w, y0 + h)]
        clip = synthetic.full_frames(311 + k, total, crop_region, frame_hw=hw, birds=8, bird_len=(5, 8), bird_wid=(4, 6), contrast=(25, 40))[::-1].copy()
        mask = np.zeros((h, w), np.uint8)
        mask[h * 2 // 5:, :] = 255
        out.append((clip, crop_region, mask))
    return out


@pytest.fixture(scope="module")
def model_pt(golden_dir):
    import tempfile
    import torch
    from swiftwatcher_amd.segment_classification import SegmentClassifier
    g = np.load(os.path.join(golden_dir, "classifier_model_pt.npz"))
    sd = {k[2:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("w:")}
    with tempfile.TemporaryDirectory() as d:
        torch.save(sd, os.path.join(d, "model.pt"))
        return SegmentClassifier(os.path.join(d, "model.pt"))


def _key(events):
    return [[(s.parent_frame_number, s.label, s.centroid) for s in e] for e in events]


@pytest.mark.parametrize("classified", [False, True], ids=["plain", "classifier"])
def test_count_swifts_by_window_equals_per_frame(clips, model_pt, classified):
    from swiftwatcher_amd import pipeline
    clf = model_pt if classified else None
    events = 0
    for clip, crop_region, mask in clips:
        by_frame = pipeline.count_swifts(list(clip), crop_region, mask, windows_per_call=2, classifier=clf, track_by_window=False)
        by_window = pipeline.count_swifts(list(clip), crop_region, mask, windows_per_call=2, classifier=clf, track_by_window=True)
        print("count_swifts, classifier %s: count %d, %d events" % (classified, by_frame[0], len(by_frame[1])))
        assert by_window[0] == by_frame[0]
        assert _key(by_window[1]) == _key(by_frame[1])
        events += len(by_frame[1])
    assert events >= (1 if classified else 6)          # the clips do make events, behind the classifier too


@pytest.mark.parametrize("classified", [False, True], ids=["plain", "classifier"])
def test_count_swifts_videos_by_window_equals_per_frame(clips, model_pt, classified):
    from swiftwatcher_amd import pipeline
    clf = model_pt if classified else None
    kw = dict(regions=[(cr, m) for _, cr, m in clips], in_flight=2, windows_per_call=2, classifier=clf)
    by_frame = pipeline.count_swifts_videos([list(c) for c, _, _ in clips], track_by_window=False, **kw)
    by_window = pipeline.count_swifts_videos([list(c) for c, _, _ in clips], track_by_window=True, **kw)
    print("count_swifts_videos, classifier %s: counts %s, events %s" % (classified, [c for c, _ in by_frame], [len(e) for _, e in by_frame]))
    assert len(by_window) == len(by_frame) == len(clips)
    for (cnt, ev), (cnt0, ev0) in zip(by_window, by_frame):
        assert cnt == cnt0
        assert _key(ev) == _key(ev0)
    assert sum(len(ev) for _, ev in by_frame) >= (1 if classified else 6)
