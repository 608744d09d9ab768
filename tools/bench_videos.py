"""Several videos at once on one GPU: aggregate ROI frames/s of count_swifts_videos (swk_batch_run_groups, in_flight videos per
call) against counting the same clips one after another with count_swifts.  Synthetic clips, each with its own chimney geometry
(crop region), lengths not multiples of the queue size; the classifier runs with model.pt's weights (tests/golden).

    python tools/bench_videos.py [--clips 8] [--frames 300] [--in-flight 1,2,4,8] [--windows-per-call 1] [--no-classifier]

Prints one JSON line: frames/s of every run and the counts each run produced (they must agree)."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# (x0, y0, width, height) of each clip's crop region: chimneys of different widths (generate_crop_region sizes the ROI from them)
GEOMETRIES = [(40, 30, 214, 107), (60, 40, 180, 90), (20, 50, 260, 120), (80, 20, 128, 64), (30, 60, 240, 100), (100, 35, 160, 80),
              (50, 45, 300, 140), (70, 25, 200, 96)]


def make_clips(count, frames, seed=500):
    from swiftwatcher_amd import synthetic
    clips = []
    for k in range(count):
        x0, y0, w, h = GEOMETRIES[k % len(GEOMETRIES)]
        crop_region = [(x0, y0), (x0 + w, y0 + h)]
        total = frames + 7 * k + 5                                  # not a multiple of 21
        clip = synthetic.full_frames(seed + k, total, crop_region, frame_hw=(y0 + h + 40, x0 + w + 40), birds=4, bird_len=(10, 14),
                                     bird_wid=(4, 6))[::-1].copy()
        mask = np.zeros((h, w), np.uint8)
        mask[h * 2 // 5:, :] = 255
        clips.append((list(clip), crop_region, mask))
    return clips


def load_classifier():
    import torch
    from swiftwatcher_amd.segment_classification import SegmentClassifier
    g = np.load(os.path.join(ROOT, "tests", "golden", "classifier_model_pt.npz"))
    sd = {k[2:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("w:")}
    with tempfile.TemporaryDirectory() as d:
        torch.save(sd, os.path.join(d, "model.pt"))
        return SegmentClassifier(os.path.join(d, "model.pt"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=8)
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--in-flight", default="1,2,4,8")
    ap.add_argument("--windows-per-call", type=int, default=1)
    ap.add_argument("--no-classifier", action="store_true")
    a = ap.parse_args()
    import torch
    from swiftwatcher_amd import pipeline
    clips = make_clips(a.clips, a.frames)
    frames = sum(len(c) for c, _, _ in clips)
    clf = None if a.no_classifier else load_classifier()
    regions = [(cr, m) for _, cr, m in clips]
    pipeline.count_swifts(clips[0][0][:64], clips[0][1], clips[0][2], classifier=clf)          # warm-up: context, kernels, graphs

    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return out, time.perf_counter() - t

    seq, dt = timed(lambda: [pipeline.count_swifts(c, cr, m, classifier=clf) for c, cr, m in clips])
    result = {"metric": "video_groups_fps", "clips": a.clips, "frames": frames, "classifier": clf is not None,
              "windows_per_call": a.windows_per_call, "sequential": {"fps": round(frames / dt, 1), "counts": [c for c, _ in seq]}}
    ok = True
    for k in (int(x) for x in a.in_flight.split(",")):
        got, dt = timed(lambda: pipeline.count_swifts_videos([c for c, _, _ in clips], regions=regions, in_flight=k,
                                                             windows_per_call=a.windows_per_call, classifier=clf))
        counts = [c for c, _ in got]
        ok = ok and counts == result["sequential"]["counts"]
        result["in_flight_%d" % k] = {"fps": round(frames / dt, 1), "counts": counts}
    result["counts_agree"] = ok
    print(json.dumps(result))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
