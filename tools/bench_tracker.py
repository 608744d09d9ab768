"""The tracker alone, on the host: replays recorded traces (tests/golden/tracker_crowd.npz, tracker_long.npz) from Segment-like objects
made beforehand, once per frame (SegmentTracker.step) and once by 21-frame windows (SegmentTracker.step_window), and reports ms per
window for both -- median and min-max of 15 replays after two warm-up replays -- and their ratio.  No GPU.

    python tools/bench_tracker.py [--replays 15] [--warmup 2] [--window 21]

Prints one JSON line per trace."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from swiftwatcher_amd.data_structures import Frame          # noqa: E402
from swiftwatcher_amd.segment_tracking import SegmentTracker          # noqa: E402


class _Seg:
    __slots__ = ("label", "centroid", "status", "segment_history", "parent_frame_number", "parent_timestamp")

    def __init__(self, label, centroid, t):
        self.label, self.centroid, self.status, self.segment_history = label, centroid, None, []
        self.parent_frame_number, self.parent_timestamp = t, "ts%05d" % t


def _frames(g):
    out, off = [], 0
    cents = g["centroids"]
    for t, k in enumerate(g["counts"].tolist()):
        fr = Frame(None, t, "ts%05d" % t)
        fr.segments = [_Seg(i + 1, (float(cents[off + i, 0]), float(cents[off + i, 1])), t) for i in range(k)]
        off += k
        out.append(fr)
    return out


def _replay(g, frames, window, by_window):
    tracker = SegmentTracker(g["roi"])
    t0 = time.perf_counter()
    if by_window:
        for at in range(0, len(frames), window):
            tracker.step_window(frames[at:at + window])
    else:
        for fr in frames:
            tracker.step(fr)
    dt = time.perf_counter() - t0
    return dt, [[(s.parent_frame_number, s.label) for s in e] for e in tracker.detected_events]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replays", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--window", type=int, default=21)
    args = ap.parse_args()
    for name in ("tracker_crowd", "tracker_long"):
        g = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))
        g = {k: g[k] for k in g.files}
        windows = -(-len(g["counts"]) // args.window)
        ms = {False: [], True: []}
        events = {}
        for rep in range(args.warmup + args.replays):
            for by_window in (False, True):                      # alternating, on fresh objects made outside the timed part
                dt, events[by_window] = _replay(g, _frames(g), args.window, by_window)
                if rep >= args.warmup:
                    ms[by_window].append(1e3 * dt / windows)
        if events[True] != events[False]:
            raise SystemExit("%s: the two paths disagree" % name)
        med = {k: statistics.median(v) for k, v in ms.items()}
        print(json.dumps({"trace": name, "frames": int(len(g["counts"])), "segments_per_frame": round(float(g["counts"].mean()), 2),
                          "events": len(events[True]), "window": args.window, "replays": args.replays,
                          "per_frame_ms_per_window": {"median": round(med[False], 4), "min": round(min(ms[False]), 4), "max": round(max(ms[False]), 4)},
                          "by_window_ms_per_window": {"median": round(med[True], 4), "min": round(min(ms[True]), 4), "max": round(max(ms[True]), 4)},
                          "ratio": round(med[False] / med[True], 2)}))


if __name__ == "__main__":
    main()
