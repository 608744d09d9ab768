"""The cost of the segments' shape properties (csrc/shape_props.hip, shape_props=True).
1. The call alone: swk_segment_shapes_u8 on the device label planes of one window of the bench geometry (424 x 212, n = 64, a
   synthetic.py scene), as FrameQueue(shape_props=True) makes it (seg_cap = the window's largest segment count) and at seg_cap 255,
   beside swk_batch_run on the same window, alternating, `repeats` blocks of `reps` calls each: wall-clock ms per (synchronous) call,
   median and min-max over the blocks.  The host derivation of every float of every segment of the window is timed too.
2. The counting loop: pipeline.count_swifts over a seeded synthetic clip (crop region 424 x 212) with and without shape_props=True,
   alternating round by round, and a third variant that also reads every event segment's orientation once (the lazy derivation is
   part of the cost a user pays).  Reports frames/s of each and their ratios.
    python tools/bench_shape_props.py [--reps 50] [--repeats 5] [--rounds 5] [--frames 210] [--windows-per-call 2]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from swiftwatcher_amd import _lib          # noqa: E402


def call_rows(ctx, reps, repeats):
    from swiftwatcher_amd import image_filtering as img, synthetic
    Wc, Hc, n = 424, 212, 64
    stack = np.ascontiguousarray(synthetic.roi_window(7, n, **synthetic.P2))
    res = ctx.batch_run(stack, 1, n, stages=("labels",), device_stages=True)
    planes, nseg = res["planes"], res["nseg"]
    cap = max(int(nseg.max()), 1)
    calls = {"batch_run": lambda: ctx.batch_run(stack, 1, n, stages=("labels",), device_stages=True),
             "shapes": lambda: ctx.segment_shapes_u8(planes, seg_cap=cap),
             "shapes_cap255": lambda: ctx.segment_shapes_u8(planes, seg_cap=255)}
    ms = {name: [] for name in calls}
    for call in calls.values():
        for _ in range(3):
            call()
    for _ in range(repeats):
        for name, call in calls.items():
            t0 = time.perf_counter()
            for _ in range(reps):
                call()
            ms[name].append((time.perf_counter() - t0) / reps * 1e3)
    recs, count = ctx.segment_shapes_u8(planes, seg_cap=cap)
    live = recs[np.arange(cap)[None, :] < count[:, None]]
    segs = res["segs"][np.arange(res["segs"].shape[1])[None, :] < nseg[:, None]]
    t0 = time.perf_counter()
    for s, rec in zip(segs, img.shape_records(live)):
        m = img.ShapeMeasures((int(s["r0"]), int(s["c0"]), int(s["r1"]), int(s["c1"])), rec)
        for name in img.SHAPE_PROPERTIES:
            getattr(m, name)
    derive_ms = (time.perf_counter() - t0) * 1e3
    row = {"bench": "shape_call", "Wc": Wc, "Hc": Hc, "frames": n, "segments": int(nseg.sum()), "seg_cap": cap, "reps": reps, "repeats": repeats,
           "label_bytes": n * Hc * Wc, "derive_all_properties_ms_per_segment": round(derive_ms / max(len(segs), 1), 4)}
    for name in calls:
        row[name + "_ms"] = round(float(np.median(ms[name])), 4)
        row[name + "_ms_min_max"] = [round(min(ms[name]), 4), round(max(ms[name]), 4)]
    row["shapes_over_batch_run"] = round(row["shapes_ms"] / row["batch_run_ms"], 4)
    return [row]


def loop_rows(frames_n, rounds, wpc):
    from swiftwatcher_amd import pipeline, synthetic
    crop = [(28, 29), (28 + 424, 29 + 212)]
    frames = synthetic.full_frames(500, frames_n, crop, frame_hw=(270, 480))[::-1].copy()
    roi_mask = np.zeros((212, 424), np.uint8)
    roi_mask[int(212 * 0.8):, :] = 255
    kw = dict(crop_region=crop, roi_mask=roi_mask, windows_per_call=wpc)
    want = pipeline.count_swifts(frames, **kw)                                   # warm-up, and the count both variants must give
    pipeline.count_swifts(frames, shape_props=True, **kw)
    times = {"plain": [], "shape": [], "shape_read": []}
    for _ in range(rounds):
        for name in times:
            t0 = time.perf_counter()
            got = pipeline.count_swifts(frames, **({} if name == "plain" else {"shape_props": True}), **kw)
            if name == "shape_read":
                for ev in got[1]:
                    for s in ev:
                        s.orientation
            times[name].append(time.perf_counter() - t0)
            assert got[0] == want[0] and len(got[1]) == len(want[1])
    med = {k: float(np.median(v)) for k, v in times.items()}
    return [{"bench": "shape_loop", "frames": frames_n, "windows_per_call": wpc, "crop": [424, 212], "events": len(want[1]),
             "event_segments": sum(len(ev) for ev in want[1]), "plain_fps": round(frames_n / med["plain"], 1),
             "shape_fps": round(frames_n / med["shape"], 1), "plain_s": [round(t, 4) for t in times["plain"]],
             "shape_s": [round(t, 4) for t in times["shape"]], "shape_over_plain": round(med["shape"] / med["plain"], 4),
             "shape_extra_ms_per_frame": round((med["shape"] - med["plain"]) / frames_n * 1e3, 4),
             "shape_read_fps": round(frames_n / med["shape_read"], 1), "shape_read_s": [round(t, 4) for t in times["shape_read"]],
             "read_ms_per_event_segment": round((med["shape_read"] - med["shape"]) / max(sum(len(ev) for ev in want[1]), 1) * 1e3, 4)}]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--frames", type=int, default=210)
    ap.add_argument("--windows-per-call", type=int, default=2)
    a = ap.parse_args()
    ctx = _lib.default_context(0)
    for row in call_rows(ctx, a.reps, a.repeats):
        print(json.dumps(row), flush=True)
    for wpc in sorted({1, a.windows_per_call}):
        for row in loop_rows(a.frames, a.rounds, wpc):
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
