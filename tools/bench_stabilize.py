"""The cost of stabilization (csrc/stabilize.hip, stabilize=S).
1. The call alone: swk_stabilize_u8 at the bench workload's region -- 424 x 212 plus the 12-px margin = a 448 x 236 rectangle, its
   source grown by S on every side --, 21 and 64 frames, S = 4, 8, 16, a synthetic.py scene.  Source, anchor and output in device
   memory (the kernels and the synchronous call's overhead), and, at S = 8, in host memory (what a reader of decoded frames pays:
   the upload of the source and the download of the rectangles included).  `repeats` blocks of `reps` calls each, alternating:
   wall-clock ms per call, median and min-max over the blocks.
2. The counting loop: pipeline.count_swifts over a seeded synthetic clip (crop region 424 x 212 in 480 x 270 pictures) with and
   without stabilize=8, alternating round by round: frames/s of each, their ratio, and where a window's extra time goes -- the
   reader's get_n_frames alone (staging the search rectangles, the call, the anchor) and the library call inside it.
--subpel adds the quarter-pixel stage (swk_stabilize_subpel_u8, stabilize_subpel=True) to both: the call at S = 8 on the same
sources, device and host, beside swk_stabilize_u8 in the same blocks ("subpel_device_s8", "subpel_host_s8"), and the counting loop
with stabilize=8, stabilize_subpel=True as a third variant of every round.
    python tools/bench_stabilize.py [--subpel] [--reps 30] [--repeats 5] [--rounds 5] [--frames 210] [--windows-per-call 2]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from swiftwatcher_amd import _lib          # noqa: E402

HO, WO = 212 + 24, 424 + 24


def call_rows(ctx, reps, repeats, subpel=False):
    import torch
    from swiftwatcher_amd import synthetic
    rows = []
    for n in (21, 64):
        calls, meta = {}, {}
        for S in (4, 8, 16):
            Hs, Ws = HO + 2 * S, WO + 2 * S
            frames = np.ascontiguousarray(synthetic.roi_window(11, n, Hs, Ws, birds=12))
            anchor = ctx.bgr2gray(np.ascontiguousarray(frames[0][S:S + HO, S:S + WO]))
            dev, danchor = torch.from_numpy(frames).cuda(), torch.from_numpy(anchor).cuda()
            rect = (S, S, HO, WO)
            calls["device_s%d" % S] = lambda d=dev, a=danchor, r=rect, s=S: ctx.stabilize(d, r, s, a, device_out=True)
            if S == 8:
                calls["host_s%d" % S] = lambda f=frames, a=anchor, r=rect, s=S: ctx.stabilize(f, r, s, a)
                if subpel:
                    calls["subpel_device_s%d" % S] = lambda d=dev, a=danchor, r=rect, s=S: ctx.stabilize_subpel(d, r, s, a, device_out=True)
                    calls["subpel_host_s%d" % S] = lambda f=frames, a=anchor, r=rect, s=S: ctx.stabilize_subpel(f, r, s, a)
            meta[S] = dict(source_bytes=int(frames.nbytes), out_bytes=n * HO * WO * 3, candidates=(2 * S + 1) ** 2)
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
        row = {"bench": "stabilize_call", "Wo": WO, "Ho": HO, "frames": n, "reps": reps, "repeats": repeats, "sizes": meta}
        for name in calls:
            row[name + "_ms"] = round(float(np.median(ms[name])), 4)
            row[name + "_ms_min_max"] = [round(min(ms[name]), 4), round(max(ms[name]), 4)]
        rows.append(row)
    return rows


def loop_rows(frames_n, rounds, wpc, search=8, subpel=False):
    from swiftwatcher_amd import pipeline, synthetic
    from swiftwatcher_amd.io_frames import ArrayReader
    from swiftwatcher_amd.stabilize import StabilizingReader
    crop = [(28, 29), (28 + 424, 29 + 212)]
    frames = synthetic.full_frames(500, frames_n, crop, frame_hw=(270, 480))[::-1].copy()
    roi_mask = np.zeros((212, 424), np.uint8)
    roi_mask[int(212 * 0.8):, :] = 255
    kw = dict(crop_region=crop, roi_mask=roi_mask, windows_per_call=wpc)
    want = pipeline.count_swifts(frames, **kw)                                   # warm-up, and the count both variants must give
    pipeline.count_swifts(frames, stabilize=search, **kw)
    variants = {"plain": {}, "stabilized": {"stabilize": search}}
    if subpel:
        variants["subpel"] = {"stabilize": search, "stabilize_subpel": True}
        pipeline.count_swifts(frames, **variants["subpel"], **kw)
    times = {name: [] for name in variants}
    for _ in range(rounds):
        for name in times:
            t0 = time.perf_counter()
            got = pipeline.count_swifts(frames, **variants[name], **kw)
            times[name].append(time.perf_counter() - t0)
            if name != "subpel":                         # (a clip that does not move: every integer shift is (0, 0); noise can move the
                assert got[0] == want[0] and len(got[1]) == len(want[1])             # quarter-pixel choice of a frame)
    # where a window's extra time goes: the reader alone, and the library call inside it
    ctx = _lib.default_context(0)
    inner, spent = ctx.stabilize, []

    def timed(*a, **k):
        t0 = time.perf_counter()
        out = inner(*a, **k)
        spent.append(time.perf_counter() - t0)
        return out
    ctx.stabilize = timed
    try:
        per_window = []
        for _ in range(rounds):
            reader = StabilizingReader(ArrayReader(list(frames)), crop, search)
            while reader.next_frame_number <= len(frames):
                t0 = time.perf_counter()
                reader.get_n_frames(21)
                per_window.append(time.perf_counter() - t0)
    finally:
        del ctx.stabilize
    plain_reader = ArrayReader(list(frames))
    t0 = time.perf_counter()
    plain_windows = 0
    while plain_reader.next_frame_number <= len(frames):
        plain_reader.get_n_frames(21)
        plain_windows += 1
    plain_read_ms = (time.perf_counter() - t0) / plain_windows * 1e3
    med = {k: float(np.median(v)) for k, v in times.items()}
    windows = -(-(frames_n + 1) // 21)
    extra = {}
    if subpel:
        extra = {"subpel_fps": round(frames_n / med["subpel"], 1), "subpel_s": [round(t, 4) for t in times["subpel"]],
                 "subpel_over_plain": round(med["subpel"] / med["plain"], 4), "subpel_over_stabilized": round(med["subpel"] / med["stabilized"], 4),
                 "subpel_extra_ms_per_window": round((med["subpel"] - med["plain"]) / windows * 1e3, 4)}
    return [{"bench": "stabilize_loop", "frames": frames_n, "windows_per_call": wpc, "crop": [424, 212], "search": search, "events": len(want[1]),
             "plain_fps": round(frames_n / med["plain"], 1), "stabilized_fps": round(frames_n / med["stabilized"], 1),
             "plain_s": [round(t, 4) for t in times["plain"]], "stabilized_s": [round(t, 4) for t in times["stabilized"]],
             "stabilized_over_plain": round(med["stabilized"] / med["plain"], 4),
             "extra_ms_per_window": round((med["stabilized"] - med["plain"]) / windows * 1e3, 4),
             "reader_get_n_frames_ms_per_window": round(float(np.median(per_window)) * 1e3, 4),
             "of_which_library_call_ms": round(float(np.median(spent)) * 1e3, 4),
             "plain_reader_get_n_frames_ms_per_window": round(plain_read_ms, 4), **extra}]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--frames", type=int, default=210)
    ap.add_argument("--windows-per-call", type=int, default=2)
    ap.add_argument("--subpel", action="store_true", help="also time swk_stabilize_subpel_u8 and the loop with stabilize_subpel=True")
    a = ap.parse_args()
    ctx = _lib.default_context(0)
    for row in call_rows(ctx, a.reps, a.repeats, a.subpel):
        print(json.dumps(row), flush=True)
    for wpc in sorted({1, a.windows_per_call}):
        for row in loop_rows(a.frames, a.rounds, wpc, subpel=a.subpel):
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
