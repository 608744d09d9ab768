"""Latency of the drop-in path: FrameQueue.preprocess_queue + segment_queue per window, from host frames,
including staging, H2D/D2H and Python object creation (what the reference's loop would see).
--yuv: the same loop from host 1080p I420 frames (io_y4m.Yuv420Frame: staged as 4:2:0, converted on the GPU) beside the loop from the
BGR frames those restate to, alternating window by window in one run."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from swiftwatcher_amd import synthetic                      # noqa: E402
from swiftwatcher_amd.data_structures import FrameQueue     # noqa: E402
from swiftwatcher_amd import _lib                            # noqa: E402

crop_region = [(748, 452), (1172, 664)]                     # the 424x212 ROI inside 1080p frames
out = {}


def yuv_beside_bgr(reps=9):
    from swiftwatcher_amd.io_y4m import Yuv420Frame
    res = {}
    for n in (21, 64):
        bgr = synthetic.full_frames(3, n, crop_region).astype(np.int32)
        b, g, r = bgr[..., 0], bgr[..., 1], bgr[..., 2]
        y = ((66 * r + 129 * g + 25 * b + 128) >> 8) + 16                      # BT.601 limited range; chroma of each cell's top-left pixel
        u = ((-38 * r - 74 * g + 112 * b + 128) >> 8)[:, ::2, ::2] + 128
        v = ((112 * r - 94 * g - 18 * b + 128) >> 8)[:, ::2, ::2] + 128
        del bgr, b, g, r
        yuv = [Yuv420Frame(*(np.ascontiguousarray(np.clip(p[i], 0, 255).astype(np.uint8)) for p in (y, u, v))) for i in range(n)]
        frames = {"yuv": yuv, "bgr": [np.asarray(f) for f in yuv]}                # the BGR frames the 4:2:0 frames restate to
        queues = {k: FrameQueue(queue_size=n, keep_stages=False) for k in frames}
        times, nseg = {k: [] for k in frames}, {}
        for rep in range(reps):
            for kind in ("bgr", "yuv"):
                q = queues[kind]
                q.push_list_of_frames(frames[kind][::-1], list(range(n)), ["t"] * n)
                t0 = time.perf_counter()
                q.preprocess_queue(crop_region, None)
                q.segment_queue((24, 24), crop_region)
                times[kind].append(time.perf_counter() - t0)
                nseg[kind] = sum(len(f.segments) for f in q)
                while not q.is_empty():
                    q.pop_frame()
        for kind in frames:
            t = np.array(times[kind][2:]) * 1e3
            res["n%d_%s" % (n, kind)] = {"ms_per_window_median": round(float(np.median(t)), 3), "ms_min": round(float(t.min()), 3),
                                        "ms_max": round(float(t.max()), 3), "frames_per_s": round(n / float(np.median(t)) * 1e3, 1),
                                        "segments": nseg[kind], "iters": queues[kind].last_iters}
    print(json.dumps(res))


if "--yuv" in sys.argv:
    yuv_beside_bgr()
    sys.exit(0)
for n, keep in [(21, True), (21, False), (64, True), (64, False)]:
    frames = synthetic.full_frames(3, n, crop_region)        # (n, 1080, 1920, 3)
    q = FrameQueue(queue_size=n, keep_stages=keep)
    times = []
    for rep in range(6):
        q.push_list_of_frames([frames[i] for i in range(n - 1, -1, -1)], list(range(n)), ["t"] * n)
        t0 = time.perf_counter()
        q.preprocess_queue(crop_region, None)
        q.segment_queue((24, 24), crop_region)
        times.append(time.perf_counter() - t0)
        nseg = sum(len(f.segments) for f in q)
        while not q.is_empty():
            q.pop_frame()
    t = float(np.median(times[1:]))
    # where the time goes on the device side: one more window with the library's per-family HIP events on
    ctx = _lib.default_context(0)
    ctx.prof_enable(True)
    ctx.prof_reset()
    q.push_list_of_frames([frames[i] for i in range(n - 1, -1, -1)], list(range(n)), ["t"] * n)
    q.preprocess_queue(crop_region, None)
    q.segment_queue((24, 24), crop_region)
    fam = {k: round(v[0], 3) for k, v in ctx.prof().items() if isinstance(v, tuple) and v[0] > 0}
    ctx.prof_enable(False)
    while not q.is_empty():
        q.pop_frame()
    out["n%d_keep%d" % (n, keep)] = {"ms_per_window": round(t * 1e3, 2), "frames_per_s": round(n / t, 1), "segments": nseg,
                                    "iters": q.last_iters, "device_ms_by_family": fam, "eig_sweeps_last": ctx.last_eig_sweeps}
print(json.dumps(out))
