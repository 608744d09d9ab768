"""Device time of swk_yuv_deinterlace (csrc/deinterlace.hip) and what deinterlace="bob" costs the counting loop.

1. The call alone, 8-bit 4:2:0 planes and both results' BGR in device memory, timed with the library's HIP events on the context's
   stream: a 1080i picture with config 3's 424 x 212 ROI plus its margin (448 x 236) and a 4K one with the 850 x 425 ROI plus its
   margin (874 x 449), 21 and 168 stored frames, both fields of every frame.  Beside it, alternating round by round on the same
   planes, swk_yuv_to_bgr over the same rectangle: the existing kernel it is most like.  Reports ms per call and per stored frame
   (median, smallest and largest round) and achieved bytes/s from the algorithm's own byte count (bytes_per_frame below).
2. The counting loop (pipeline.count_swifts, host clock around the whole count, which ends in a device synchronise) over an
   interlaced 1080i clip with deinterlace="bob", beside the same pictures handed over already progressive at twice the rate:
   pictures per second, median and spread of the rounds.
    python tools/bench_deinterlace.py [--reps 20] [--rounds 5] [--clip-frames 63] [--skip-loop]"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK = 8.0e12

# name -> (frame H, W, rectangle (x0, y0, Wr, Hr)): the ROI plus half the minimum segment size on every side
RECTS = {
    "1080i_roi_424x212": (1080, 1920, (736, 422, 448, 236)),
    "4k_roi_850x425": (2160, 3840, (1483, 855, 874, 449)),
}


def bytes_per_frame(Wr, Hr, rate=2):
    """What the algorithm has to move per stored 8-bit 4:2:0 frame of a Wr x Hr rectangle, whatever the kernels do: the frame's
    samples once (1.5 B a pixel; its neighbours in time are frames of the same call), and per picture the sample planes written
    and read again by the conversion (2 x 1.5 B) and the BGR result (3 B)."""
    return Wr * Hr * (1.5 + rate * (1.5 + 1.5 + 3.0))


def yuv_bytes_per_frame(Wr, Hr):
    return Wr * Hr * 4.5


def stats(rounds, frames, moved):
    r = sorted(rounds)
    med = r[len(r) // 2]
    return {"ms_rounds": [round(x, 4) for x in rounds], "ms_median": round(med, 4), "ms_min": round(r[0], 4), "ms_max": round(r[-1], 4),
            "us_per_stored_frame": round(med * 1e3 / frames, 3), "GBps_median": round(moved / med / 1e6, 1),
            "of_hbm_peak": round(moved / (med * 1e-3) / PEAK, 4)}


def bench_call(ctx, torch, a):
    g = torch.Generator(device="cuda:0")
    g.manual_seed(7)
    out = {}

    def timed(call, reps):
        ctx.prof_enable(True)
        ctx.prof_reset()
        for _ in range(reps):
            res = call()
        ms, _ = ctx.prof()["gray"]
        ctx.prof_enable(False)
        del res
        return ms / reps

    for name, (H, W, rect) in RECTS.items():
        for F in (21, 168):
            y = torch.randint(0, 256, (F, H, W), dtype=torch.uint8, device="cuda:0", generator=g)
            u = torch.randint(0, 256, (F, H // 2, W // 2), dtype=torch.uint8, device="cuda:0", generator=g)
            v = torch.randint(0, 256, (F, H // 2, W // 2), dtype=torch.uint8, device="cuda:0", generator=g)
            torch.cuda.synchronize()
            deint = lambda: ctx.yuv_deinterlace((y, u, v), rect, True, device_out=True)          # noqa: E731
            plain = lambda: ctx.yuv_to_bgr(y, u, v, rect=rect, device_out=True)                  # noqa: E731
            deint(); plain()                                                                     # warm-up
            rounds = {"swk_yuv_deinterlace": [], "swk_yuv_to_bgr": []}
            for _ in range(a.rounds):
                rounds["swk_yuv_deinterlace"].append(timed(deint, a.reps))
                rounds["swk_yuv_to_bgr"].append(timed(plain, a.reps))
            x0, y0, Wr, Hr = rect
            out["%s_%d_frames" % (name, F)] = {
                "swk_yuv_deinterlace": dict(stats(rounds["swk_yuv_deinterlace"], F, F * bytes_per_frame(Wr, Hr)),
                                            bytes_per_stored_frame=int(bytes_per_frame(Wr, Hr))),
                "swk_yuv_to_bgr": dict(stats(rounds["swk_yuv_to_bgr"], F, F * yuv_bytes_per_frame(Wr, Hr)),
                                       bytes_per_stored_frame=int(yuv_bytes_per_frame(Wr, Hr)))}
            del y, u, v
    return out


def bench_loop(ctx, torch, a):
    import numpy as np
    from swiftwatcher_amd import pipeline, synthetic
    from swiftwatcher_amd.io_y4m import Y4MWriter
    N = a.clip_frames
    crop_region = [(748, 434), (748 + 424, 434 + 212)]
    roi_mask = np.zeros((212, 424), np.uint8)
    roi_mask[106:, 42:382] = 255
    shown = synthetic.full_frames(3, 2 * N, crop_region, **{k: synthetic.P2[k] for k in ("bird_len", "bird_wid", "birds")})[::-1]
    planes = [np.concatenate(p) for p in zip(*(ctx.bgr_to_yuv420(np.ascontiguousarray(shown[k:k + 16])) for k in range(0, 2 * N, 16)))]
    del shown
    woven = []
    for p in planes:
        w = p[0::2].copy()
        w[:, 1::2] = p[1::2][:, 1::2]
        woven.append(w)
    out = {}
    with tempfile.TemporaryDirectory() as d:
        paths = {}
        for name, pl, order, fps in (("interlaced_bob", woven, "t", 30), ("progressive_twin", planes, "p", 60)):
            paths[name] = os.path.join(d, name + ".y4m")
            with Y4MWriter(paths[name], 1920, 1080, fps, interlaced=order) as w:
                for k in range(len(pl[0])):
                    w.append(pl[0][k], pl[1][k], pl[2][k])
        kws = {"interlaced_bob": dict(deinterlace="bob"), "progressive_twin": {}}
        rounds = {k: [] for k in paths}
        counts = {}
        for r in range(a.rounds + 1):                  # (the first round warms up: page cache, code objects, staging buffers)
            for name, path in paths.items():
                t0 = time.perf_counter()
                count, events = pipeline.count_swifts(path, crop_region, roi_mask, **kws[name])
                torch.cuda.synchronize()
                if r:
                    rounds[name].append(time.perf_counter() - t0)
                counts[name] = (int(count), len(events))
        for name, secs in rounds.items():
            s = sorted(secs)
            out[name] = {"pictures": 2 * N, "count_events": counts[name], "s_rounds": [round(x, 4) for x in secs],
                         "pictures_per_s_median": round(2 * N / s[len(s) // 2], 1), "pictures_per_s_min": round(2 * N / s[-1], 1),
                         "pictures_per_s_max": round(2 * N / s[0], 1)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--clip-frames", type=int, default=63, help="stored frames of the counting loop's clip")
    ap.add_argument("--skip-loop", action="store_true")
    a = ap.parse_args()
    import torch
    from swiftwatcher_amd import _lib
    ctx = _lib.default_context(0)
    out = {"call": bench_call(ctx, torch, a)}
    if not a.skip_loop:
        out["loop"] = bench_loop(ctx, torch, a)
    out["settings"] = {"reps": a.reps, "rounds": a.rounds, "clip_frames": a.clip_frames}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
