"""Device time of the 4:2:0 -> BGR conversion kernel (csrc/yuv.hip) at the headline's batch: 128 windows x 64 frames of the 424 x 212
ROI plus its margin (448 x 236), planes and result in device memory, timed with the library's HIP events on the context's stream.
Reports ms per call and achieved bytes/s (1.5 B read + 3 B written per pixel) against the MI355X's 8 TB/s HBM peak.
    python tools/bench_yuv.py [--windows 128] [--n 64] [--reps 20] [--step-ms <measured step time of the batch, for the share>]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from swiftwatcher_amd import _lib          # noqa: E402

PEAK = 8.0e12


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=128)
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--step-ms", type=float, default=0.0)
    a = ap.parse_args()
    ctx = _lib.default_context(0)
    F, H, W = a.windows * a.n, 236, 448
    g = torch.Generator(device="cuda:0")
    g.manual_seed(1)
    out = {}
    for layout in ("i420", "nv12"):
        for name, (fh, fw, rect) in {"whole": (H, W, (0, 0, W, H)), "odd_origin": (H + 1, W + 1, (1, 1, W, H))}.items():
            ch, cw = (fh + 1) // 2, (fw + 1) // 2
            y = torch.randint(0, 256, (F, fh, fw), dtype=torch.uint8, device="cuda:0", generator=g)
            if layout == "i420":
                u = torch.randint(0, 256, (F, ch, cw), dtype=torch.uint8, device="cuda:0", generator=g)
                v = torch.randint(0, 256, (F, ch, cw), dtype=torch.uint8, device="cuda:0", generator=g)
            else:
                u, v = torch.randint(0, 256, (F, ch, cw, 2), dtype=torch.uint8, device="cuda:0", generator=g), None
            torch.cuda.synchronize()
            ctx.yuv420_to_bgr(y, u, v, rect=rect, device_out=True)          # warm-up
            ctx.prof_enable(True)
            ctx.prof_reset()
            for _ in range(a.reps):
                bgr = ctx.yuv420_to_bgr(y, u, v, rect=rect, device_out=True)
            ms, launches = ctx.prof()["gray"]
            ctx.prof_enable(False)
            per = ms / a.reps
            moved = F * H * W * 4.5
            row = {"ms": round(per, 4), "launches_per_call": launches // a.reps, "GBps": round(moved / per / 1e6, 1),
                   "of_peak": round(moved / (per * 1e-3) / PEAK, 3)}
            if a.step_ms > 0:
                row["share_of_step"] = round(per / a.step_ms, 5)
            out["%s_%s" % (layout, name)] = row
            del y, u, v, bgr
    out["batch"] = {"windows": a.windows, "n": a.n, "rect": [H, W], "bytes_per_call": int(F * H * W * 4.5)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
