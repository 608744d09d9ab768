"""Device time of the YUV -> BGR conversion kernels (csrc/yuv.hip) at the headline's batch: 128 windows x 64 frames of the 424 x 212
ROI plus its margin (448 x 236), planes and result in device memory, timed with the library's HIP events on the context's stream.
First k_yuv420_to_bgr (I420 and NV12, whole frame and origin (1, 1)), as before; then, on identical planes and alternating round by
round, k_yuv420_to_bgr beside k_yuv_to_bgr's 8-bit 4:2:0 instantiation; then every other format of swk_yuv_to_bgr.  Reports ms per
call and achieved bytes/s (the samples read plus 3 B written per pixel) against the MI355X's 8 TB/s HBM peak; for the side-by-side
pairs also the smallest and largest round.
    python tools/bench_yuv.py [--windows 128] [--n 64] [--reps 20] [--rounds 5] [--step-ms <measured step time of the batch, for the share>]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from swiftwatcher_amd import _lib          # noqa: E402

PEAK = 8.0e12

# name -> (sx, sy, bits, semiplanar, msb_aligned, full_range); sx None = mono
FORMATS = {
    "yuvj420p": (1, 1, 8, False, False, True),
    "yuv422p": (1, 0, 8, False, False, False),
    "nv16": (1, 0, 8, True, False, False),
    "yuv444p": (0, 0, 8, False, False, False),
    "nv24": (0, 0, 8, True, False, False),
    "yuv411p": (2, 0, 8, False, False, False),
    "gray": (None, None, 8, False, False, False),
    "yuv420p10": (1, 1, 10, False, False, False),
    "p010": (1, 1, 10, True, True, False),
    "yuv422p10": (1, 0, 10, False, False, True),
    "p210": (1, 0, 10, True, True, False),
    "yuv444p16": (0, 0, 16, False, False, False),
    "gray16": (None, None, 16, False, False, False),
}


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=128)
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--step-ms", type=float, default=0.0)
    a = ap.parse_args()
    ctx = _lib.default_context(0)
    F, H, W = a.windows * a.n, 236, 448
    g = torch.Generator(device="cuda:0")
    g.manual_seed(1)

    def rand(shape, bits=8):
        """random samples; 16-bit words hold random bits in every position (the kernel takes samples as stored)"""
        if bits == 8:
            return torch.randint(0, 256, shape, dtype=torch.uint8, device="cuda:0", generator=g)
        return torch.randint(0, 256, shape[:-1] + (2 * shape[-1],), dtype=torch.uint8, device="cuda:0", generator=g).view(torch.uint16)

    def timed(call, reps):
        ctx.prof_enable(True)
        ctx.prof_reset()
        for _ in range(reps):
            bgr = call()
        ms, launches = ctx.prof()["gray"]
        ctx.prof_enable(False)
        del bgr
        return ms / reps, launches // reps

    def row(per, launches, moved):
        r = {"ms": round(per, 4), "launches_per_call": launches, "GBps": round(moved / per / 1e6, 1), "of_peak": round(moved / (per * 1e-3) / PEAK, 3)}
        if a.step_ms > 0:
            r["share_of_step"] = round(per / a.step_ms, 5)
        return r

    out = {}
    pairs = {}
    for layout in ("i420", "nv12"):
        for name, (fh, fw, rect) in {"whole": (H, W, (0, 0, W, H)), "odd_origin": (H + 1, W + 1, (1, 1, W, H))}.items():
            ch, cw = (fh + 1) // 2, (fw + 1) // 2
            y = rand((F, fh, fw))
            if layout == "i420":
                u, v = rand((F, ch, cw)), rand((F, ch, cw))
            else:
                u, v = rand((F, ch, cw, 2)), None
            torch.cuda.synchronize()
            old = lambda: ctx.yuv420_to_bgr(y, u, v, rect=rect, device_out=True)          # noqa: E731
            new = lambda: ctx.yuv_to_bgr(y, u, v, rect=rect, device_out=True)             # noqa: E731
            assert torch.equal(old(), new())                                               # warm-up, and the same bytes
            moved = F * H * W * 4.5
            per, launches = timed(old, a.reps)
            out["%s_%s" % (layout, name)] = row(per, launches, moved)
            # the two kernels on these planes, alternating: the spread of the old kernel's rounds is the yardstick for the new one's
            rounds = {"k_yuv420_to_bgr": [], "k_yuv_to_bgr": []}
            for _ in range(a.rounds):
                rounds["k_yuv420_to_bgr"].append(timed(old, a.reps)[0])
                rounds["k_yuv_to_bgr"].append(timed(new, a.reps)[0])
            pairs["%s_%s" % (layout, name)] = {k: {"ms_rounds": [round(x, 4) for x in r], "ms_min": round(min(r), 4), "ms_median": round(sorted(r)[len(r) // 2], 4),
                                                   "ms_max": round(max(r), 4), "GBps_median": round(moved / sorted(r)[len(r) // 2] / 1e6, 1)}
                                               for k, r in rounds.items()}
            del y, u, v
    out["side_by_side_8bit_420"] = pairs
    formats = {}
    for name, (sx, sy, bits, semi, msb, full) in FORMATS.items():
        B = 2 if bits > 8 else 1
        y = rand((F, H, W), bits)
        u = v = None
        read = B
        if sx is not None:
            ch, cw = ((H - 1) >> sy) + 1, ((W - 1) >> sx) + 1
            read += 2 * B * ch * cw / (H * W)
            if semi:
                u = rand((F, ch, 2 * cw), bits)
            else:
                u, v = rand((F, ch, cw), bits), rand((F, ch, cw), bits)
        torch.cuda.synchronize()
        call = lambda: ctx.yuv_to_bgr(y, u, v, subsampling=(sx or 0, sy or 0), bits=bits, msb_aligned=msb, full_range=full, device_out=True)          # noqa: E731
        call()                                                                                 # warm-up
        per, launches = timed(call, a.reps)
        formats[name] = dict(row(per, launches, F * H * W * (read + 3.0)), bytes_per_pixel=round(read + 3.0, 3))
        del y, u, v
    out["formats"] = formats
    out["batch"] = {"windows": a.windows, "n": a.n, "rect": [H, W], "bytes_per_call": int(F * H * W * 4.5), "reps": a.reps, "rounds": a.rounds}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
