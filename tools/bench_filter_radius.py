"""The fused filter kernel at one bilateral radius beside the unfused stage chain on the same sparse planes.

    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_filter_radius.py --radius 2 --n 21

One swk_batch_run of `--windows` windows of 424 x 212 (two synthetic windows, repeated) at bil_d = 2 * radius + 1 runs
k_filter_fused<false, radius> over every frame; swk_bilateral_u8, swk_thresh_tozero_u8 and swk_grey_open3x3_u8 then run k_bilateral,
k_thresh and k_open3x3 over the same frames' sparse images (the route a caller had for another diameter before the batch call took it).
The kernel times are read from the trace's statistics; the script itself only checks that both routes give the same opened image."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--radius", type=int, required=True, choices=[1, 2, 3, 4])
    ap.add_argument("--n", type=int, default=21)
    ap.add_argument("--windows", type=int, default=128)
    ap.add_argument("--size", default="212x424")
    ap.add_argument("--repeat", type=int, default=3)
    args = ap.parse_args()
    from swiftwatcher_amd import _lib, synthetic
    H, W = (int(v) for v in args.size.split("x"))
    d = 2 * args.radius + 1
    two = np.concatenate([synthetic.roi_window(77 + w, args.n, H, W) for w in range(2)])
    frames = np.ascontiguousarray(np.concatenate([two] * ((args.windows + 1) // 2))[:args.windows * args.n])
    ctx = _lib.Context(0)
    params = _lib.default_params(bil_d=d)
    for _ in range(args.repeat):
        res = ctx.batch_run(frames, args.windows, args.n, params=params, stages=("rpca", "opened"))
    for _ in range(args.repeat):
        blur = ctx.bilateral_u8(res["rpca"], d=d)
        thr = ctx.thresh_tozero_u8(blur, 15)
        opened = ctx.grey_open3x3_u8(thr)
    assert np.array_equal(opened, res["opened"]), "the two routes differ"
    print("radius %d (d = %d), %d windows x %d frames of %d x %d: %d launches of each kernel; nonzero sparse pixels %.2f %%"
          % (args.radius, d, args.windows, args.n, W, H, args.repeat, 100.0 * np.count_nonzero(res["rpca"]) / res["rpca"].size))
    ctx.close()


if __name__ == "__main__":
    main()
