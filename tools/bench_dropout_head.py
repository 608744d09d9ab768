"""The cost of dropout sampling ("The dropout head") beside tools/bench_classifier.py: a forward of `--rows` segments
in eval mode (two chains, the default, and one chain) and under the reference's live Dropout(0.5) at each `--samples` count, and the two
head kernels alone on the last Fire's live output.  Random weights of the right shapes; every figure is the median and the min .. max
of `--runs` timings of `--inner` launches each, between HIP events on torch's stream, after three untimed calls.  Prints one JSON line.

    python tools/bench_dropout_head.py [--rows 4096] [--samples 1 32 256] [--runs 7] [--inner 10]"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import classifier_ref as ref                                  # noqa: E402  (weights generator only)
from swiftwatcher_amd import _lib                                         # noqa: E402
from swiftwatcher_amd.segment_classification import SegmentClassifier    # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--samples", type=int, nargs="+", default=[1, 32, 256])
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--inner", type=int, default=10)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    clf = SegmentClassifier.from_state_dict(ref.random_state_dict(14), batch_size=a.rows)
    rows = a.rows
    x = torch.randn((rows, 3, 40, 40), generator=torch.Generator().manual_seed(1)).to(dev).contiguous(memory_format=torch.channels_last)
    keys = torch.arange(rows, dtype=torch.int64, device=dev) * 256 + 1

    def timed(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.runs):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(a.inner):
                fn()
            t1.record()
            torch.cuda.synchronize()
            ms.append(t0.elapsed_time(t1) / a.inner)
        return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}

    out = {"rows": rows, "runs": a.runs, "inner": a.inner, "forward": {}, "head_alone": {}}
    out["forward"]["eval_default"] = timed(lambda: clf._forward(x))
    split, clf._split_rows = clf._split_rows, 0
    out["forward"]["eval_one_chain"] = timed(lambda: clf._forward(x))
    clf._split_rows = split
    for s in a.samples:
        out["forward"]["dropout_S%d" % s] = timed(lambda: clf._forward_dropout(x, keys, s, 0))
    # the heads alone on the last Fire's live output (the forwards above left it in the persistent tiles)
    lib = _lib.load()
    cr = clf.cropped
    f9 = cr._buf[1][-1][:rows]
    px, c = f9.shape[2] * f9.shape[3], f9.shape[1]
    hw, hb, ring = cr._head_operand()
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    o2 = torch.empty((rows, 2), device=dev)
    out["head_alone"]["eval"] = timed(lambda: lib.swk_nhwc_head2_relu_mean(st, f9.data_ptr(), rows, px, c, hw.data_ptr(), hb.data_ptr(),
                                                                           ring.data_ptr(), cr.n_pos, o2.data_ptr()))
    for s in a.samples:
        o = torch.empty((rows, s, 2), device=dev)
        out["head_alone"]["dropout_S%d" % s] = timed(lambda: lib.swk_nhwc_head2_dropout_relu_mean(
            st, f9.data_ptr(), rows, px, c, cr.head_pos.data_ptr(), cr.head_bg.data_ptr(), int(cr.n_pos), hw.data_ptr(), hb.data_ptr(),
            keys.data_ptr(), ctypes.c_uint64(0), s, o.data_ptr()))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
