"""A YUV4MPEG2 video from a pipe (io_y4m.Y4MStreamReader) beside the same clip read from a file (open_y4m(path): a memory map).
The clip is a generated 1080p 8-bit 4:2:0 video (flat sky, synthetic.roi_window inside the 424 x 212 crop region of SURVEY 8d's
340-px chimney): --frames frames of 3.11 MB, written once to --dir.  The pipe is fed by a child process that writes the file to its
standard output.  Every figure is the median and the smallest-largest of --plays plays of the whole clip, after one warm-up play.

  reader  (no GPU)  windows of 21 frames until `frames_processed < total_frames` turns false; each window's crop region plus margin is
                    copied out of its frames (the host work stack_frames does), so that the memory map reads its pages.  For the
                    pipe also the share of the wall clock spent in the source's read calls.
  loop    (MI355X)  pipeline.count_swifts over the path and over the pipe, --windows-per-call windows per GPU call: a host clock
                    around the whole call, which ends with the tracker having seen every frame (every GPU call is waited for).
                    Counts and event counts must be equal.

    python tools/bench_y4m_stream.py [--what reader,loop] [--frames 105] [--plays 5] [--windows-per-call 1] [--dir DIR]"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CROP = [(748, 452), (1172, 664)]
FRAME_HW = (1080, 1920)
N = 21
WRITER = "import shutil, sys\nwith open(sys.argv[1], 'rb') as fh:\n    shutil.copyfileobj(fh, sys.stdout.buffer, 1 << 20)\n"


def make_clip(path, frames, seed=20190816):
    """BT.601 limited-range planes of a BGR clip whose crop region holds synthetic.roi_window; 4:2:0 by averaging each 2 x 2 cell."""
    from swiftwatcher_amd import synthetic
    from swiftwatcher_amd.io_y4m import Y4MWriter
    (x0, y0), (x1, y1) = CROP
    H, W = FRAME_HW
    roi = synthetic.roi_window(seed, frames, y1 - y0, x1 - x0, **{k: synthetic.P2[k] for k in ("birds", "bird_len", "bird_wid")})[::-1].astype(np.float64)
    b, g, r = roi[..., 0], roi[..., 1], roi[..., 2]
    yy = 16.0 + (65.481 * r + 128.553 * g + 24.966 * b) / 255.0
    uu = 128.0 + (-37.797 * r - 74.203 * g + 112.0 * b) / 255.0
    vv = 128.0 + (112.0 * r - 93.786 * g - 18.214 * b) / 255.0
    half = lambda p: p.reshape(frames, (y1 - y0) // 2, 2, (x1 - x0) // 2, 2).mean((2, 4))      # noqa: E731  (the crop region is even)
    q = lambda p: np.clip(np.rint(p), 0, 255).astype(np.uint8)                                   # noqa: E731
    yr, ur, vr = q(yy), q(half(uu)), q(half(vv))
    y = np.full((H, W), 126, np.uint8)                     # BGR (128, 128, 128)
    u = np.full((H // 2, W // 2), 128, np.uint8)
    v = np.full((H // 2, W // 2), 128, np.uint8)
    with Y4MWriter(path, W, H, 30) as w:
        for k in range(frames):
            y[y0:y1, x0:x1] = yr[k]
            u[y0 // 2:y1 // 2, x0 // 2:x1 // 2] = ur[k]
            v[y0 // 2:y1 // 2, x0 // 2:x1 // 2] = vr[k]
            w.append(y, u, v)
    return path


def spread(values, digits=1):
    s = sorted(values)
    return {"median": round(s[len(s) // 2], digits), "min": round(s[0], digits), "max": round(s[-1], digits), "plays": len(s)}


class Piped:
    """The clip on a pipe: a child process writes the file to its standard output."""

    def __init__(self, path):
        self.proc = subprocess.Popen([sys.executable, "-c", WRITER, path], stdout=subprocess.PIPE, bufsize=0)
        self.source = self.proc.stdout

    def close(self):
        self.source.close()
        self.proc.wait()


def play_reader(reader, rect):
    """The loop's reads, and the copy of every frame's rectangle that staging makes.  Returns the frames read."""
    ya, yb, xa, xb = rect
    luma = np.empty((N, yb - ya, xb - xa), np.uint8)
    chroma = np.empty((2, N, (yb - ya) // 2, (xb - xa) // 2), np.uint8)
    processed = 0
    while processed < reader.total_frames:
        frames, numbers, _ = reader.get_n_frames(N)
        processed += sum(1 for k in numbers if k >= 0)
        for i, f in enumerate(frames):
            oy, ox = getattr(f, "origin", (0, 0))
            luma[i] = f.y[ya - oy:yb - oy, xa - ox:xb - ox]
            chroma[0, i] = f.u[(ya - oy) // 2:(yb - oy) // 2, (xa - ox) // 2:(xb - ox) // 2]
            chroma[1, i] = f.v[(ya - oy) // 2:(yb - oy) // 2, (xa - ox) // 2:(xb - ox) // 2]
    return reader.frames_read


def bench_reader(path, plays):
    from swiftwatcher_amd.io_y4m import held_rect, open_y4m
    rect = held_rect(FRAME_HW, CROP, (24, 24), (1, 1))
    rates = {"file": [], "pipe": []}
    shares = []
    for k in range(plays + 1):                    # play 0 warms the page cache and the interpreter
        for kind in ("file", "pipe"):
            piped = Piped(path) if kind == "pipe" else None
            t0 = time.perf_counter()
            reader = open_y4m(path) if piped is None else open_y4m(piped.source, crop_region=CROP)
            frames = play_reader(reader, rect)
            wall = time.perf_counter() - t0
            if piped is not None:
                share = reader.read_seconds / wall
                reader.close()
                piped.close()
            if k:
                rates[kind].append(frames / wall)
                if piped is not None:
                    shares.append(share)
    return {"file_frames_per_s": spread(rates["file"]), "pipe_frames_per_s": spread(rates["pipe"]),
            "pipe_share_of_wall_in_read": spread(shares, 3), "pipe_MB_per_s": spread([r * 3.1104 for r in rates["pipe"]])}


def bench_loop(path, plays, windows_per_call):
    import torch
    from swiftwatcher_amd import pipeline
    if not torch.cuda.is_available():
        raise SystemExit("the counting loop is measured on the GPU: none found")
    (x0, y0), (x1, y1) = CROP
    roi_mask = np.zeros((y1 - y0, x1 - x0), np.uint8)
    roi_mask[(y1 - y0) // 2:, 40:-40] = 255
    rates = {"file": [], "pipe": []}
    results = {}
    frames = None
    for k in range(plays + 1):                    # play 0 warms up every shape of the loop
        for kind in ("file", "pipe"):
            piped = Piped(path) if kind == "pipe" else None
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            count, events = pipeline.count_swifts(path if piped is None else piped.source, CROP, roi_mask, windows_per_call=windows_per_call)
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
            if piped is not None:
                piped.close()
            if frames is None:
                from swiftwatcher_amd.io_y4m import open_y4m
                frames = open_y4m(path).total_frames
            results.setdefault(kind, (count, len(events)))
            if results[kind] != (count, len(events)) or results["file"] != (count, len(events)):
                raise SystemExit("the %s run counted %r, an earlier run %r" % (kind, (count, len(events)), results["file"]))
            if k:
                rates[kind].append(frames / wall)
    return {"file_frames_per_s": spread(rates["file"]), "pipe_frames_per_s": spread(rates["pipe"]), "count": results["file"][0],
            "events": results["file"][1], "windows_per_call": windows_per_call}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="reader")
    ap.add_argument("--frames", type=int, default=105)
    ap.add_argument("--plays", type=int, default=5)
    ap.add_argument("--windows-per-call", type=int, default=1)
    ap.add_argument("--dir", default=None)
    a = ap.parse_args()
    if a.plays < 5:
        raise SystemExit("at least five plays")
    out = {"clip": {"frames": a.frames, "frame_hw": list(FRAME_HW), "crop_region": [list(CROP[0]), list(CROP[1])], "format": "C420jpeg",
                    "MB_per_frame": 3.1104}}
    with tempfile.TemporaryDirectory(dir=a.dir) as folder:
        path = make_clip(os.path.join(folder, "clip.y4m"), a.frames)
        for what in a.what.split(","):
            if what == "reader":
                out["reader"] = bench_reader(path, a.plays)
            elif what == "loop":
                out["loop"] = bench_loop(path, a.plays, a.windows_per_call)
            else:
                raise SystemExit("--what takes reader and loop")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
