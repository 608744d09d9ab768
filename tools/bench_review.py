"""The review video's cost (csrc/review.hip, swiftwatcher_amd/review.py).
1. The kernel alone: swk_bgr_to_yuv420 and swk_render_review (about 12 boxes per frame, a mark per frame, the mask, a border on every
   fifth frame) on device BGR frames with a device destination, at 424 x 212 x 64 frames and 850 x 425 x 21 frames, timed with the
   library's HIP events on the context's stream.  Reports ms per call and achieved bytes/s against the 4.5 B per pixel it must move
   (3 read, 1.5 written) and the MI355X's 8 TB/s HBM peak.
2. The counting loop: pipeline.count_swifts over a seeded synthetic clip (crop region 424 x 212) with and without review=, alternating
   round by round, the review written to --out (a file on the local disk).  Reports frames/s of each, their ratio, and what the
   review's frames weigh, so the loop's extra time can be set against the device-to-host copy plus the file write.
--text adds the review's text (swk_render_review_labels): a kernel row "render_text" -- the same overlay plus a status line (two labels)
and two event numbers on every frame, at the writer's default scale for the size -- and, in the loop, a review with review_text=True
beside the one without, in the same alternation.
--stages LIST (e.g. rpca,thresh,opened,labels) adds the stage panels (swk_render_review_panels): a row "review_panels" -- at 424 x 212 x 21
frames the mosaic of the same overlay and one panel per stage (device planes, the writer's gains, layers and captions) beside swk_render_review
on the same frames, alternating, five repeats of --reps calls each: ms per call (median, min, max) and the time per output luma pixel of
both, whose ratio says whether a stage cell (2.5 B per pixel) costs no more than a composed one (4.5 B) --, and, in the loop, a review with
review_stages=LIST in the same alternation.
    python tools/bench_review.py [--text] [--stages LIST] [--reps 50] [--rounds 5] [--frames 210] [--windows-per-call 2] [--out /tmp/review_bench.y4m]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from swiftwatcher_amd import _lib          # noqa: E402

PEAK = 8.0e12
STYLES = [(0, 255, 0, 32, 256), (0, 0, 255, 0, 160), (0, 255, 255, 0, 256), (255, 128, 0, 40, 0)]
TEXT_STYLES = STYLES + [(255, 255, 255, 0, 256), (0, 0, 0, 160, 0)]


def text_labels(F, Hc, Wc, rng):
    """Per frame what ReviewWriter(text=True) draws on an event frame: the status line (33 bytes: two labels) and two event numbers."""
    from swiftwatcher_amd.review import ReviewWriter, status_text, text_scale_for
    s, B = text_scale_for(Wc, Hc, ReviewWriter.BORDER), ReviewWriter.BORDER
    labels = []
    for f in range(F):
        line = status_text(f, "00:00:%02d.%03d" % (f // 30, f % 30 * 33), 12, 1, f // 5)
        labels += [(f, Hc - B - 8 * s, B + s + 6 * s * at, 5, 6, s, line[at:at + 32]) for at in range(0, len(line), 32)]
        labels += [(f, int(rng.integers(B + s, Hc - B - 8 * s)), int(rng.integers(B + s, Wc - B - 18 * s)), 3, 6, s, "#%d" % (f + k)) for k in (1, 2)]
    return labels


def kernel_rows(ctx, reps, text=False):
    import torch
    g = torch.Generator(device="cuda:0")
    g.manual_seed(1)
    rng = np.random.default_rng(2)
    out = []
    for Wc, Hc, F in ((424, 212, 64), (850, 425, 21)):
        frames = torch.randint(0, 256, (F, Hc, Wc, 3), dtype=torch.uint8, device="cuda:0", generator=g)
        r0, c0 = rng.integers(0, Hc - 40, (F, 12)), rng.integers(0, Wc - 60, (F, 12))
        boxes = [(f, int(r0[f, k]), int(c0[f, k]), int(r0[f, k] + rng.integers(8, 40)), int(c0[f, k] + rng.integers(8, 60)), 1 + k % 2)
                 for f in range(F) for k in range(12)]
        marks = [(f, Hc // 2, Wc // 2, 3) for f in range(F)]
        frame_style = np.array([3 if f % 5 == 0 else 0 for f in range(F)], np.int32)
        mask = np.zeros((Hc, Wc), np.uint8)
        mask[int(Hc * 0.8):, Wc // 10:Wc * 9 // 10] = 255
        calls = {"convert": lambda: ctx.bgr_to_yuv420(frames, device_out=True),
                 "render": lambda: ctx.render_review(frames, boxes=boxes, marks=marks, frame_style=frame_style, mask=mask, styles=STYLES,
                                                     mask_style=4, mark_arm=4, border=3, device_out=True)}
        if text:
            labels = _lib.label_records(text_labels(F, Hc, Wc, rng))
            calls["render_text"] = lambda: ctx.render_review(frames, boxes=boxes, marks=marks, frame_style=frame_style, mask=mask, styles=TEXT_STYLES,
                                                             mask_style=4, mark_arm=4, border=3, device_out=True, labels=labels)
        moved = F * Hc * Wc * 4.5
        for name, call in calls.items():
            for _ in range(3):
                call()
            ctx.prof_enable(True)
            ctx.prof_reset()
            for _ in range(reps):
                call()
            ms, launches = ctx.prof()["gray"]
            ctx.prof_enable(False)
            per = ms / reps
            out.append({"bench": "review_kernel", "call": name, "Wc": Wc, "Hc": Hc, "frames": F, "ms": round(per, 5), "launches_per_call": launches // reps,
                        "GBps": round(moved / per / 1e6, 1), "of_hbm_peak": round(moved / (per * 1e-3) / PEAK, 4), "bytes_moved": int(moved)})
    return out


def panel_rows(ctx, reps, stages, repeats=5):
    """swk_render_review_panels beside swk_render_review (k_review<true, false>) on the same 21 frames of 424 x 212, in the same run."""
    import torch
    from swiftwatcher_amd.review import DEFAULT_STAGE_GAIN, ReviewWriter, default_stage_cols, stage_caption, text_scale_for
    Wc, Hc, F = 424, 212, 21
    g = torch.Generator(device="cuda:0")
    g.manual_seed(3)
    rng = np.random.default_rng(4)
    frames = torch.randint(0, 256, (F, Hc, Wc, 3), dtype=torch.uint8, device="cuda:0", generator=g)
    r0, c0 = rng.integers(0, Hc - 40, (F, 12)), rng.integers(0, Wc - 60, (F, 12))
    boxes = [(f, int(r0[f, k]), int(c0[f, k]), int(r0[f, k] + rng.integers(8, 40)), int(c0[f, k] + rng.integers(8, 60)), 1 + k % 2)
             for f in range(F) for k in range(12)]
    marks = [(f, Hc // 2, Wc // 2, 3) for f in range(F)]
    frame_style = np.array([3 if f % 5 == 0 else 0 for f in range(F)], np.int32)
    mask = np.zeros((Hc, Wc), np.uint8)
    mask[int(Hc * 0.8):, Wc // 10:Wc * 9 // 10] = 255
    s = text_scale_for(Wc, Hc, ReviewWriter.BORDER)
    at = ReviewWriter.BORDER + s
    panels = []
    for key in stages:
        plane = torch.randint(0, 13 if key == "labels" else 256, (F, Hc, Wc), dtype=torch.uint8, device="cuda:0", generator=g)
        panels.append(dict(plane=plane, kind="labels" if key == "labels" else "gray", gain=DEFAULT_STAGE_GAIN[key], layers=14,
                           caption=(at, at, 5, 6, s, stage_caption(key, DEFAULT_STAGE_GAIN[key]))))
    cols = default_stage_cols(Hc, Wc, 1 + len(panels))
    height, width, _ = _lib.panel_layout(Hc, Wc, 1 + len(panels), cols)
    kw = dict(boxes=boxes, marks=marks, frame_style=frame_style, mask=mask, styles=TEXT_STYLES, mask_style=4, mark_arm=4, border=3, device_out=True)
    calls = {"render": lambda: ctx.render_review(frames, **kw), "panels": lambda: ctx.render_review_panels(frames, panels=panels, cols=cols, **kw)}
    ms = {name: [] for name in calls}
    launches = {}
    for call in calls.values():
        for _ in range(3):
            call()
    for _ in range(repeats):
        for name, call in calls.items():
            ctx.prof_enable(True)
            ctx.prof_reset()
            for _ in range(reps):
                call()
            total, count = ctx.prof()["gray"]
            ctx.prof_enable(False)
            ms[name].append(total / reps)
            launches[name] = count // reps
    pixels = {"render": F * Hc * Wc, "panels": F * height * width}
    row = {"bench": "review_panels", "Wc": Wc, "Hc": Hc, "frames": F, "stages": list(stages), "cols": cols, "mosaic": [width, height], "reps": reps,
           "repeats": repeats}
    for name in calls:
        med = float(np.median(ms[name]))
        row.update({name + "_ms": round(med, 5), name + "_ms_min_max": [round(min(ms[name]), 5), round(max(ms[name]), 5)],
                    name + "_timed_sections_per_call": launches[name], name + "_ns_per_luma_pixel": round(med * 1e6 / pixels[name], 5)})
    row["panels_over_render_per_pixel"] = round(row["panels_ns_per_luma_pixel"] / row["render_ns_per_luma_pixel"], 4)
    row["bytes_moved"] = {"render": int(pixels["render"] * 4.5), "panels": int(F * Hc * Wc * (4.5 + 2.5 * len(panels)))}
    return [row]


def loop_rows(frames_n, rounds, wpc, path, text=False, stages=()):
    from swiftwatcher_amd import pipeline, synthetic
    crop = [(28, 29), (28 + 424, 29 + 212)]
    frames = synthetic.full_frames(500, frames_n, crop, frame_hw=(270, 480))[::-1].copy()
    roi_mask = np.zeros((212, 424), np.uint8)
    roi_mask[int(212 * 0.8):, :] = 255
    kw = dict(crop_region=crop, roi_mask=roi_mask, windows_per_call=wpc)
    want = pipeline.count_swifts(frames, **kw)                                   # warm-up, and the count both variants must give
    pipeline.count_swifts(frames, review=path, **kw)
    names = ("plain", "review") + (("text",) if text else ()) + (("stages",) if stages else ())
    if text:
        pipeline.count_swifts(frames, review=path, review_text=True, **kw)
    if stages:
        pipeline.count_swifts(frames, review=path, review_stages=stages, **kw)
    times = {name: [] for name in names}
    sizes = {}
    for _ in range(rounds):
        for name in names:
            t0 = time.perf_counter()
            got = pipeline.count_swifts(frames, review=None if name == "plain" else path, review_text=name == "text",
                                        review_stages=stages if name == "stages" else (), **kw)
            times[name].append(time.perf_counter() - t0)
            assert got[0] == want[0] and len(got[1]) == len(want[1])
            sizes[name] = os.path.getsize(path) if name != "plain" else 0
    size = sizes["review"]
    med = {k: float(np.median(v)) for k, v in times.items()}
    more = {}
    if text:
        more = {"text_fps": round(frames_n / med["text"], 1), "text_s": [round(t, 4) for t in times["text"]],
                "text_over_review": round(med["text"] / med["review"], 4), "text_extra_ms_per_frame": round((med["text"] - med["review"]) / frames_n * 1e3, 4)}
    if stages:
        more.update({"stages": list(stages), "stages_fps": round(frames_n / med["stages"], 1), "stages_s": [round(t, 4) for t in times["stages"]],
                     "stages_over_review": round(med["stages"] / med["review"], 4), "stages_over_plain": round(med["stages"] / med["plain"], 4),
                     "stages_extra_ms_per_frame": round((med["stages"] - med["review"]) / frames_n * 1e3, 4), "stages_file_bytes": sizes["stages"]})
    return [{**more, "bench": "review_loop", "frames": frames_n, "windows_per_call": wpc, "crop": [424, 212], "events": len(want[1]),
             "plain_fps": round(frames_n / med["plain"], 1), "review_fps": round(frames_n / med["review"], 1),
             "plain_s": [round(t, 4) for t in times["plain"]], "review_s": [round(t, 4) for t in times["review"]],
             "review_over_plain": round(med["review"] / med["plain"], 4), "review_extra_ms_per_frame": round((med["review"] - med["plain"]) / frames_n * 1e3, 4),
             "review_file_bytes": size, "review_bytes_per_frame": size // max(frames_n, 1)}]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--text", action="store_true", help="also measure the review with text (labels)")
    ap.add_argument("--stages", default="", metavar="LIST", help="also measure the stage panels, e.g. rpca,thresh,opened,labels")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--frames", type=int, default=210)
    ap.add_argument("--windows-per-call", type=int, default=2)
    ap.add_argument("--out", default=os.path.join("/tmp", "review_bench.y4m"))
    a = ap.parse_args()
    from swiftwatcher_amd.review import stage_keys
    stages = stage_keys(a.stages)
    ctx = _lib.default_context(0)
    for row in kernel_rows(ctx, a.reps, a.text):
        print(json.dumps(row), flush=True)
    if stages:
        for row in panel_rows(ctx, a.reps, stages):
            print(json.dumps(row), flush=True)
    for wpc in sorted({1, a.windows_per_call}):
        for row in loop_rows(a.frames, a.rounds, wpc, a.out, a.text, stages):
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
