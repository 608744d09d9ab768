"""Stage panels in the review video, end to end on the MI355X: count_swifts at windows_per_call 1 and 2, count_swifts_videos and the
command line with review_stages= / --review-stages write a mosaic whose cell 0 is the review without stages and whose other cells
are the stage images of the same frame -- checked against tests/review_panels_ref.py applied to the processed_frames of an
independent FrameQueue(keep_stages=True) run over the same windows.  Counts and events do not change, no window is segmented twice,
and a writer fed frames without device planes writes the same bytes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from review_panels_ref import panel_cell, paste

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CROP = [(30, 20), (30 + 96, 20 + 64)]
CROP_ODD = [(31, 21), (31 + 95, 21 + 63)]          # 63 x 95: a pad row and a pad column in every cell
CORNERS = ((40, 71), (116, 71))                    # the top edge of the clip's chimney (tests/test_y4m_stream_gpu.py)
STAGES = ("rpca", "thresh", "labels")
MARK_ARM, BORDER, LAYERS = 4, 3, 14                # ReviewWriter's documented defaults
PALETTE = [(0, 255, 0, 32, 256), (0, 0, 255, 0, 160), (0, 255, 255, 0, 256), (255, 128, 0, 40, 0), (255, 255, 255, 0, 256), (0, 0, 0, 160, 0)]
CAPTIONS = {"rpca": ("gray", 4, "RPCA X4"), "thresh": ("gray", 4, "THRESH X4"), "labels": ("labels", 1, "LABELS")}
NAMES = {"rpca": "RPCA", "thresh": "thresh_15", "labels": "cc_labeling"}


@pytest.fixture(scope="module")
def font():
    from swiftwatcher_amd import _lib
    return _lib.review_font()


@pytest.fixture(scope="module")
def palette():
    from swiftwatcher_amd import _lib
    return _lib.review_label_palette()


def _mask(crop, top):
    (x0, y0), (x1, y1) = crop
    m = np.zeros((y1 - y0, x1 - x0), np.uint8)
    m[top:, :] = 255
    return m


@pytest.fixture(scope="module")
def clip(tmp_path_factory):
    """tests/test_review_gpu.py's seeded 52-frame 110 x 160 clip: BGR frames, and an 8-bit 4:2:0 file of them (and of the first 23)."""
    import yuv_ref
    from swiftwatcher_amd import synthetic
    from swiftwatcher_amd.io_y4m import Y4MWriter
    bgr = synthetic.full_frames(500, 52, CROP, frame_hw=(110, 160), birds=4, bird_len=(8, 12), bird_wid=(3, 5))[::-1].copy()
    folder = tmp_path_factory.mktemp("review_stages_gpu")
    y, u, v = yuv_ref.bgr_to_yuv420(bgr)
    paths = {}
    for name, count in (("y4m", 52), ("y4m_23", 23)):
        paths[name] = str(folder / (name + ".y4m"))
        with Y4MWriter(paths[name], 160, 110, 30) as w:
            for k in range(count):
                w.append(y[k], u[k], v[k])
    return dict(bgr=bgr, folder=folder, **paths)


_REFERENCE = {}


def _stage_reference(source, crop):
    """frame number -> {stage key: (Hc, Wc) uint8} from an independent FrameQueue(keep_stages=True) over the source's windows, computed
    once per (source, crop); and the popped Frame objects per window (they carry the device planes)."""
    from swiftwatcher_amd.data_structures import FrameQueue
    from swiftwatcher_amd.io_frames import ArrayReader
    from swiftwatcher_amd.io_y4m import open_y4m
    key = (source if isinstance(source, str) else id(source), str(crop))
    if key not in _REFERENCE:
        reader = open_y4m(source) if isinstance(source, str) else ArrayReader(source, fps=30)
        images, windows = {}, []
        queue = FrameQueue(21, keep_stages=True)
        while queue.frames_processed < reader.total_frames:
            queue.push_list_of_frames(*reader.get_n_frames(n=21))
            queue.preprocess_queue(crop, None)
            queue.segment_queue((24, 24), crop)
            popped = []
            while not queue.is_empty():
                popped.append(queue.pop_frame())
            windows.append(popped)
            for fr in popped:
                if fr.frame_number >= 0:
                    images[fr.frame_number] = {k: np.array(fr.processed_frames[NAMES[k]]) for k in STAGES}
        _REFERENCE[key] = (images, windows, reader)          # (the reader stays open: the windows' frames are its frames)
    return _REFERENCE[key][:2]


def _event_records(events):
    return [[(s.parent_frame_number, str(s.parent_timestamp), tuple(s.centroid), tuple(s.bbox), np.array(s.segment_image).tobytes()) for s in ev]
            for ev in events]


def _read(path):
    """(y, u, v) stacks of a 4:2:0 .y4m file."""
    from swiftwatcher_amd.io_y4m import open_y4m
    reader = open_y4m(path)
    frames = [reader.frames[k] for k in range(reader.total_frames)]
    got = tuple(np.stack([np.asarray(getattr(f, p)) for f in frames]) for p in "yuv")
    if hasattr(reader, "close"):
        reader.close()
    return got


def _recording_writer(path, crop, roi_mask, **kw):
    """A ReviewWriter that keeps every window's plan (frame numbers, boxes, marks, frame_style) beside writing it."""
    from swiftwatcher_amd.review import ReviewWriter

    class Recording(ReviewWriter):
        plans = []

        def plan_window(self, popped_frames, rejected=None, new_events=()):
            plan = ReviewWriter.plan_window(self, popped_frames, rejected, new_events)
            self.plans.append(([f.frame_number for f in plan[0]], list(plan[1]), list(plan[2]), list(plan[3])))
            return plan
    w = Recording(path, crop, roi_mask, 30, **kw)
    w.plans = []
    return w


def _expected_mosaic(plans, plain, images, crop, roi_mask, font, palette, scale):
    """The mosaic's (y, u, v): cell 0 from the review without stages (plain: its (y, u, v)), every stage cell from the reference
    images under the recorded overlay's layers 2..4 (stage_layers = 14) and the caption."""
    (x0, y0), (x1, y1) = crop
    Hc, Wc = y1 - y0, x1 - x0
    cells = [[] for _ in STAGES]
    for numbers, boxes, marks, frame_style in plans:
        overlay = dict(boxes=boxes, marks=marks, frame_style=frame_style, mask=roi_mask, styles=PALETTE, mask_style=4, mark_arm=MARK_ARM, border=BORDER)
        for k, key in enumerate(STAGES):
            kind, gain, text = CAPTIONS[key]
            plane = np.stack([images[n][key] for n in numbers])
            cells[k].append(panel_cell(plane, kind, gain, LAYERS, (BORDER + scale, BORDER + scale, 5, 6, scale, text), overlay, font, palette))
    stage_cells = [tuple(np.concatenate([w[p] for w in per]) for p in range(3)) for per in cells]
    cols = 1 if Wc > Hc else 1 + len(STAGES)
    return paste([plain] + stage_cells, Hc, Wc, cols)


def _check(run, source, crop, roi_mask, folder, name, font, palette, frames=52, min_events=1):
    """run(review, review_stages) -> (count, events) with no review, a review without stages, a review with stages made from a path
    and a recording writer with stages: equal counts and events; the two staged files are equal; the staged file is the mosaic of the
    plain file and the reference's stage images."""
    paths = {k: str(folder / ("%s_%s.y4m" % (name, k))) for k in ("plain", "staged", "recorded")}
    none = run(None, ())
    plain = run(paths["plain"], ())
    staged = run(paths["staged"], STAGES)
    recorder = _recording_writer(paths["recorded"], crop, roi_mask, stages=STAGES)
    recorded = run(recorder, ())
    recorder.close()
    assert len(none[1]) >= min_events
    for got in (plain, staged, recorded):
        assert got[0] == none[0] and _event_records(got[1]) == _event_records(none[1])
    assert open(paths["staged"], "rb").read() == open(paths["recorded"], "rb").read()
    images, _ = _stage_reference(source, crop)
    got, cell0 = _read(paths["staged"]), _read(paths["plain"])
    (x0, y0), (x1, y1) = crop
    Hc, Wc = y1 - y0, x1 - x0
    # (a reader hands out one frame past the clip's last, the reference's inclusive end: 52 frames are 53 written ones)
    assert cell0[0].shape[0] >= frames
    frames = cell0[0].shape[0]
    assert cell0[0].shape == (frames, Hc, Wc) and sum(len(p[0]) for p in recorder.plans) == frames == len(images)
    want = _expected_mosaic(recorder.plans, cell0, images, crop, roi_mask, font, palette, recorder.text_scale)
    assert got[0].shape == want[0].shape == (frames, recorder.frame_height, recorder.frame_width)
    # cell 0's rectangles are the review without stages ...
    assert np.array_equal(got[0][:, :Hc, :Wc], cell0[0]) and np.array_equal(got[1][:, :(Hc + 1) // 2, :(Wc + 1) // 2], cell0[1])
    assert np.array_equal(got[2][:, :(Hc + 1) // 2, :(Wc + 1) // 2], cell0[2])
    # ... and every plane of the mosaic is the expected one: stage cells, pads, empty cells
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    # the panels show the stages: the labels cell is coloured on some frame, the rpca cell is not the thresh cell
    origins = recorder.cell_origins
    r, c = origins[3]
    assert (got[1][:, r // 2:r // 2 + Hc // 2, c // 2:c // 2 + Wc // 2] != 128).any()
    (r1, c1), (r2, c2) = origins[1], origins[2]
    assert not np.array_equal(got[0][:, r1:r1 + Hc, c1:c1 + Wc], got[0][:, r2:r2 + Hc, c2:c2 + Wc])
    return recorder


class _Spy:
    """Counts the windows that Context.batch_run / batch_run_groups segment while it is installed."""

    def __init__(self, monkeypatch):
        from swiftwatcher_amd import _lib
        self.windows, self.stages = 0, []
        run, groups = _lib.Context.batch_run, _lib.Context.batch_run_groups

        def batch_run(ctx, frames, nwin, n, *a, **kw):
            self.windows += nwin
            self.stages.append(tuple(kw.get("stages", _lib.STAGES)))
            return run(ctx, frames, nwin, n, *a, **kw)

        def batch_run_groups(ctx, specs, *a, **kw):
            self.windows += sum(int(g["nwin"]) for g in specs)
            self.stages.append(tuple(kw.get("stages", _lib.STAGES)))
            return groups(ctx, specs, *a, **kw)
        monkeypatch.setattr(_lib.Context, "batch_run", batch_run)
        monkeypatch.setattr(_lib.Context, "batch_run_groups", batch_run_groups)


@pytest.mark.parametrize("wpc", [1, 2])
def test_staged_review_of_a_y4m_file(clip, font, palette, monkeypatch, wpc):
    from swiftwatcher_amd import pipeline
    roi_mask = _mask(CROP_ODD, 27)
    _stage_reference(clip["y4m"], CROP_ODD)                     # (before the spy counts)
    spy = _Spy(monkeypatch)

    def run(rv, stages):
        return pipeline.count_swifts(clip["y4m"], crop_region=CROP_ODD, roi_mask=roi_mask, windows_per_call=wpc, review=rv, review_stages=stages)
    recorder = _check(run, clip["y4m"], CROP_ODD, roi_mask, clip["folder"], "file_%d" % wpc, font, palette)
    assert (recorder.stage_cols, recorder.frame_height, recorder.frame_width) == (1, 4 * 64, 96)
    # four runs of three windows, none segmented twice; the batched loop produces the stages asked for, and only in the staged runs
    assert spy.windows == 4 * 3
    if wpc == 2:
        assert sorted(set(spy.stages)) == [(), STAGES] and spy.stages.count(STAGES) == 2 * 2


def test_staged_review_through_count_swifts_videos(clip, font, palette, monkeypatch):
    """Two videos of different crop regions in one groups call; the first gets a staged review, the second none."""
    from swiftwatcher_amd import pipeline
    small = [(40, 30), (40 + 64, 30 + 48)]
    regions = [(CROP, _mask(CROP, 28)), (small, _mask(small, 20))]
    _stage_reference(clip["bgr"], CROP)
    spy = _Spy(monkeypatch)
    seen = []

    def run(rv, stages):
        out = pipeline.count_swifts_videos([clip["bgr"], clip["y4m"]], regions=regions, reviews=None if rv is None else [rv, None], review_stages=stages)
        seen.append(out[1])
        return out[0]
    _check(run, clip["bgr"], CROP, regions[0][1], clip["folder"], "videos", font, palette)
    assert all(o[0] == seen[0][0] and _event_records(o[1]) == _event_records(seen[0][1]) for o in seen[1:])          # the other video's count
    assert spy.windows == 4 * 2 * 3 and sorted(set(spy.stages)) == [(), STAGES]


def test_cli_writes_the_staged_review(clip, font, palette):
    """python -m swiftwatcher_amd --review PATH --review-stages rpca,thresh,labels in a fresh child process, on the 23-frame file: the
    same bytes as the in-process count with the same corners, which is checked against the restatement."""
    from swiftwatcher_amd import image_filtering as img
    from swiftwatcher_amd import pipeline
    from swiftwatcher_amd.io_y4m import open_y4m
    first = open_y4m(clip["y4m_23"])
    crop, roi_mask, _ = img.generate_regions(first.read_frame(0, increment=False), CORNERS)
    first.close() if hasattr(first, "close") else None
    crop = [tuple(int(v) for v in crop[0]), tuple(int(v) for v in crop[1])]
    _check(lambda rv, stages: pipeline.count_swifts(clip["y4m_23"], corners=CORNERS, review=rv, review_stages=stages), clip["y4m_23"], crop, roi_mask,
           clip["folder"], "inproc", font, palette, frames=23, min_events=0)
    out = str(clip["folder"] / "cli_staged.y4m")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    p = subprocess.run([sys.executable, "-m", "swiftwatcher_amd", clip["y4m_23"], "--corners", "%d,%d,%d,%d" % (CORNERS[0] + CORNERS[1]),
                        "--review", out, "--review-stages", ",".join(STAGES)], capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert p.returncode == 0, p.stdout + p.stderr
    line = json.loads(p.stdout.strip().splitlines()[-1])
    assert line["source"] == clip["y4m_23"] and line["frames"] == 23
    assert open(out, "rb").read() == open(str(clip["folder"] / "inproc_staged.y4m"), "rb").read()


def test_frames_without_device_planes_take_the_host_path(clip):
    """The windows of a FrameQueue(keep_stages=True) written twice: as popped (the frames carry the window's DevicePlanes: the panels
    name that memory) and as hand-made Frames whose processed_frames are numpy arrays (stacked on the host and uploaded).  The same
    bytes; with text on, too."""
    from swiftwatcher_amd.data_structures import Frame
    from swiftwatcher_amd.review import ReviewWriter
    roi_mask = _mask(CROP_ODD, 27)
    images, windows = _stage_reference(clip["y4m"], CROP_ODD)
    paths = [str(clip["folder"] / ("path_%s.y4m" % k)) for k in ("device", "host")]
    taken = []
    for path, by_hand in zip(paths, (False, True)):
        with ReviewWriter(path, CROP_ODD, roi_mask, 30, stages=STAGES + ("rpca",), text=True, stage_cols=2) as w:
            plan_panels = w.plan_panels

            def spy(frames, plan_panels=plan_panels):
                panels, held = plan_panels(frames)
                taken.append("device" if held is not None else "host")
                return panels, held
            w.plan_panels = spy
            for popped in windows:
                assert all(fr.stage_planes is not None and fr.stage_planes[1] == len(popped) - 1 - k for k, fr in enumerate(popped))
                if by_hand:
                    made = []
                    for fr in popped:
                        new = Frame(fr.frame, fr.frame_number, fr.timestamp)
                        new.segments = fr.segments
                        if fr.frame_number >= 0:
                            new.processed_frames.update({NAMES[k]: images[fr.frame_number][k] for k in STAGES})
                        made.append(new)
                    popped = made
                w.write_window(popped)
            assert w.frames == len(images) >= 52 and (w.frame_height, w.frame_width) == (3 * 64, 2 * 96)
    assert taken == ["device"] * len(windows) + ["host"] * len(windows) and len(windows) == 3
    assert open(paths[0], "rb").read() == open(paths[1], "rb").read()
