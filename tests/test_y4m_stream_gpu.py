"""The counting loop over a YUV4MPEG2 pipe (io_y4m.Y4MStreamReader) on the MI355X: staging of rectangle-holding frames, count_swifts,
the reader that segments ahead, several videos in flight and python -m swiftwatcher_amd -- each equal to the same bytes read from a
file.  The clip recipe is tests/test_yuv_gpu.py's."""
import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import yuv_formats_ref as fref
import yuv_ref
from test_yuv_gpu import CROP, CROP_ODD, _event_records, _queue_run, _same_windows

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CORNERS = ((40, 71), (116, 71))          # the top edge of the clip's chimney (synthetic._background inside CROP)


@pytest.fixture(scope="module")
def clips(tmp_path_factory):
    """The seeded 52-frame 110 x 160 clip as an 8-bit 4:2:0 and a C422p10 file, the first 42 frames of the former, and their bytes."""
    from swiftwatcher_amd import synthetic
    from swiftwatcher_amd.io_y4m import Y4MWriter
    bgr = synthetic.full_frames(500, 52, CROP, frame_hw=(110, 160), birds=4, bird_len=(8, 12), bird_wid=(3, 5))[::-1].copy()
    folder = tmp_path_factory.mktemp("y4m_stream_gpu")
    out = {}
    y, u, v = yuv_ref.bgr_to_yuv420(bgr)
    for name, count in (("420", 52), ("420_42", 42)):
        path = str(folder / (name + ".y4m"))
        with Y4MWriter(path, 160, 110, 30) as w:
            for k in range(count):
                w.append(y[k], u[k], v[k])
        out[name] = path
    y, u, v = fref.bgr_to_planes(bgr, (1, 0), 10, False, False)
    out["422p10"] = str(folder / "422p10.y4m")
    with Y4MWriter(out["422p10"], 160, 110, 30, chroma="422", bits=10) as w:
        for k in range(52):
            w.append(y[k], u[k], v[k])
    for name in list(out):
        with open(out[name], "rb") as fh:
            out[name, "bytes"] = fh.read()
    return out


class _Pipe:
    """An os.pipe fed with `data` by a thread: .source is the read end (a descriptor)."""

    def __init__(self, data):
        self.source, w = os.pipe()

        def feed():
            try:
                at = 0
                while at < len(data):
                    at += os.write(w, data[at:at + 65536])
            except OSError:
                pass
            finally:
                os.close(w)
        self._thread = threading.Thread(target=feed, daemon=True)
        self._thread.start()

    def close(self):
        os.close(self.source)          # (a feeder still writing ends with EPIPE)
        self._thread.join(10)
        assert not self._thread.is_alive()


# ------------------------------------------------------------------------------------------ 1. staging is bit for bit
@pytest.mark.parametrize("crop", [CROP, CROP_ODD], ids=["even", "odd"])
@pytest.mark.parametrize("fmt", ["420", "422p10"])
def test_staging_of_rectangle_frames_is_bit_for_bit(clips, fmt, crop):
    from swiftwatcher_amd import _lib
    from swiftwatcher_amd.data_structures import stack_frames
    from swiftwatcher_amd.io_y4m import open_y4m
    import io
    ctx = _lib.default_context(0)
    on_file = open_y4m(clips[fmt])
    stream = open_y4m(io.BytesIO(clips[fmt, "bytes"]), crop_region=crop)
    for _ in range(2):
        want_frames = on_file.get_n_frames(5)[0][::-1]
        got_frames = stream.get_n_frames(5)[0][::-1]
        assert all(hasattr(f, "origin") and f.y.shape[0] < 110 and f.y.shape[1] < 160 for f in got_frames)
        want = stack_frames(want_frames, crop, (24, 24), ctx.staging, 0)
        want_stack = want[0].cpu().numpy().copy()
        got = stack_frames(got_frames, crop, (24, 24), ctx.staging, 0)
        assert got[1:] == want[1:]
        assert got[0].is_cuda and tuple(got[0].shape) == want_stack.shape and np.array_equal(got[0].cpu().numpy(), want_stack)
        (x0, y0), (x1, y1) = crop
        assert np.array_equal(want_stack[0][got[1][1]:got[1][1] + y1 - y0, got[1][0]:got[1][0] + x1 - x0], np.asarray(want_frames[0])[y0:y1, x0:x1])
    # frames that hold another rectangle cannot join, and a rectangle that is too small is refused
    other = open_y4m(io.BytesIO(clips[fmt, "bytes"]), crop_region=[(crop[0][0] + 2, crop[0][1]), crop[1]]).get_n_frames(1)[0]
    with pytest.raises(ValueError):
        stack_frames(got_frames[:2] + other, crop, (24, 24), ctx.staging, 0)
    with pytest.raises(ValueError):
        stack_frames(got_frames, [(crop[0][0] - 16, crop[0][1]), crop[1]], (24, 24), ctx.staging, 0)
    stream.close()


# ------------------------------------------------------------------------------------------ 2. the counting loop over a pipe
@pytest.mark.parametrize("regions", ["crop_region", "corners"])
@pytest.mark.parametrize("wpc", [1, 2])
@pytest.mark.parametrize("name", ["420", "420_42"])
def test_count_swifts_over_a_pipe(clips, name, wpc, regions):
    """52 frames = two windows and a padded one; 42 = two windows and none."""
    from swiftwatcher_amd import pipeline
    roi_mask = np.zeros((64, 96), np.uint8)
    roi_mask[28:, :] = 255
    kw = dict(crop_region=CROP, roi_mask=roi_mask) if regions == "crop_region" else dict(corners=CORNERS)
    want = pipeline.count_swifts(clips[name], windows_per_call=wpc, **kw)
    print("%s %s windows_per_call=%d: count %d, %d events" % (name, regions, wpc, want[0], len(want[1])))
    assert len(want[1]) >= 1, "the run over the file has no event: equality would be vacuous"
    pipe = _Pipe(clips[name, "bytes"])
    try:
        got = pipeline.count_swifts(pipe.source, windows_per_call=wpc, **kw)
    finally:
        pipe.close()
    assert got[0] == want[0] and _event_records(got[1]) == _event_records(want[1])


# ------------------------------------------------------------------------------------------ 3. the reader that segments ahead
def test_presegmenting_reader_over_a_stream_reader(clips):
    from swiftwatcher_amd.io_frames import PresegmentingReader
    from swiftwatcher_amd.io_y4m import open_y4m
    runs = []
    pipe = _Pipe(clips["420", "bytes"])
    try:
        for inner in (open_y4m(pipe.source, crop_region=CROP), open_y4m(clips["420"])):
            reader = PresegmentingReader(inner, crop_region=CROP, queue_size=21, windows=2)
            runs.append(_queue_run(reader, 21, CROP, 3))
            reader.close()
    finally:
        pipe.close()
    assert any(f["segs"] for w in runs[1] for f in w["frames"])
    _same_windows(runs[0], runs[1])


# ------------------------------------------------------------------------------------------ 4. several videos in flight
def test_a_stream_and_a_file_in_flight(clips):
    from swiftwatcher_amd import pipeline
    roi_mask = np.zeros((64, 96), np.uint8)
    roi_mask[28:, :] = 255
    regions = [(CROP, roi_mask), (CROP_ODD, roi_mask)]
    lone = [pipeline.count_swifts(clips["420"], CROP, roi_mask), pipeline.count_swifts(clips["422p10"], CROP_ODD, roi_mask)]
    assert len(lone[0][1]) >= 1
    for wpc in (1, 2):
        pipe = _Pipe(clips["420", "bytes"])
        try:
            both = pipeline.count_swifts_videos([pipe.source, clips["422p10"]], regions=regions, in_flight=2, windows_per_call=wpc)
        finally:
            pipe.close()
        for got, want in zip(both, lone):
            assert got[0] == want[0] and _event_records(got[1]) == _event_records(want[1])


# ------------------------------------------------------------------------------------------ 5. the entry point
def test_entry_point_reads_standard_input(clips, tmp_path):
    from swiftwatcher_amd import event_classification as ec
    from swiftwatcher_amd import pipeline
    from swiftwatcher_amd.io_data import export_results
    from swiftwatcher_amd.io_y4m import open_y4m
    reader = open_y4m(clips["420"])
    count, events = pipeline.count_swifts(reader, corners=CORNERS)
    assert len(events) >= 1
    want_dir, got_dir = tmp_path / "want", tmp_path / "got"
    export_results(str(want_dir), ec.classify_events(events), reader.fps, reader.start_frame, reader.end_frame)
    with open(clips["420"], "rb") as fh:
        done = subprocess.run(["timeout", "-k", "10", "120", sys.executable, "-m", "swiftwatcher_amd", "-", "--corners", "40,71,116,71", "--out", str(got_dir)],
                              stdin=fh, cwd=ROOT, capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
    lines = [ln for ln in done.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    assert json.loads(lines[0]) == {"source": "-", "frames": 52, "events": len(events), "count": count}
    names = sorted(os.listdir(str(want_dir)))
    assert len(names) == 6 and sorted(os.listdir(str(got_dir))) == names
    for name in names:
        assert (got_dir / name).read_bytes() == (want_dir / name).read_bytes(), name
    # an unreadable source: one line on stderr, a non-zero exit status
    done = subprocess.run(["timeout", "-k", "10", "120", sys.executable, "-m", "swiftwatcher_amd", "-", "--corners", "40,71,116,71"],
                          stdin=subprocess.DEVNULL, cwd=ROOT, capture_output=True, text=True)
    assert done.returncode == 1 and done.stdout == "" and len(done.stderr.strip().splitlines()) == 1 and "not a YUV4MPEG2 file" in done.stderr
