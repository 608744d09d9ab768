"""The counting loop over an interlaced clip: count_swifts(..., deinterlace="bob") against count_swifts over an ArrayReader of the
restatement's BGR pictures (tests/deinterlace_ref.py) at twice the rate -- events, counts and CSV tables; from a file, from a pipe,
with several windows per call, through count_swifts_videos, with a review video, with the stabilizer on top, and through the CLI."""
import json
import os
import threading

import numpy as np
import pytest

import deinterlace_ref as ref
import pipeline_options
import yuv_ref

pytestmark = pytest.mark.gpu

CORNERS = pipeline_options.CLIPS[0]["corners"]
FPS = 30          # of the stored frames


@pytest.fixture(scope="module")
def clip(tmp_path_factory):
    """52 field-rate pictures (the still twin of the option tests' first clip: 110 x 160, a 47 x 94 crop region from the chimney's
    corners, small faint birds, noise) woven into 26 stored 4:2:0 frames, top field first; the restatement's 52 BGR pictures; the
    files"""
    from swiftwatcher_amd.io_y4m import Y4MWriter
    folder = tmp_path_factory.mktemp("deint_loop")
    shown = np.ascontiguousarray(pipeline_options.clip(0)["still"])
    y, u, v = yuv_ref.bgr_to_yuv420(shown)
    stored = tuple(ref.weave(p[0::2], p[1::2]) for p in (y, u, v))
    pictures = ref.call_bgr(*(p.astype(np.int64) for p in stored), subsampling=(1, 1), tff=True)
    paths = {}
    for name, planes, order, fps in (("interlaced", stored, "t", FPS), ("progressive", (y, u, v), "p", 2 * FPS)):
        paths[name] = str(folder / (name + ".y4m"))
        with Y4MWriter(paths[name], 160, 110, fps, interlaced=order) as w:
            for k in range(len(planes[0])):
                w.append(planes[0][k], planes[1][k], planes[2][k])
    return dict(folder=folder, stored=stored, pictures=pictures, paths=paths, N=len(stored[0]))


def _count(entry, *args, **kw):
    """pipeline.count_swifts / count_swifts_videos with the trackers spied on -> per video (count, events as tuples, the segments every
    frame number came to its tracker with), and the raw results"""
    from swiftwatcher_amd import pipeline
    made = []

    class Spy(pipeline.SegmentTracker):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            self.seen = {}
            made.append(self)

        def _note(self, frame):
            if frame.frame_number >= 0:
                self.seen[frame.frame_number] = [(str(frame.timestamp), s.label, tuple(s.bbox), tuple(s.centroid), s.area) for s in frame.segments]

        def set_current_frame(self, frame):
            self._note(frame)
            super().set_current_frame(frame)

        def step_window(self, frames):
            for frame in frames:
                self._note(frame)
            return super().step_window(frames)

    saved = pipeline.SegmentTracker
    pipeline.SegmentTracker = Spy
    try:
        raw = getattr(pipeline, entry)(*args, **kw)
    finally:
        pipeline.SegmentTracker = saved
    results = raw if entry == "count_swifts_videos" else [raw]
    sigs = [(count, [[(s.parent_frame_number, str(s.parent_timestamp), s.label, tuple(s.bbox)) for s in ev] for ev in events], t.seen)
            for (count, events), t in zip(results, made)]
    return sigs, results


def _tables(folder, events, fps, last):
    """the CSV tables of a count, as {file name: bytes}"""
    from swiftwatcher_amd import event_classification as ec
    from swiftwatcher_amd.io_data import export_results
    if not events:
        return {}
    os.makedirs(folder, exist_ok=True)
    export_results(str(folder), ec.classify_events(events), fps, 0, last)
    return {name: open(os.path.join(folder, name), "rb").read() for name in sorted(os.listdir(folder))}


@pytest.fixture(scope="module")
def expected(clip):
    """the count over the restatement's pictures handed over already progressive, at twice the rate"""
    from swiftwatcher_amd.io_frames import ArrayReader
    (sig,), (result,) = _count("count_swifts", ArrayReader(list(clip["pictures"]), fps=2.0 * FPS), corners=CORNERS)
    seen = sig[2]
    print("expected: count %d, %d events, %d segments in %d pictures" % (sig[0], len(sig[1]), sum(len(v) for v in seen.values()), len(seen)))
    assert sorted(seen) == list(range(2 * clip["N"] + 1)) and sum(len(v) for v in seen.values()) > 30, "the clip gives the tracker too little"
    return dict(result=result, sig=sig, tables=_tables(str(clip["folder"] / "want"), result[1], 2.0 * FPS, 2 * clip["N"]))


def test_bob_from_a_file(clip, expected):
    (sig,), (result,) = _count("count_swifts", clip["paths"]["interlaced"], corners=CORNERS, deinterlace="bob")
    assert sig == expected["sig"]
    assert _tables(str(clip["folder"] / "got"), result[1], 2.0 * FPS, 2 * clip["N"]) == expected["tables"]
    # ... which is not what the stored frames give as they are: 26 frames, and other segments in them
    (woven,), _ = _count("count_swifts", clip["paths"]["interlaced"], corners=CORNERS, deinterlace="weave")
    assert sorted(woven[2]) == list(range(clip["N"] + 1))
    assert sum([s[1:] for s in woven[2][t]] != [s[1:] for s in sig[2][2 * t]] for t in range(clip["N"])) > clip["N"] // 2


def test_bob_from_a_pipe(clip, expected):
    data = open(clip["paths"]["interlaced"], "rb").read()
    rd, wr = os.pipe()

    def feed():
        with os.fdopen(wr, "wb") as out:
            out.write(data)

    feeder = threading.Thread(target=feed, daemon=True)
    feeder.start()
    with os.fdopen(rd, "rb", buffering=0) as source:
        (sig,), _ = _count("count_swifts", source, corners=CORNERS, deinterlace="bob")
    feeder.join()
    assert sig == expected["sig"]


def test_bob_with_four_windows_per_call(clip, expected):
    (sig,), _ = _count("count_swifts", clip["paths"]["interlaced"], corners=CORNERS, deinterlace="bob", windows_per_call=4)
    assert sig == expected["sig"]


def test_an_interlaced_and_a_progressive_video_in_one_round(clip, expected):
    (alone,), _ = _count("count_swifts", clip["paths"]["progressive"], corners=CORNERS)
    both, _ = _count("count_swifts_videos", [clip["paths"]["interlaced"], clip["paths"]["progressive"]], corners=[CORNERS, CORNERS],
                     deinterlace=["bob", None])
    assert both == [expected["sig"], alone]


def test_review_has_2n_frames_at_the_doubled_rate(clip, expected):
    from swiftwatcher_amd import pipeline
    from swiftwatcher_amd.io_frames import ArrayReader
    from swiftwatcher_amd.io_y4m import Y4MReader
    got, want = str(clip["folder"] / "review_got.y4m"), str(clip["folder"] / "review_want.y4m")
    (sig,), _ = _count("count_swifts", clip["paths"]["interlaced"], corners=CORNERS, deinterlace="bob", review=got)
    assert sig == expected["sig"]
    pipeline.count_swifts(ArrayReader(list(clip["pictures"]), fps=2.0 * FPS), corners=CORNERS, review=want)
    r = Y4MReader(got)
    assert r.rate == (2 * FPS, 1) and r.total_frames >= 2 * clip["N"]
    assert open(got, "rb").read() == open(want, "rb").read()


def test_stabilizer_on_top(clip, expected):
    """the clip does not shake: stabilize=4 over the deinterlaced pictures finds no shift and gives the unstabilized count"""
    (sig,), _ = _count("count_swifts", clip["paths"]["interlaced"], corners=CORNERS, deinterlace="bob", stabilize=4)
    assert sig == expected["sig"]


def test_cli_prints_the_deinterlace_object(clip, expected, capsys):
    from swiftwatcher_amd import __main__ as cli
    corners = "%d,%d,%d,%d" % (CORNERS[0] + CORNERS[1])
    assert cli.main([clip["paths"]["interlaced"], "--corners", corners, "--deinterlace", "bob"]) == 0
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    N = clip["N"]
    assert line["deinterlace"] == {"mode": "bob", "field_order": "t", "stored_frames": N, "frames": 2 * N}
    assert line["frames"] == 2 * N and line["count"] == expected["sig"][0] and line["events"] == len(expected["sig"][1])
    assert cli.main([clip["paths"]["progressive"], "--corners", corners]) == 0
    assert "deinterlace" not in json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    # refusals through the CLI: exit status 1 and the reason on standard error
    assert cli.main([clip["paths"]["progressive"], "--corners", corners, "--deinterlace", "bob"]) == 1
    assert "progressive" in capsys.readouterr().err
    assert cli.main([clip["paths"]["interlaced"], "--corners", corners]) == 1
    err = capsys.readouterr().err
    assert "interlaced YUV4MPEG2 files are not supported" in err and "--deinterlace" in err


def test_refusals(clip):
    from swiftwatcher_amd import pipeline
    with pytest.raises(ValueError, match="progressive"):
        pipeline.count_swifts(clip["paths"]["progressive"], corners=CORNERS, deinterlace="bob")
    with pytest.raises(ValueError, match="interlaced YUV4MPEG2 files are not supported"):
        pipeline.count_swifts(clip["paths"]["interlaced"], corners=CORNERS)
    with pytest.raises(ValueError, match="one of"):
        pipeline.count_swifts(clip["paths"]["interlaced"], corners=CORNERS, deinterlace="blend")
