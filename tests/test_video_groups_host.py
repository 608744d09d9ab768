"""Host side of counting several videos at once: the call planner, the in-flight scheduler (driven by a stub segmenter, no GPU) and
the C ABI's new symbol."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_groups_symbol_is_exported_and_declared():
    from swiftwatcher_amd import _lib
    assert "swk_batch_run_groups" in _lib.EXPORTS
    with open(os.path.join(ROOT, "include", "swk.h")) as f:
        assert "int32_t swk_batch_run_groups(swk_ctx *ctx, const swk_input *groups, int32_t ngroups" in f.read()


def test_planner_keeps_similar_sizes_together_largest_first():
    from swiftwatcher_amd.pipeline import plan_calls
    assert plan_calls([("a", 100, 1), ("b", 60, 1), ("c", 40, 1)], 21) == [["a", "b", "c"]]          # 300 padded vs 200 own
    assert plan_calls([("s", 400, 2), ("b", 9000, 1)], 21) == [["b"], ["s"]]           # 27000 padded vs 9800 own
    assert plan_calls([], 21) == []


def test_planner_padding_factor_boundary():
    from swiftwatcher_amd.pipeline import plan_calls
    # two windows: P = 100 and p.  Padded elements 200, own 100 + p: exactly twice at p = 0 .. split only when MORE than twice
    assert plan_calls([("a", 100, 1), ("b", 50, 1)], 21) == [["a", "b"]]           # 200 <= 2 * 150
    assert plan_calls([("a", 100, 1), ("b", 50, 1)], 21, pad_factor=1.33) == [["a"], ["b"]]      # 200 > 1.33 * 150 = 199.5
    assert plan_calls([("a", 100, 1), ("b", 50, 1)], 21, pad_factor=200 / 150) == [["a", "b"]]   # exactly the factor: kept
    # the window counts weigh in
    assert plan_calls([("a", 100, 1), ("b", 30, 3)], 21, pad_factor=2.0) == [["a"], ["b"]]       # 400 > 2 * 190
    assert plan_calls([("a", 100, 3), ("b", 30, 1)], 21, pad_factor=2.0) == [["a", "b"]]         # 400 <= 2 * 330


def test_planner_small_windows_join_without_padding():
    from swiftwatcher_amd.pipeline import plan_calls
    assert plan_calls([("t", 16, 1), ("a", 5000, 1)], 21) == [["a", "t"]]
    assert plan_calls([("t", 16, 1), ("u", 20, 2)], 21) == [["t", "u"]]


class _Reader:
    """get_n_frames / total_frames like io_frames.ArrayReader, frames are (video, index) tags; pads past the end with -1"""

    def __init__(self, v, total):
        self.v, self.total_frames, self.pos = v, total, 0

    def get_n_frames(self, n):
        frames, numbers, stamps = [], [], []
        for _ in range(n):
            k = self.pos if self.pos < self.total_frames else -1
            frames.append((self.v, k)); numbers.append(k); stamps.append("t")
            self.pos += 1
        return frames, numbers, stamps


def _run(lengths, sizes, in_flight, wpc, n=21, pad_factor=2.0):
    from swiftwatcher_amd.pipeline import schedule_videos
    readers = [_Reader(v, t) for v, t in enumerate(lengths)]
    seen = {v: [] for v in range(len(lengths))}
    calls = []

    def segment(groups):
        calls.append([v for v, _ in groups])
        return [[list(frames) for frames, _, _ in windows] for _, windows in groups]

    def consume(v, popped):
        for frames in popped:
            seen[v].extend(k for vv, k in frames if k >= 0 and vv == v)
    log = schedule_videos(readers, sizes, segment, consume, in_flight=in_flight, windows_per_call=wpc, queue_size=n,
                          pad_factor=pad_factor)
    return seen, calls, log


def test_scheduler_every_video_sees_its_frames_in_order():
    lengths = [52, 47, 65, 30, 44]
    for in_flight in (1, 2, 4, 8):
        for wpc in (1, 8):
            seen, calls, log = _run(lengths, [5000] * 5, in_flight, wpc)
            for v, t in enumerate(lengths):
                assert seen[v] == list(range(t)), (in_flight, wpc, v)
            assert all(len(c) <= in_flight for c in calls)


def test_scheduler_replaces_finished_videos_in_input_order():
    # 1 window, 3, 1, 2 windows of 21 frames; two in flight, one window per call
    seen, calls, log = _run([21, 60, 10, 42], [5000] * 4, 2, 1)
    assert calls == [[0, 1], [1, 2], [1, 3], [3]]
    assert log == [[(0, 1), (1, 1)], [(1, 1), (2, 1)], [(1, 1), (3, 1)], [(3, 1)]]
    # in_flight 1 = one video after the other
    seen, calls, log = _run([21, 60, 10], [5000] * 3, 1, 8)
    assert calls == [[0], [1], [2]] and log == [[(0, 1)], [(1, 3)], [(2, 1)]]


def test_scheduler_splits_calls_the_planner_splits():
    seen, calls, log = _run([42, 42, 42], [100, 9000, 3000], 3, 1)          # 9000 + 3000 together; 100 more would pad 27000 vs 12100
    assert calls == [[1, 2], [0], [1, 2], [0]]
    for v in range(3):
        assert seen[v] == list(range(42))


def test_count_swifts_videos_without_gpu_uses_the_scheduler(monkeypatch):
    """count_swifts_videos hands every video's frames to its own tracker in order, through the scheduler (segmenter stubbed)."""
    from swiftwatcher_amd import pipeline
    stepped = {}

    class Tracker:
        def __init__(self, mask):
            self.mask, self.detected_events = mask, []
            stepped[id(self)] = self.frames = []

        def step(self, frame):
            self.frames.append(frame)

    def fake_groups(groups, min_seg_size, device=0, params=None, classifier=None):
        return [[list(frames) for frames, _, _ in windows] for windows, _ in groups]
    monkeypatch.setattr(pipeline, "SegmentTracker", Tracker)
    monkeypatch.setattr(pipeline, "segment_window_groups", fake_groups)
    vids = [np.arange(t, dtype=np.uint8).reshape(t, 1, 1).repeat(4, 1).repeat(4, 2) for t in (25, 50, 7)]
    regions = [([(0, 0), (4, 4)], np.zeros((4, 4), np.uint8))] * 3
    out = pipeline.count_swifts_videos(vids, regions=regions, in_flight=2)
    assert [c for c, _ in out] == [0, 0, 0]
    per = list(stepped.values())
    for frames, t in zip(per, (25, 50, 7)):
        real = [int(f[0, 0]) for f in frames[:t]]
        assert real == list(range(t))
        assert len(frames) % 21 == 0
