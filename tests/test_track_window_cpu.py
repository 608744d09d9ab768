"""SegmentTracker.step_window / swk_track_window: a whole window of frames per library call must leave exactly what per-frame stepping
leaves -- the same events, made of the very Segment objects that were handed in -- on the recorded reference traces, when the two paths
are mixed at random boundaries, and on seeded random streams with and without exact cost ties.  Host logic: no GPU."""
import os

import numpy as np
import pytest

from swiftwatcher_amd import _lib
from swiftwatcher_amd.data_structures import Frame
from swiftwatcher_amd import segment_tracking as st
from swiftwatcher_amd import event_classification as ec

TRACES = ["tracker_a", "tracker_b", "tracker_sparse", "tracker_crowd", "tracker_long", "tracker_grid"]
WINDOWS = [1, 2, 21, 64, None]          # None: the whole trace as one window


class _Seg:
    def __init__(self, label, centroid, t):
        self.label = label
        self.centroid = centroid
        self.status = None
        self.segment_history = []
        self.parent_frame_number = t
        self.parent_timestamp = "ts%05d" % t
        self.segment_image = None


def _frames(counts, cents):
    """Fresh Frame and segment objects of a stream: counts[t] segments in frame t, their centroids row after row in cents."""
    out, off = [], 0
    for t, k in enumerate(counts):
        fr = Frame(None, t, "ts%05d" % t)
        fr.segments = [_Seg(i + 1, (float(cents[off + i][0]), float(cents[off + i][1])), t) for i in range(int(k))]
        off += int(k)
        out.append(fr)
    return out


def _key(events):
    return [[(s.parent_frame_number, s.label, s.centroid) for s in e] for e in events]


def _six_calls(tracker, frame):
    tracker.set_current_frame(frame)
    tracker.store_assignments(st.apply_hungarian_algorithm(tracker.formulate_cost_matrix()))
    tracker.link_matching_segments()
    tracker.check_for_events()
    tracker.cache_current_frame()


def _per_frame(roi, counts, cents):
    tracker = st.SegmentTracker(roi)
    for fr in _frames(counts, cents):
        tracker.step(fr)
    return tracker


def _by_windows(roi, frames, size):
    tracker = st.SegmentTracker(roi)
    size = size or max(len(frames), 1)
    for at in range(0, len(frames), size):
        tracker.step_window(frames[at:at + size])
    return tracker


def _cached_state(tracker):
    """The cached frame as the next step reads it: per segment its centroid and its history as centroids."""
    return [(s.centroid, [(m.parent_frame_number, m.label, m.centroid) for m in s.segment_history])
            for s in tracker.get_cached_frame().segments]


_reference = {}


def _trace(golden_dir, name):
    """(fixture, event keys of the per-frame replay): made once per trace and left alone."""
    if name not in _reference:
        g = np.load(os.path.join(golden_dir, name + ".npz"))
        g = {k: g[k] for k in g.files}
        _reference[name] = (g, _key(_per_frame(g["roi"], g["counts"], g["centroids"]).detected_events))
    return _reference[name]


def _check_fixture(g, events):
    """What the reference recorded about the trace's events (oracle/make_tracker_goldens.py)."""
    assert [e[-1].parent_frame_number for e in events] == list(g["ev_last_frame"])
    assert [len(e) for e in events] == list(g["ev_len"])
    np.testing.assert_array_equal(np.array([e[0].centroid for e in events]).reshape(-1, 2), g["ev_first"])
    np.testing.assert_array_equal(np.array([e[-1].centroid for e in events]).reshape(-1, 2), g["ev_last"])
    np.testing.assert_array_equal(np.array([ec.compute_angle([s.centroid for s in e]) for e in events]), g["angles_all"])
    assert ec.classify_events(events)["label"] == list(g["labels"])
    assert ec.count_swifts(events) == int(g["total"])


@pytest.mark.parametrize("window", WINDOWS, ids=lambda w: "w%s" % (w or "all"))
@pytest.mark.parametrize("name", TRACES)
def test_traces_by_windows(golden_dir, name, window):
    g, expected = _trace(golden_dir, name)
    frames = _frames(g["counts"], g["centroids"])
    handed = {(s.parent_frame_number, s.label): s for fr in frames for s in fr.segments}
    tracker = _by_windows(g["roi"], frames, window)
    events = tracker.detected_events
    assert len(expected) > 0 and _key(events) == expected
    for e in events:
        for s in e:
            assert s is handed[(s.parent_frame_number, s.label)]
    assert tracker.current_frame is frames[-1] and tracker.cached_frame is frames[-1]
    if name != "tracker_grid":          # (its recorded events follow another SciPy's tie-breaking: tests/test_tracking_counts.py)
        _check_fixture(g, events)


@pytest.mark.parametrize("name", ["tracker_crowd", "tracker_grid"])
def test_mixing_the_paths_at_random_boundaries(golden_dir, name):
    g, expected = _trace(golden_dir, name)
    used = set()
    for seed in range(24):
        rng = np.random.default_rng(1000 + seed)
        frames = _frames(g["counts"], g["centroids"])
        tracker = st.SegmentTracker(g["roi"])
        at = 0
        while at < len(frames):
            mode = int(rng.integers(0, 3))
            run = int(rng.integers(1, 40))
            chunk = frames[at:at + run]
            at += len(chunk)
            used.add(mode)
            if mode == 0:
                for fr in chunk:
                    tracker.step(fr)
            elif mode == 1:
                for fr in chunk:
                    _six_calls(tracker, fr)
            else:
                tracker.step_window(chunk)
        assert _key(tracker.detected_events) == expected, seed
        assert tracker.cached_frame is frames[-1]
    assert used == {0, 1, 2}


def _random_stream(rng, H, W, nframes, snap):
    """Birds that fly straight with some jitter, appear and vanish: (counts, centroids) with 0-12 segments per frame inside H x W."""
    birds, counts, cents = [], [], []
    for _ in range(nframes):
        birds = [(p + v + rng.normal(0, 0.7, 2), v) for p, v in birds if rng.random() > 0.12]
        birds = [(p, v) for p, v in birds if 0 <= p[0] < H and 0 <= p[1] < W]
        while len(birds) < 12 and rng.random() < 0.45:
            birds.append((rng.uniform((0, 0), (H, W)), rng.normal(0, 4, 2)))
        if rng.random() < 0.08:
            birds = []
        order = rng.permutation(len(birds))
        pts = [birds[i][0] for i in order]
        if snap:
            pts = [np.minimum(np.floor(p / 4) * 4, (H - 4, W - 4)) for p in pts]
        counts.append(len(pts))
        cents.extend((float(p[0]), float(p[1])) for p in pts)
    return counts, cents


def test_seeded_streams_window_path_equals_per_frame_path():
    H, W = 64, 96
    events = tied = 0
    for stream in range(200):
        rng = np.random.default_rng(5000 + stream)
        roi = np.zeros((H, W), np.uint8)
        r0, c0 = int(rng.integers(0, H - 8)), int(rng.integers(0, W - 8))
        roi[r0:r0 + int(rng.integers(8, H)), c0:c0 + int(rng.integers(8, W))] = 255
        snap = stream % 2 == 1
        counts, cents = _random_stream(rng, H, W, 60, snap)
        assert max(counts) <= 12
        want = _per_frame(roi, counts, cents)
        got = _by_windows(roi, _frames(counts, cents), [21, 1, 7, 60][(stream // 2) % 4])
        assert _key(got.detected_events) == _key(want.detected_events), stream
        assert _cached_state(got) == _cached_state(want), stream
        events += len(want.detected_events)
        tied += snap and len(want.detected_events) > 0
    assert events > 400 and tied > 50          # the streams do make events, the snapped ones too


# ---- edges ----
def _roi():
    return np.full((40, 40), 255, np.uint8)


def _bird(t0, n, label=1):
    """n frames with one segment moving down the diagonal, numbered from t0."""
    return _frames_at(t0, [[(2.0 + 3 * k, 3.0 + 3 * k)] for k in range(n)], label)


def _frames_at(t0, per_frame, label=1):
    out = []
    for k, pts in enumerate(per_frame):
        fr = Frame(None, t0 + k, "t")
        fr.segments = [_Seg(label + i, p, t0 + k) for i, p in enumerate(pts)]
        out.append(fr)
    return out


def test_empty_window_and_null_frames():
    tracker = st.SegmentTracker(_roi())
    tracker.step_window([])                                   # the first window of a tracker, and empty
    assert tracker.current_frame is None and tracker.detected_events == []
    flight = _bird(0, 4)
    tracker.step_window(flight)                               # the first window with frames
    tracker.step_window([])
    assert tracker.cached_frame is flight[-1] and tracker.detected_events == []
    nulls = [Frame() for _ in range(5)]                       # the padding at a video's end: the bird vanishes in the first of them
    tracker.step_window(nulls)
    assert [[s for s in e] for e in tracker.detected_events] == [[fr.segments[0] for fr in flight]]
    assert tracker.cached_frame is nulls[-1] and tracker.current_frame is nulls[-1]
    tracker.step_window([Frame() for _ in range(3)])
    assert len(tracker.detected_events) == 1
    # the touched segments look as per-frame stepping leaves them
    path = tracker.detected_events[0]
    assert all(s.segment_history is path for s in path) and path[-1].status == "D"


def test_replaced_single_calls_still_see_every_frame(golden_dir):
    """A subclass that hooks one of the per-frame methods (the suite's spies do) gets its windows stepped per frame."""
    g, expected = _trace(golden_dir, "tracker_sparse")
    seen = []

    class Spy(st.SegmentTracker):
        def set_current_frame(self, frame):
            seen.append(frame.frame_number)
            super().set_current_frame(frame)

    frames = _frames(g["counts"], g["centroids"])
    spy = Spy(g["roi"])
    for at in range(0, len(frames), 21):
        spy.step_window(frames[at:at + 21])
    assert seen == list(range(len(frames))) and _key(spy.detected_events) == expected and spy._native is None
    plain = st.SegmentTracker(g["roi"])
    calls = []
    plain.step = lambda frame: calls.append(frame)          # ... and so does an instance whose step was replaced
    plain.step_window(frames[:5])
    assert calls == frames[:5]
    # the loops' helper: a tracker that only has the reference's step() is stepped per frame
    from swiftwatcher_amd import pipeline

    class OnlyStep:
        def __init__(self):
            self.frames = []

        def step(self, frame):
            self.frames.append(frame)

    only = OnlyStep()
    pipeline._track(only, frames[:3], True)
    assert only.frames == frames[:3]


def test_event_buffers_that_start_too_small_are_retried():
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "tracker_crowd.npz"))
    want = _key(_per_frame(g["roi"], g["counts"], g["centroids"]).detected_events)
    frames = _frames(g["counts"], g["centroids"])
    tracker = st.SegmentTracker(g["roi"])
    tracker.step_window(frames[:1])
    native = tracker._native
    native.event_capacity, native.ordinal_capacity = 0, 0
    tracker.step_window(frames[1:100])
    assert native.event_capacity > 0 and native.ordinal_capacity > 0
    native.event_capacity, native.ordinal_capacity = 1, 1 << 16          # events alone too small
    tracker.step_window(frames[100:150])
    native.event_capacity, native.ordinal_capacity = 1 << 10, 1          # ordinals alone too small
    tracker.step_window(frames[150:])
    assert _key(tracker.detected_events) == want


def test_capacity_error_reports_sizes_and_changes_nothing():
    lib = _lib.load()
    t = _lib.Tracker(_roi())
    nseg = np.array([1, 1, 1, 0], np.int32)
    cents = np.array([[2, 3], [5, 6], [8, 9]], np.float64)
    off, ords = np.full(8, -1, np.int64), np.full(8, -1, np.int64)
    o32, o64 = np.zeros(2, np.int32), np.zeros(3, np.int64)

    def call(ev_cap, ord_cap):
        return lib.swk_track_window(t._handle, 4, nseg.ctypes.data, cents.ctypes.data, ev_cap, ord_cap, off.ctypes.data, ords.ctypes.data,
                                    o32.ctypes.data, o64.ctypes.data, o32.ctypes.data + 4, o64.ctypes.data + 8, o64.ctypes.data + 16)
    assert call(0, 8) == _lib.ERR_CAPACITY and (int(o32[0]), int(o64[0])) == (1, 3)
    assert call(1, 2) == _lib.ERR_CAPACITY and (int(o32[0]), int(o64[0])) == (1, 3)
    assert len(t.export_state()[0]) == 0                                         # nothing was applied
    assert call(1, 3) == 0
    assert off[:2].tolist() == [0, 3] and ords[:3].tolist() == [0, 1, 2]
    assert o32.tolist() == [1, 4] and o64.tolist() == [3, 0, 3]                  # first ordinal 0; nothing live: the next ordinal


def test_argument_errors():
    lib = _lib.load()
    handle = _lib.ctypes.c_void_p()
    roi = _roi()
    assert lib.swk_tracker_create(None, 4, 4, _lib.ctypes.byref(handle)) == -1
    assert lib.swk_tracker_create(roi.ctypes.data, -1, 4, _lib.ctypes.byref(handle)) == -1
    assert lib.swk_tracker_create(roi.ctypes.data, 4, 4, None) == -1
    t = _lib.Tracker(roi)
    nseg = np.array([1, -1], np.int32)
    one = np.array([1], np.int32)
    cents = np.zeros((2, 2), np.float64)
    off, ords = np.zeros(4, np.int64), np.zeros(4, np.int64)
    o32, o64 = np.zeros(2, np.int32), np.zeros(3, np.int64)
    outs = (o32.ctypes.data, o64.ctypes.data, o32.ctypes.data + 4, o64.ctypes.data + 8, o64.ctypes.data + 16)
    bufs = (3, 4, off.ctypes.data, ords.ctypes.data)
    assert lib.swk_track_window(None, 0, None, None, *bufs, *outs) == -1
    assert lib.swk_track_window(t._handle, -1, nseg.ctypes.data, cents.ctypes.data, *bufs, *outs) == -1
    assert lib.swk_track_window(t._handle, 2, nseg.ctypes.data, cents.ctypes.data, *bufs, *outs) == -1           # a negative count
    assert lib.swk_track_window(t._handle, 1, None, cents.ctypes.data, *bufs, *outs) == -1                       # null with a count
    assert lib.swk_track_window(t._handle, 1, one.ctypes.data, None, *bufs, *outs) == -1
    assert lib.swk_track_window(t._handle, 1, one.ctypes.data, cents.ctypes.data, -1, 4, off.ctypes.data, ords.ctypes.data, *outs) == -1
    assert lib.swk_track_window(t._handle, 1, one.ctypes.data, cents.ctypes.data, 3, 4, None, ords.ctypes.data, *outs) == -1
    assert lib.swk_track_window(t._handle, 0, None, None, *bufs, *outs) == 0                                     # nframes = 0 is valid
    none = np.zeros(1, np.int32)
    assert lib.swk_track_window(t._handle, 1, none.ctypes.data, None, *bufs, *outs) == 0                         # and a frame without segments
    assert len(t.export_state()[0]) == 0
    lens = np.array([-1], np.int64)
    assert lib.swk_tracker_import(t._handle, 1, cents.ctypes.data, lens.ctypes.data, cents.ctypes.data, None) == -1
    assert lib.swk_tracker_import(t._handle, 1, None, lens.ctypes.data, cents.ctypes.data, None) == -1
    assert lib.swk_tracker_import(t._handle, -1, None, None, None, None) == -1
    assert lib.swk_tracker_import(t._handle, 0, None, None, None, None) == 0
    with pytest.raises(ValueError):
        t.track_window([2], [1.0, 2.0])
    with pytest.raises(ValueError):
        _lib.Tracker(np.zeros(5, np.uint8))


def test_a_vanished_segment_outside_the_mask():
    tracker = st.SegmentTracker(np.full((10, 10), 255, np.uint8))
    inside = _frames_at(0, [[(1.0, 1.0)], [(2.0, 2.0)]])
    tracker.step_window(inside)
    with pytest.raises(IndexError):
        tracker.step_window(_frames_at(2, [[(30.0, 3.0)], []]))
    assert tracker.cached_frame is inside[-1]                 # the refused window was not applied
    tracker.step_window([Frame()])
    assert len(tracker.detected_events) == 1
    # a negative index counts from the end, as numpy's does
    roi = np.zeros((10, 10), np.uint8)
    roi[9, 8] = 255
    for path in (0, 1):
        tracker = st.SegmentTracker(roi)
        frames = _frames_at(0, [[(-1.5, -2.5)], [(-1.2, -2.2)], []])          # int() truncates: [-1, -2]
        if path:
            tracker.step_window(frames)
        else:
            for fr in frames:
                tracker.step(fr)
        assert len(tracker.detected_events) == 1


def test_export_and_import_of_the_live_state():
    t = _lib.Tracker(_roi())
    failed, done, first, min_live, off, ords = t.track_window([1, 2, 2], [2, 2, 4, 4, 30, 30, 6, 6, 31, 31])
    assert (failed, done, first, off, ords) == (False, 3, 0, [0], [])
    cents, ordinals, offsets, chain = t.export_state()
    assert cents.tolist() == [[6, 6], [31, 31]] and ordinals.tolist() == [3, 4]
    assert offsets.tolist() == [0, 2, 3] and chain.tolist() == [0, 1, 2] and min_live == 0
    u = _lib.Tracker(_roi())
    u.track_window([3], [0, 0, 1, 1, 2, 2])                   # ordinals 0..2 are taken
    assert u.import_state(cents, [2, 1], [[2, 2], [30, 30]]) == 3
    cents2, ordinals2, offsets2, chain2 = u.export_state()    # numbered from 3: chain of 0, chain of 1, then the two segments
    assert cents2.tolist() == cents.tolist() and ordinals2.tolist() == [6, 7]
    assert offsets2.tolist() == [0, 2, 3] and chain2.tolist() == [3, 4, 5]
    # both now vanish inside the mask: the same two events, in the importing handle's numbering
    assert t.track_window([0], [])[4:] == ([0, 3, 5], [0, 1, 3, 2, 4])
    assert u.track_window([0], [])[4:] == ([0, 3, 5], [3, 4, 6, 5, 7])


def test_a_segment_without_a_status_raises_like_the_per_frame_path():
    """The None-status quirk (segment_tracking.py:139 of the reference): reached through the library's white-box hook
    swk_debug_tracker_force_assignment, because no state that can be imported makes the solver return such an assignment (it would
    have to prefer two 1 + eps cells to two diagonal cells of cost 1)."""
    def stream():
        return _bird(0, 2) + [Frame(None, 2, "t")] + _frames_at(3, [[(5.0, 5.0), (20.0, 20.0)]]) + _bird(4, 2)
    swapped = [1, 0]                      # frame 3: no previous segments, both current ones off their diagonal
    want = st.SegmentTracker(_roi())
    frames = stream()
    for fr in frames[:3]:
        want.step(fr)
    want.set_current_frame(frames[3])
    want.formulate_cost_matrix()
    want.store_assignments(swapped)
    with pytest.raises(TypeError):
        want.link_matching_segments()
    assert len(want.detected_events) == 1

    got = st.SegmentTracker(_roi())
    frames = stream()
    got.step_window([])
    got._native_state().force_assignment(swapped, skip_frames=3)
    with pytest.raises(TypeError):
        got.step_window(frames)
    assert _key(got.detected_events) == _key(want.detected_events)          # the frames before it were applied
    assert got.cached_frame is frames[2] and got.current_frame is frames[3]
    # both go on from there alike
    rest = stream()[3:]
    for fr in rest:
        want.step(fr)
    got.step_window(frames[3:])
    got.step_window([Frame()])
    want.step(Frame())
    assert _key(got.detected_events) == _key(want.detected_events) and len(got.detected_events) == 2
