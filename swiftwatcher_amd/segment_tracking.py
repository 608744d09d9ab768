"""Drop-in for the reference's swiftwatcher/segment_tracking.py (SegmentTracker :17-176, module functions
:179-263) -- SURVEY.md section 8f rank 1, the step right after the segment path.  Same class, method names
and call order as the counting loop uses (__main__.py:87-92); the cost matrix and the assignment solve run in
C++ inside libswk (host code, no GPU: this is sequential per-frame logic on a few dozen segments), the
status / history / event bookkeeping is re-implemented here.

Quirks of the reference that are behaviour, and kept:
  * segment histories are ONE list shared along a chain of matches (:149-152), so appending to it updates
    every earlier segment's view; an event's motion path is that same list plus the vanished segment (:174-176);
  * a current-frame segment that is neither matched nor "A"ppeared keeps status None and link_matching_segments
    then indexes a list with None (TypeError) -- only reachable when the solver picks an "impossible" cell;
  * the cost of not matching is 1 and impossible cells cost 1 + eps (:186, :254): a pair is matched only when
    its cost is below 1 - eps.
"""
import numpy as np

from . import _lib
from .data_structures import Frame


def intialize_cost_matrix(n_curr, n_prev):          # (sic) the reference's spelling, :179-186
    n = n_curr + n_prev
    return np.ones((n, n)) + np.finfo(np.float64).eps


def calculate_nonmatch_cost():                        # :250-254
    return 1


def apply_hungarian_algorithm(cost_matrix):
    """:257-263.  Column chosen for every row, with scipy.optimize.linear_sum_assignment's tie-breaking."""
    cost_matrix = np.asarray(cost_matrix, np.float64)
    if cost_matrix.size == 0:
        return np.zeros(0, np.int32)
    return _lib.lsap(cost_matrix)


class SegmentTracker:
    def __init__(self, roi_mask):
        self.current_frame = None
        self.cached_frame = Frame()                   # empty frame, no segments (:28)
        self.roi_mask = roi_mask
        self.detected_events = []
        # step_window's side: the library handle, the frame whose state it holds (None: this object's attributes hold it), and
        # the Segment objects a later event can still name, _store[k] being ordinal _store_base + k
        self._native = None
        self._native_mask = None
        self._native_frame = None
        self._store = []
        self._store_base = 0

    def get_current_frame(self):
        return self.current_frame

    def get_cached_frame(self):
        if self._native_frame is not None:
            self._materialise()
        return self.cached_frame

    def set_current_frame(self, frame):
        if self._native_frame is not None:          # the last frames went through step_window: hand the state back first
            self._materialise()
        self.current_frame = frame

    def cache_current_frame(self):
        self.cached_frame = self.current_frame

    def formulate_cost_matrix(self):
        """:46-102, one C call instead of a Python double loop with scipy/math scalar calls."""
        prev, curr = self.cached_frame.segments, self.current_frame.segments
        flat = [c for s in prev for c in s.centroid]
        flat += [c for s in prev for c in (s.segment_history[0].centroid if s.segment_history else (0.0, 0.0))]
        flat += [c for s in curr for c in s.centroid]
        flags = bytes([1 if s.segment_history else 0 for s in prev])
        return _lib.track_costs_packed(np.array(flat, np.float64), flags, len(prev), len(curr))

    def store_assignments(self, assignments):
        """:104-131."""
        prev, curr = self.cached_frame.segments, self.current_frame.segments
        n_prev = len(prev)
        targets = assignments.tolist() if hasattr(assignments, "tolist") else list(assignments)
        for prev_label in range(n_prev):
            target = targets[prev_label] - n_prev
            if target >= 0:
                prev[prev_label].status = target
                curr[target].status = prev_label
            else:
                prev[prev_label].status = "D"
        for curr_label in range(len(curr)):
            if targets[n_prev + curr_label] - n_prev == curr_label:
                curr[curr_label].status = "A"

    def link_matching_segments(self):
        """:133-152: a matched segment takes over (not copies) its predecessor's history list."""
        prev = self.cached_frame.segments
        for segment in self.current_frame.segments:
            if segment.status != "A":
                matched = prev[segment.status]
                history = matched.segment_history
                history.append(matched)
                segment.segment_history = history

    def check_for_events(self):
        """:154-176: vanished inside the chimney ROI after at least one match = a candidate swift entry."""
        for segment in self.cached_frame.segments:
            if segment.status != "D":
                continue
            pos = segment.centroid
            if self.roi_mask[int(pos[0]), int(pos[1])] != 255:
                continue
            if len(segment.segment_history) < 1:
                continue
            path = segment.segment_history
            path.append(segment)
            self.detected_events.append(path)

    def step(self, frame):
        """The six calls the counting loop makes per popped frame (__main__.py:87-92)."""
        self.set_current_frame(frame)
        self.store_assignments(apply_hungarian_algorithm(self.formulate_cost_matrix()))
        self.link_matching_segments()
        self.check_for_events()
        self.cache_current_frame()

    def step_window(self, frames):
        """step(frame) for every frame of `frames`, in order, as ONE library call (swk_track_window): the same cost matrices, the same
        assignments, the same events -- appended to detected_events as lists of the very Segment objects the frames carry -- and
        current_frame / cached_frame both the last frame afterwards.  An empty list is valid and changes nothing.

        Only the segments of an event of this window are touched (segment_history = the event's path, shared along it as the
        per-frame path leaves it; the vanished segment's status "D").  The `status` and `segment_history` of every other segment
        that is not on the cached frame are UNSPECIFIED after this call, and so is the `status` of the cached frame's segments (the
        next step overwrites it before anything reads it).  The segment_history of the cached frame's segments is made exact --
        lists shared along each chain and all -- as soon as step(), one of the six single calls or get_cached_frame() asks for it,
        so the two paths can be mixed freely.  Segments of earlier windows are kept only as long as a later event can still name
        them.

        A subclass (or an instance) that replaces step() or one of the six single calls expects to see every frame go through them:
        its windows are stepped per frame, which gives the same events.

        Raises TypeError where the per-frame path does (a current segment without a status, see the module's notes): the frames
        before that one are applied then, and current_frame is the failing frame.  IndexError when a vanished segment's centroid
        lies outside the ROI mask; the window is not applied then."""
        frames = list(frames)
        if not frames:
            return
        if self._per_frame_hooks():
            for frame in frames:
                self.step(frame)
            return
        native = self._native_state()
        per_frame = [fr.segments for fr in frames]
        flat = [c for segs in per_frame for s in segs for c in s.centroid]
        try:
            failed, done, first, min_live, offsets, ordinals = native.track_window([len(segs) for segs in per_frame], flat)
        except _lib.SwkError as exc:
            raise IndexError("a vanished segment's centroid lies outside the ROI mask (%s)" % exc)
        store, base = self._store, self._store_base
        if first != base + len(store):
            raise _lib.SwkError("the tracker's ordinals and the kept segments disagree")
        for segs in (per_frame if done == len(frames) else per_frame[:done]):
            store.extend(segs)
        for e in range(len(offsets) - 1):
            path = [store[o - base] for o in ordinals[offsets[e]:offsets[e + 1]]]
            for s in path:
                s.segment_history = path
            path[-1].status = "D"
            self.detected_events.append(path)
        if min_live > base:
            del store[:min_live - base]
            self._store_base = min_live
        if done:
            self.current_frame = self.cached_frame = self._native_frame = frames[done - 1]
        if failed:
            self._materialise()
            self.current_frame = frames[done]
            raise TypeError("list indices must be integers or slices, not NoneType")

    _SINGLE_CALLS = ("step", "set_current_frame", "formulate_cost_matrix", "store_assignments", "link_matching_segments",
                     "check_for_events", "cache_current_frame")

    def _per_frame_hooks(self):
        """True when step() or one of the six single calls is not SegmentTracker's own (a subclass's, or set on the instance)."""
        cls = type(self)
        if cls is SegmentTracker:
            return any(name in self.__dict__ for name in self._SINGLE_CALLS)
        return any(getattr(cls, name) is not getattr(SegmentTracker, name) or name in self.__dict__ for name in self._SINGLE_CALLS)

    def _native_state(self):
        """The library handle, holding the cached frame's state: imported from the segments' attributes unless the last thing that
        happened to this tracker was a step_window."""
        if self._native is None or self._native_mask is not self.roi_mask:
            self._native, self._native_mask, self._native_frame = _lib.Tracker(self.roi_mask), self.roi_mask, None
        if self._native_frame is None or self._native_frame is not self.cached_frame:
            segs = self.cached_frame.segments
            first = self._native.import_state(
                [c for s in segs for c in s.centroid], [len(s.segment_history) for s in segs],
                [c for s in segs for c in (s.segment_history[0].centroid if s.segment_history else (0.0, 0.0))])
            self._store = [m for s in segs for m in s.segment_history] + list(segs)
            self._store_base = first
            self._native_frame = self.cached_frame
        return self._native

    def _materialise(self):
        """segment_history of the cached frame's segments as per-frame stepping would have left it, from the chains the library
        holds: one list per chain, shared by the segment and every member of the chain."""
        frame, self._native_frame = self._native_frame, None
        if frame is not self.cached_frame:
            return
        _, _, offsets, chain = self._native.export_state()
        offsets, chain = offsets.tolist(), chain.tolist()
        store, base = self._store, self._store_base
        if len(offsets) - 1 != len(frame.segments):
            raise _lib.SwkError("the cached frame's segments changed behind the tracker")
        for k, segment in enumerate(frame.segments):
            history = [store[o - base] for o in chain[offsets[k]:offsets[k + 1]]]
            for member in history:
                member.segment_history = history
            segment.segment_history = history
        self._store = []
