"""The counting loop's options in combination (tests/test_pipeline_options_gpu.py, tests/test_pipeline_options_cpu.py): two small
shaken clips with their still twins, the option axes and a fixed pairwise covering array of runs over them, one runner that observes
everything a run hands on, and the helpers that compare two observations.  Host code: the package's GPU parts are imported inside
the functions that run something.

Clips.  stabilize_ref.scene_frames with small faint birds, turned into pictures that every kind of source hands out byte for byte
alike: the scene's grey becomes the luma plane (kept within 16..235), the chroma is one (U, V) pair for the whole picture -- a bluish
tint like the scene's own; the trained classifier keeps no segment of a colourless picture -- and the canonical BGR picture is what
the 4:2:0 conversion makes of the two.  That is a function of the pixel alone, so cutting a picture out of the scene and converting
it commute, and 4:2:0 subsampling of a flat chroma plane loses nothing.  The BGR array, the 4:4:4 file and the 4:2:0 stream of a clip
therefore hold the same video, and a run from any of them is compared with the baseline from the array.  Clip 0's regions come from
the chimney's corners (image_filtering.generate_regions on the first frame: what the command line does), clip 1's are given: an odd
origin and an odd width.

Observation of a run, per video: see run_case."""
import itertools
import os
import threading

import numpy as np

import stabilize_ref as ref

N = 21                                   # frames per window
MIN_SEG = (24, 24)
SEARCH = 8

# crop_region of clip 0 = what its corners give (asserted where the library runs); corners as the CLI's --corners take them
CLIPS = (dict(seed=9693, total=52, frame_hw=(110, 160), crop_region=[(31, 33), (125, 80)], corners=((40, 71), (116, 71))),
         dict(seed=9412, total=47, frame_hw=(100, 125), crop_region=[(21, 23), (104, 79)], corners=None))
CHROMA = (133, 122)                      # one (U, V) for the whole picture: 4:2:0 subsampling loses nothing; a bluish tint like the scene's
LUMA = "direct"
BIRDS = dict(birds=8, bird_len=(5, 8), bird_wid=(4, 6), contrast=(25, 40))
MIN_EVENTS_PLAIN, MIN_EVENTS_CLASSIFIED = 6, 1          # over both still twins: the thresholds of tests/test_track_window_gpu.py

AXES = (("source", ("array", "y4m444", "pipe420")),
        ("stabilize", (0, SEARCH)),
        ("classifier", ("none", "eval", "dropout")),
        ("shape_props", (False, True)),
        ("review", ("none", "plain", "full")),
        ("windows_per_call", (1, 2)),
        ("track_by_window", (False, True)),
        ("entry", ("single", "videos")))
AXIS_NAMES = tuple(name for name, _ in AXES)
DROPOUT_SEED = 3
REVIEW_FULL = dict(review_text=True, review_stages=("rpca", "labels"))


def _case(name, source, stabilize, classifier, shape_props, review, windows_per_call, track_by_window, entry, reader=None):
    return dict(name=name, source=source, stabilize=stabilize, classifier=classifier, shape_props=shape_props, review=review,
                windows_per_call=windows_per_call, track_by_window=track_by_window, entry=entry, reader=reader)


# The covering array: every pair of levels of two different axes occurs in some run (uncovered_pairs).  The first three are the
# all-on runs, the fourth has io_frames.PresegmentingReader between the StabilizingReader and the loop.
RUNS = (
    _case("all_on_serial", "pipe420", SEARCH, "dropout", True, "full", 1, True, "single"),
    _case("all_on_producer", "pipe420", SEARCH, "eval", True, "full", 2, True, "single"),
    _case("all_on_videos", "y4m444", SEARCH, "eval", True, "full", 2, True, "videos"),
    _case("presegmenting", "array", SEARCH, "eval", True, "none", 1, False, "single", reader="presegmenting"),
    _case("videos_plain_review", "array", 0, "none", False, "plain", 2, False, "videos"),
    _case("y4m444_nothing_on", "y4m444", 0, "none", False, "none", 1, True, "single"),
    _case("videos_pipe_dropout", "pipe420", 0, "dropout", False, "none", 2, False, "videos"),
    _case("pipe_stab_shape_review", "pipe420", SEARCH, "none", True, "plain", 1, True, "single"),
    _case("videos_eval_full_review", "array", 0, "eval", False, "full", 1, False, "videos"),
    _case("y4m444_dropout_shape_review", "y4m444", 0, "dropout", True, "plain", 1, False, "single"),
    _case("stab_full_review", "array", SEARCH, "none", False, "full", 1, True, "single"),
    _case("eval_plain_review", "array", 0, "eval", False, "plain", 1, False, "single"),
    _case("dropout_alone", "array", 0, "dropout", False, "none", 1, False, "single"),
    _case("videos_y4m444_stab_dropout", "y4m444", SEARCH, "dropout", False, "plain", 2, True, "videos"),
    _case("videos_pipe_eval_shape", "pipe420", 0, "eval", True, "plain", 2, False, "videos"),
)


def case_named(name):
    return next(c for c in RUNS if c["name"] == name)


def all_pairs():
    out = set()
    for (a, la), (b, lb) in itertools.combinations(AXES, 2):
        out |= {((a, x), (b, y)) for x in la for y in lb}
    return out


def uncovered_pairs(runs):
    """the pairs ((axis, level), (other axis, level)) that no run of `runs` holds; a level outside its axis is a ValueError"""
    levels = dict(AXES)
    seen = set()
    for run in runs:
        for name in AXIS_NAMES:
            if run[name] not in levels[name]:
                raise ValueError("%s: %s = %r is no level of that axis" % (run.get("name"), name, run[name]))
        seen |= {((a, run[a]), (b, run[b])) for a, b in itertools.combinations(AXIS_NAMES, 2)}
    return sorted(all_pairs() - seen, key=repr)


def baseline_case(classifier, windows_per_call, entry):
    """the still twin as a BGR array with every option off but the classifier level"""
    return _case("baseline_%s_w%d_%s" % (classifier, windows_per_call, entry), "array", 0, classifier, False, "none", windows_per_call, True, entry)


def baseline_key(case):
    return (case["classifier"], case["windows_per_call"], case["entry"])


def review_reference_case(case):
    """the run whose only options are the case's review level and classifier level, on the still twin.  Eval scores and the plain
    loop do not depend on how windows are batched (the baselines are asserted to agree); a dropout run keeps the case's batching."""
    wpc, entry = (case["windows_per_call"], case["entry"]) if case["classifier"] == "dropout" else (1, "single")
    return _case("review_%s_%s_w%d_%s" % (case["review"], case["classifier"], wpc, entry), "array", 0, case["classifier"], False,
                 case["review"], wpc, True, entry)


def shape_reference_case():
    return _case("shape_props_alone", "array", 0, "none", True, "none", 1, True, "single")


# ---- clips ------------------------------------------------------------------------------------------------------------------------
_clips = {}


def luma(frames, mapping="limited"):
    """luma of BGR pictures: "limited" 16 + grey * 219 // 255 (stabilize_ref.yuv_planes); "direct" the grey itself, kept in 16..235"""
    g = ref.gray(frames).astype(np.int32)
    return (16 + g * 219 // 255).astype(np.uint8) if mapping == "limited" else np.clip(g, 16, 235).astype(np.uint8)


def flat_chroma(shape_hw, chroma, uv=None):
    """(u, v) planes of one value each for a picture of that size in that chroma format"""
    H, W = shape_hw
    shape = (H, W) if chroma == "444" else ((H + 1) // 2, (W + 1) // 2)
    u, v = CHROMA if uv is None else uv
    return np.full(shape, u, np.uint8), np.full(shape, v, np.uint8)


def build_clip(spec):
    """dict: shaken, still (total, H, W, 3) BGR; y_shaken, y_still (total, H, W) the luma planes they were made from; jitter
    (total, 2) (jy, jx), frame 0 at (0, 0); frame_hw, crop_region, corners, total.  Read-only."""
    from swiftwatcher_amd.io_y4m import yuv420_rect_to_bgr
    hw = spec["frame_hw"]
    scene = ref.scene_frames(spec["seed"], spec["total"], hw, spec["crop_region"], **dict(BIRDS, **spec.get("scene", {})))
    y_scene = luma(scene, spec.get("luma", LUMA))
    Hs, Ws = y_scene.shape[1:]
    u, v = flat_chroma((Hs, Ws), "420", spec.get("chroma"))
    bgr_scene = np.stack([yuv420_rect_to_bgr(y, u, v, 0, Hs, 0, Ws) for y in y_scene])
    if spec.get("raw"):          # (a control: the scene's own pictures, which no file of a clip holds)
        bgr_scene = scene
    jitter = np.random.default_rng(spec["seed"] + 1).integers(-ref.JITTER, ref.JITTER + 1, size=(spec["total"], 2))
    jitter[0] = 0
    zero = np.zeros_like(jitter)
    out = dict(shaken=ref.cut(bgr_scene, jitter, hw), still=ref.cut(bgr_scene, zero, hw), y_shaken=ref.cut(y_scene, jitter, hw),
               y_still=ref.cut(y_scene, zero, hw), jitter=jitter)
    for a in out.values():
        a.setflags(write=False)
    out.update(frame_hw=hw, crop_region=[tuple(p) for p in spec["crop_region"]], corners=spec["corners"], total=spec["total"])
    return out


def clip(k):
    """build_clip(CLIPS[k]), cached"""
    if k not in _clips:
        _clips[k] = build_clip(CLIPS[k])
    return _clips[k]


_regions = {}


def regions(k):
    """(crop_region, roi_mask) of clip k: from the corners and the first frame where the clip has corners (the library's host code),
    else the lower three fifths of the crop region"""
    if k not in _regions:
        _regions[k] = build_regions(clip(k))
    return _regions[k]


def build_regions(c):
    if c["corners"] is not None:
        from swiftwatcher_amd import image_filtering as img
        crop_region, mask, _ = img.generate_regions(c["still"][0], c["corners"])
        crop_region = [tuple(int(v) for v in p) for p in crop_region]
        assert crop_region == c["crop_region"], "the corners give %s" % (crop_region,)
    else:
        (x0, y0), (x1, y1) = crop_region = c["crop_region"]
        mask = np.zeros((y1 - y0, x1 - x0), np.uint8)
        mask[(y1 - y0) * 2 // 5:, :] = 255
    return crop_region, mask


def write_y4m(path, planes, chroma):
    """the luma planes (count, H, W) with the flat chroma as an 8-bit file of that chroma format, 30 frames a second"""
    from swiftwatcher_amd.io_y4m import Y4MWriter
    H, W = planes.shape[1:]
    u, v = flat_chroma((H, W), chroma)
    with Y4MWriter(str(path), W, H, 30, chroma=chroma) as w:
        for y in planes:
            w.append(y, u, v)
    return str(path)


def y4m_path(workdir, k, twin, chroma):
    path = os.path.join(str(workdir), "clip%d_%s_%s.y4m" % (k, twin, chroma))
    if not os.path.exists(path):
        write_y4m(path, clip(k)["y_" + twin], chroma)
    return path


class _Pipe:
    """a file's bytes through an os.pipe: .source is the read end as an unbuffered binary file object"""

    def __init__(self, path):
        with open(path, "rb") as fh:
            data = fh.read()
        rd, wr = os.pipe()

        def feed():
            try:
                with os.fdopen(wr, "wb") as out:
                    out.write(data)
            except BrokenPipeError:
                pass

        self.thread = threading.Thread(target=feed, daemon=True)
        self.thread.start()
        self.source = os.fdopen(rd, "rb", buffering=0)

    def close(self):
        self.source.close()
        self.thread.join()


# ---- the runner -------------------------------------------------------------------------------------------------------------------
def shape_values(obj):
    """every attribute of image_filtering.SHAPE_PROPERTIES as the bytes of its float64 value(s)"""
    from swiftwatcher_amd import image_filtering as img
    return tuple((name, np.asarray(getattr(obj, name), dtype=np.float64).tobytes()) for name in img.SHAPE_PROPERTIES)


_spy = {}


def spy_classifier_class():
    """SegmentClassifier that notes every score it computes on the device (SpyClassifier.scores, in the order computed) and the boxes
    it removes: per Frame object (_removed) where it is handed frames, else in last_removed until the tracker takes the frame"""
    if "cls" not in _spy:
        from swiftwatcher_amd.segment_classification import SegmentClassifier

        class SpyClassifier(SegmentClassifier):
            scores = []
            active = None

            def _scores_device_unlocked(self, cut, keys=None):
                out = super()._scores_device_unlocked(cut, keys)
                SpyClassifier.scores.append(out[0].detach().cpu().numpy().copy())
                return out

            def classify_frames(self, frames):
                SpyClassifier.active = self
                before = [list(fr.segments) for fr in frames]
                super().classify_frames(frames)
                for fr, was in zip(frames, before):
                    kept = {id(s) for s in fr.segments}
                    fr._removed = [tuple(s.bbox) for s in was if id(s) not in kept]

            def __call__(self, segments):
                SpyClassifier.active = self
                kept = super().__call__(segments)
                ids = {id(s) for s in kept}
                self.last_removed = [tuple(s.bbox) for s in segments if id(s) not in ids]
                return kept

        _spy["cls"] = SpyClassifier
    return _spy["cls"]


def make_classifiers(golden_dir, workdir):
    """{"none": None, "eval": ..., "dropout": ...} of spy classifiers with the trained weights of tests/golden, and the path of the
    state_dict file they were loaded from (the CLI's --classify)"""
    import torch
    g = np.load(os.path.join(golden_dir, "classifier_model_pt.npz"))
    sd = {k[2:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("w:")}
    path = os.path.join(str(workdir), "model.pt")
    torch.save(sd, path)
    cls = spy_classifier_class()
    return {"none": None, "eval": cls(path), "dropout": cls(path, dropout_seed=DROPOUT_SEED)}, path


def segment_record(s):
    return (s.label, tuple(s.bbox), tuple(s.centroid), s.area)


def event_records(events):
    return [[(s.parent_frame_number,) + segment_record(s) for s in ev] for ev in events]


def event_shapes(events):
    """per event, per segment: shape_values, or None for a segment that raises the documented AttributeError"""
    out = []
    for ev in events:
        row = []
        for s in ev:
            try:
                row.append(shape_values(s))
            except AttributeError as exc:
                assert "no shape record" in str(exc), exc
                row.append(None)
        out.append(row)
    return out


class spies:
    """Context manager: pipeline.SegmentTracker, stabilize.StabilizingReader.__init__, _lib.Context.stabilize and
    segment_classification.SegmentClassifier replaced by their observing versions.  trackers: in the order made (one per video); made:
    the StabilizingReaders; calls: how often Context.stabilize ran."""

    def __init__(self, all_shapes=False):
        self.all_shapes = all_shapes          # note the shape attributes of every segment the tracker sees, not of the events' alone

    def __enter__(self):
        from swiftwatcher_amd import _lib, pipeline, segment_classification, stabilize
        all_shapes = self.all_shapes
        self.trackers, self.made, self.calls = trackers, made, calls = [], [], []
        cls = spy_classifier_class()
        cls.scores, cls.active = [], None
        self.cls = cls

        def note(tracker, frame):
            clf = cls.active
            if frame.frame_number >= 0:
                tracker.seen[frame.frame_number] = [segment_record(s) for s in frame.segments]
                if all_shapes:
                    for s in frame.segments:
                        tracker.shape_table[(frame.frame_number, tuple(s.bbox))] = shape_values(s)
                if clf is not None:
                    gone = frame.__dict__.get("_removed")
                    tracker.removed[frame.frame_number] = sorted(gone if gone is not None else clf.last_removed)
            if clf is not None:
                clf.last_removed = []

        class Spy(pipeline.SegmentTracker):
            def __init__(self, *a, **k):
                super().__init__(*a, **k)
                self.seen, self.removed, self.shape_table = {}, {}, {}
                trackers.append(self)

            def set_current_frame(self, frame):
                note(self, frame)
                super().set_current_frame(frame)

            def step_window(self, frames):
                for frame in frames:
                    note(self, frame)
                return super().step_window(frames)

        init, call = stabilize.StabilizingReader.__init__, _lib.Context.stabilize

        def spy_init(reader, *a, **k):
            made.append(reader)
            init(reader, *a, **k)

        def spy_call(ctx, *a, **k):
            calls.append(1)
            return call(ctx, *a, **k)

        self._saved = [(pipeline, "SegmentTracker", pipeline.SegmentTracker), (stabilize.StabilizingReader, "__init__", init),
                       (_lib.Context, "stabilize", call), (segment_classification, "SegmentClassifier", segment_classification.SegmentClassifier)]
        pipeline.SegmentTracker = Spy
        stabilize.StabilizingReader.__init__ = spy_init
        _lib.Context.stabilize = spy_call
        segment_classification.SegmentClassifier = cls
        return self

    def __exit__(self, *exc):
        for owner, name, value in self._saved:
            setattr(owner, name, value)

    def observations(self, results, review_paths, classified, stabilized):
        """results: (count, events) per video -> {"videos": [...], "scores", "stabilize_calls", "readers_made"}"""
        videos = []
        for v, (count, events) in enumerate(results):
            tracker = self.trackers[v]
            review = None
            if review_paths[v] is not None:
                with open(review_paths[v], "rb") as fh:
                    review = fh.read()
            shapes = event_shapes(events)
            videos.append(dict(segments=tracker.seen, count=int(count), events=event_records(events), shapes=shapes,
                               removed=tracker.removed if classified else None, review=review,
                               shifts=dict(self.made[v].shifts) if stabilized else None, raw_events=events,
                               shape_table=tracker.shape_table if self.all_shapes else None))
        return dict(videos=videos, scores=list(self.cls.scores), stabilize_calls=len(self.calls), readers_made=len(self.made))


def run_case(case, workdir, classifiers, clips=(0, 1), all_shapes=False):
    """One run of the counting loop as `case` says, on the clips given (each after the other through count_swifts, all in one call
    through count_swifts_videos) -> the observation: per video the segments the tracker saw per frame number (label, bbox, centroid,
    area), the count, the events as tuples, the event segments' shape attributes (None where unbound), the boxes the classifier
    removed per frame number (the kept ones are the segments the tracker saw), the review file's bytes, the StabilizingReader's
    shifts; per run the score arrays in the order computed, the calls of Context.stabilize and the StabilizingReaders made.
    all_shapes: also shape_table, (frame number, bbox) -> shape attributes of every segment the tracker saw."""
    from swiftwatcher_amd import pipeline
    twin = case.get("twin") or ("shaken" if case["stabilize"] else "still")          # ("twin": the shaken clip as it is, for a control)
    classifier = classifiers[case["classifier"]]
    tag = case["name"]
    review_paths = [os.path.join(str(workdir), "%s_review%d.y4m" % (tag, k)) if case["review"] != "none" else None for k in clips]
    for p in review_paths:
        if p is not None and os.path.exists(p):
            os.remove(p)
    opened = []

    def source(k):
        if case["source"] == "array":
            return list(clip(k)[twin])
        if case["source"] == "y4m444":
            return y4m_path(workdir, k, twin, "444")
        pipe = _Pipe(y4m_path(workdir, k, twin, "420"))
        opened.append(pipe)
        return pipe.source

    kw = dict(windows_per_call=case["windows_per_call"], track_by_window=case["track_by_window"], classifier=classifier)
    if case["shape_props"]:
        kw["shape_props"] = True
    if case["review"] == "full":
        kw.update(REVIEW_FULL)
    try:
        with spies(all_shapes) as spy:
            if case["entry"] == "videos":
                assert case["reader"] is None
                results = pipeline.count_swifts_videos([source(k) for k in clips], regions=[regions(k) for k in clips], in_flight=2,
                                                       stabilize=case["stabilize"],
                                                       reviews=review_paths if case["review"] != "none" else None, **kw)
            else:
                results = []
                for k, review in zip(clips, review_paths):
                    crop_region, mask = regions(k)
                    if case["reader"] == "presegmenting":
                        results.append(_count_presegmented(case, k, source(k), review, kw))
                    else:
                        results.append(pipeline.count_swifts(source(k), crop_region, mask, stabilize=case["stabilize"], review=review, **kw))
            return spy.observations(results, review_paths, classifier is not None, bool(case["stabilize"]))
    finally:
        for pipe in opened:
            pipe.close()


def _count_presegmented(case, k, frames, review, kw):
    """count_swifts over io_frames.PresegmentingReader, which reads and segments two windows ahead of the loop; with stabilize it
    wraps the StabilizingReader (the loop is then told nothing of the stabilization: it gets a reader of a stabilized video)"""
    from swiftwatcher_amd import pipeline
    from swiftwatcher_amd.io_frames import ArrayReader, PresegmentingReader
    from swiftwatcher_amd.stabilize import StabilizingReader
    crop_region, mask = regions(k)
    inner = ArrayReader(frames, fps=30.0)
    if case["stabilize"]:
        inner = StabilizingReader(inner, crop_region, case["stabilize"], MIN_SEG)
    reader = PresegmentingReader(inner, crop_region, queue_size=N, windows=2)
    try:
        return pipeline.count_swifts(reader, crop_region, mask, review=review, **kw)
    finally:
        reader.close()


# ---- comparing observations -------------------------------------------------------------------------------------------------------
def check_tracking(got, want, label=""):
    """equal segments per frame number, an equal count and equal events"""
    assert sorted(got["segments"]) == sorted(want["segments"]), "%s: frame numbers differ" % label
    for k in sorted(want["segments"]):
        assert got["segments"][k] == want["segments"][k], "%s: segments of frame %d: %s, expected %s" % (label, k, got["segments"][k], want["segments"][k])
    assert got["count"] == want["count"], "%s: count %d, expected %d" % (label, got["count"], want["count"])
    assert len(got["events"]) == len(want["events"]), "%s: %d events, expected %d" % (label, len(got["events"]), len(want["events"]))
    for e, (a, b) in enumerate(zip(got["events"], want["events"])):
        assert a == b, "%s: event %d: %s, expected %s" % (label, e, a, b)


def check_removed(got, want, label=""):
    """the boxes the classifier removed, per frame number (the kept ones are check_tracking's segments)"""
    assert got["removed"] is not None and want["removed"] is not None, "%s: no classifier was seen" % label
    assert sorted(got["removed"]) == sorted(want["removed"]), "%s: frame numbers differ" % label
    for k in sorted(want["removed"]):
        assert got["removed"][k] == want["removed"][k], "%s: removed boxes of frame %d: %s, expected %s" % (label, k, got["removed"][k], want["removed"][k])


def score_rows(scores):
    """the score arrays of a run as one (T, 2) array, in the order computed"""
    return np.concatenate([np.asarray(s).reshape(-1, 2) for s in scores]) if scores else np.zeros((0, 2), np.float32)


def check_scores(got, want, ordered=True, label=""):
    """bit equality of the scores; ordered=False (another batching): the same set of rows"""
    a, b = score_rows(got), score_rows(want)
    assert a.dtype == b.dtype, "%s: %s scores, expected %s" % (label, a.dtype, b.dtype)
    if ordered:
        assert a.shape == b.shape, "%s: %d scores, expected %d" % (label, len(a), len(b))
        bad = np.nonzero((a.view(np.uint32) != b.view(np.uint32)).any(axis=1))[0] if a.dtype == np.float32 else np.nonzero((a != b).any(axis=1))[0]
        assert not len(bad), "%s: %d of %d score rows differ, first at %d: %s, expected %s" % (label, len(bad), len(a), bad[0], a[bad[0]], b[bad[0]])
    else:
        rows = lambda x: sorted({r.tobytes() for r in x})          # noqa: E731
        assert rows(a) == rows(b), "%s: the sets of score rows differ" % label


def check_shapes(got, want, label=""):
    """every shape attribute of every event segment, exactly"""
    assert len(got["shapes"]) == len(want["shapes"]), "%s: %d events, expected %d" % (label, len(got["shapes"]), len(want["shapes"]))
    for e, (ga, wa) in enumerate(zip(got["shapes"], want["shapes"])):
        assert len(ga) == len(wa), "%s: event %d has %d segments, expected %d" % (label, e, len(ga), len(wa))
        for i, (g, w) in enumerate(zip(ga, wa)):
            assert g is not None and w is not None, "%s: event %d segment %d carries no shape record" % (label, e, i)
            for (name, a), (_, b) in zip(g, w):
                assert a == b, "%s: event %d segment %d: %s differs" % (label, e, i, name)


def check_shapes_in(got, table, label=""):
    """every shape attribute of every event segment equals the entry of `table` ((frame number, bbox) -> shape_values) for it: a
    classifier relabels and thins the segments out, the frame and the box stay"""
    assert len(got["shapes"]) == len(got["events"])
    for e, (row, event) in enumerate(zip(got["shapes"], got["events"])):
        for i, (g, seg) in enumerate(zip(row, event)):
            key = (seg[0], seg[2])
            assert g is not None, "%s: event %d segment %d carries no shape record" % (label, e, i)
            assert key in table, "%s: event %d segment %d: no segment of frame %d has the box %s" % (label, e, i, seg[0], seg[2])
            for (name, a), (_, b) in zip(g, table[key]):
                assert a == b, "%s: event %d segment %d: %s differs" % (label, e, i, name)


def check_unbound(obs, label=""):
    """without shape_props every event segment raises the documented AttributeError"""
    for e, row in enumerate(obs["shapes"]):
        assert all(v is None for v in row), "%s: event %d carries shape attributes" % (label, e)


def check_review(got, want, label=""):
    """the review files, byte for byte"""
    assert got["review"] is not None and want["review"] is not None, "%s: no review file" % label
    a, b = got["review"], want["review"]
    assert len(a) == len(b), "%s: review file of %d bytes, expected %d" % (label, len(a), len(b))
    if a != b:
        x, y = np.frombuffer(a, np.uint8), np.frombuffer(b, np.uint8)
        bad = np.nonzero(x != y)[0]
        raise AssertionError("%s: %d bytes of the review file differ, first at offset %d" % (label, len(bad), bad[0]))


def check_shifts(obs, jitter, label=""):
    """every frame's shift is (-jy, -jx) (the frame one past the end is the last one again)"""
    shifts = obs["shifts"]
    assert shifts is not None, "%s: no StabilizingReader" % label
    total = len(jitter)
    assert set(range(total)) <= set(shifts), "%s: frames without a shift" % label
    for k in sorted(shifts):
        jy, jx = jitter[min(k, total - 1)]
        assert tuple(shifts[k][:2]) == (-jy, -jx), "%s: frame %d shifted by %s, expected %s" % (label, k, shifts[k][:2], (-jy, -jx))


def windows_of(total):
    """queue-fuls the loop reads of a clip of `total` frames (the frame one past the end is served once)"""
    return -(-total // N)
