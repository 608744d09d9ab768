"""The reference's per-video loop (swift_counting_algorithm, __main__.py:56-100) over the MI355X segment path:
read queue_size frames -> preprocess_queue + segment_queue (one GPU call) -> per popped frame: optional
classifier, tracker step -> events -> swift count.  The regions come from the chimney corners like in the reference
(generate_regions on the first frame, __main__.py:62-63) or are handed in; the reader is anything with the
reference FrameReader's read_frame / get_n_frames / total_frames (swiftwatcher_amd.io_frames.ArrayReader for decoded
frames)."""
from .data_structures import FrameQueue, segment_window_groups, segment_windows
from .io_frames import ArrayReader
from .segment_tracking import SegmentTracker, apply_hungarian_algorithm
from . import event_classification as ec
from . import image_filtering as img


def swift_counting_algorithm(reader, crop_region=None, roi_mask=None, queue_size=21, classifier=None, min_seg_size=(24, 24),
                             device=0, keep_stages=False, windows_per_call=1, corners=None, export_dir=None, params=None,
                             track_by_window=True, review=None, review_text=False, review_stages=(), shape_props=False, stabilize=0,
                             stabilize_subpel=False, deinterlace=None, deinterlace_temporal=True):
    """Same call order as __main__.py:62-100.  corners = ((x1, y1), (x2, y2)) of the chimney's top edge: crop region
    and ROI mask are then generated from the video's first frame (:62-63) instead of being passed in.  Returns the tracker's detected events (lists of Segment objects,
    the structure the reference hands to event classification).  windows_per_call > 1 reads that many queue-fuls
    ahead and segments (and classifies) them in one GPU call each; the tracker still sees the frames one by one in
    the reference's order, so the events are the same.  track_by_window (windows_per_call > 1 only): the tracker takes each
    window's frames in one library call (SegmentTracker.step_window) instead of one step per frame -- the same events; False is the
    per-frame path.  params: a _lib.default_params(...) struct for the segment path (bilateral
    diameter and sigmas, threshold, ...); None = the reference's values.  review: a path (a file's or a FIFO's) or a review.ReviewWriter:
    every window's frames are written there as a 4:2:0 video of the crop region with the segments, the boxes the classifier removed,
    the ROI mask and the events drawn in (review.py); a writer made here from a path is closed when the count ends.  Counts and
    events are the same with and without it.  review_text: a writer made here from a path also writes the status line and the event
    numbers (ReviewWriter's text=True); a ReviewWriter handed in carries its own setting.  review_stages: names of stage images
    (rpca, thresh, labels, ...: ReviewWriter's stages=) that a writer made here from a path shows as panels beside every frame; the
    segment path then keeps those images on the GPU, where the writer reads them.  shape_props: every segment (those of the returned
    events among them) also answers the shape properties of image_filtering.ShapeMeasures -- orientation, eccentricity, axis lengths,
    perimeter, moments, ... -- from one more GPU call per window over its label planes; counts and events are the same with and
    without it, and without it nothing is different (no extra call, no label planes).  stabilize: a search range S of 1..16 pixels
    (True = 8) for shaken footage: the reader is wrapped in a stabilize.StabilizingReader, which hands out every frame cut at the
    integer shift that matches it best to the video's first frame (one more GPU call per window, swk_stabilize_u8); everything else
    sees a stabilized video.  A reader that is a StabilizingReader already is taken as it is.  0 (the default): nothing is different.
    stabilize_subpel=True (with stabilize; ValueError without): the quarter-pixel stage after the integer search
    (swk_stabilize_subpel_u8 in swk_stabilize_u8's place): every frame is resampled at the best of the 25 quarter-pixel shifts
    around the integer one.  False (the default): nothing is different.  deinterlace: "bob", "frame" or "weave" for an interlaced
    source (a reader of io_y4m opened with interlaced=...: YUV4MPEG2 tags It / Ib): the reader is wrapped in a
    deinterlace.DeinterlacingReader, which hands out the fields as whole pictures -- "bob": every field, at twice the frame rate;
    "frame": each frame's first field; "weave": the stored frames as they are (one more GPU call per window, swk_yuv_deinterlace;
    none for "weave"); the regions are then made from its first picture, and stabilize works on its pictures.  deinterlace_temporal
    =False: spatial interpolation only.  A source whose header says progressive is a ValueError.  None (the default): nothing is
    different."""
    if deinterlace:
        from .deinterlace import wrap
        reader = wrap(reader, deinterlace, None, deinterlace_temporal, min_seg_size, device)
    if corners is not None:
        first_frame = reader.read_frame(0, increment=False)                        # :62
        crop_region, roi_mask, _ = img.generate_regions(first_frame, corners)      # :63
    if crop_region is None or roi_mask is None:
        raise ValueError("either corners or crop_region + roi_mask are needed")
    reader = _stabilized(reader, crop_region, stabilize, min_seg_size, device, params, stabilize_subpel)
    if hasattr(reader, "set_region"):                # a reader of a pipe (io_y4m.Y4MStreamReader): it keeps only what this loop reads
        reader.set_region(crop_region, min_seg_size)
    tracker = SegmentTracker(roi_mask)
    own_review = None
    if review is not None and not hasattr(review, "write_window"):
        from .review import ReviewWriter
        review = own_review = ReviewWriter(review, crop_region, roi_mask, getattr(reader, "fps", 30.0), device=device, text=review_text,
                                           stages=review_stages)
    try:
        return _counting_loop(reader, crop_region, roi_mask, queue_size, classifier, min_seg_size, device, keep_stages, windows_per_call,
                              export_dir, params, track_by_window, tracker, review, shape_props)
    finally:
        if own_review is not None:
            own_review.close()


def _stabilized(reader, crop_region, stabilize, min_seg_size, device, params, subpel=False):
    """The reader itself, or with stabilize = S > 0 a stabilize.StabilizingReader around it (grey as the segment path's params say);
    subpel: with its quarter-pixel stage."""
    if not stabilize:
        if subpel:
            raise ValueError("stabilize_subpel refines the integer search of stabilize=S: it needs stabilize")
        return reader
    from .stabilize import StabilizingReader, search_range
    if isinstance(reader, StabilizingReader):
        return reader
    kw = {"gray_mode": params.gray_mode} if params is not None else {}
    if subpel:
        kw["subpel"] = True
    return StabilizingReader(reader, crop_region, search_range(stabilize), min_seg_size, device=device, **kw)


def _counting_loop(reader, crop_region, roi_mask, queue_size, classifier, min_seg_size, device, keep_stages, windows_per_call, export_dir,
                   params, track_by_window, tracker, review, shape_props=False):
    """swift_counting_algorithm once the regions, the tracker and the review writer exist."""
    seen = 0                                         # events already handed to the review
    stages = _review_stages([review])                # the stage images the review shows: kept on the GPU by the segment path
    keep = {"stages": stages} if stages else {}      # (without them the segmenters are called as they always were)
    if shape_props:
        keep["shape_props"] = True
        if hasattr(reader, "shape_props"):           # a reader that segments ahead (io_frames.PresegmentingReader): its windows carry the records
            reader.shape_props = True
    if classifier is not None and getattr(reader, "_classifier_hint", False) is None:
        import weakref
        reader._classifier_hint = weakref.ref(classifier)          # a reader that segments ahead scores every batch for this classifier
    if windows_per_call > 1:
        if hasattr(reader, "ahead"):                 # a reader that reads ahead (io_roi_stream, io_y4m's of a pipe): as far as one GPU call takes
            reader.ahead = max(reader.ahead, windows_per_call)
        # producer thread: reads ahead and segments (GPU call and array copies release the GIL);
        # this thread: classifier and the strictly sequential tracker
        import queue as _queue
        import threading
        ready = _queue.Queue(maxsize=2)

        def produce():
            try:
                ahead = 0
                while ahead < reader.total_frames:
                    windows = []
                    while len(windows) < windows_per_call and ahead < reader.total_frames:
                        triple = reader.get_n_frames(n=queue_size)                  # :73 (pads with null frames)
                        windows.append(triple)
                        ahead += sum(1 for k in triple[1] if k >= 0)                # null frames are not counted (:146-147)
                    ready.put(segment_windows(windows, crop_region, min_seg_size, device=device, params=params, classifier=classifier, **keep))
                ready.put(None)
            except BaseException as exc:                                            # surfaces in the consumer
                ready.put(exc)

        worker = threading.Thread(target=produce, daemon=True)
        worker.start()
        while True:
            batches = ready.get()
            if batches is None:
                break
            if isinstance(batches, BaseException):
                raise batches
            removed = {}
            if classifier is not None:
                flat = [fr for popped in batches for fr in popped]
                before = [list(fr.segments) for fr in flat] if review is not None else None          # (the boxes the classifier removes)
                classifier.classify_frames(flat)
                if review is not None:
                    from .review import removed_boxes
                    removed = {id(fr): gone for fr, gone in zip(flat, removed_boxes(before, flat))}
            for popped in batches:
                _track(tracker, popped, track_by_window)
                if review is not None:
                    review.write_window(popped, [removed.get(id(fr)) for fr in popped], tracker.detected_events[seen:])
                    seen = len(tracker.detected_events)
        worker.join()
        return tracker.detected_events
    queue = FrameQueue(queue_size, device=device, params=params, keep_stages=keep_stages or bool(stages),
                       **({"shape_props": True} if shape_props else {}))
    while queue.frames_processed < reader.total_frames:
        frames, numbers, stamps = reader.get_n_frames(n=queue.maxlen)          # :73 (pads with null frames)
        queue.push_list_of_frames(frames, numbers, stamps)                     # :74
        queue.preprocess_queue(crop_region, None)                              # :77
        queue.segment_queue(min_seg_size, crop_region)                         # :78
        popped, removed = [], []
        while not queue.is_empty():                                            # :81
            frame = queue.pop_frame()
            popped.append(frame)
            if classifier is not None:                                         # :84-85 (--classify)
                before = frame.segments
                frame.segments = classifier(frame.segments)
                if review is not None:
                    kept = {id(s) for s in frame.segments}
                    removed.append([tuple(s.bbox) for s in before if id(s) not in kept])
            tracker.set_current_frame(frame)                                   # :87-92, call by call
            cost_matrix = tracker.formulate_cost_matrix()
            tracker.store_assignments(apply_hungarian_algorithm(cost_matrix))
            tracker.link_matching_segments()
            tracker.check_for_events()
            tracker.cache_current_frame()
            if export_dir is not None:                                         # :94-96 (--export): needs keep_stages=True (the "crop" image)
                frame.export_segments(min_seg_size, crop_region, export_dir)
        if review is not None:
            review.write_window(popped, removed if classifier is not None else None, tracker.detected_events[seen:])
            seen = len(tracker.detected_events)
    return tracker.detected_events


def _review_stages(reviews):
    """The stage keys that the given review writers (or None) show, each once."""
    return tuple(dict.fromkeys(key for rv in reviews if rv is not None for key in getattr(rv, "stages", ())))


def _track(tracker, popped, by_window):
    """One window's popped frames (oldest first) to the tracker: in one call where it is asked for and the tracker has one (anything
    with the reference's step() alone is stepped per frame)."""
    if by_window and hasattr(tracker, "step_window"):
        tracker.step_window(popped)
    else:
        for frame in popped:
            tracker.step(frame)


def count_swifts(frames, crop_region=None, roi_mask=None, fps=30.0, params=None, review=None, review_text=False, review_stages=(), **kw):
    """Decoded frames (oldest first) -> (swift count, events).  frames may also be a reader (get_n_frames / read_frame / total_frames,
    e.g. io_y4m.Y4MReader: its fps holds) or anything io_y4m.open_y4m opens: the path of a .y4m file (any format it reads), or a
    YUV4MPEG2 stream of unknown length -- "-" (standard input), a FIFO's path, a file descriptor, a binary file object (a pipe from a
    decoder: proc.stdout).  Regions either explicit or from corners=...; params, review (a path or a
    review.ReviewWriter: the review video of the count), review_text (text in a review made from a path) and review_stages (stage
    images as panels in it) as in swift_counting_algorithm; so is shape_props=True (among **kw): the events' segments then carry the
    shape properties; and stabilize=S (among **kw; True = 8): shaken footage is brought back onto its first frame before it is
    segmented, with stabilize_subpel=True to a quarter pixel; and deinterlace="bob" | "frame" | "weave" (among **kw, with
    deinterlace_temporal): an interlaced source is counted on the pictures of its fields -- without it an interlaced file is refused
    by name, and with it a progressive one is."""
    opened = None
    if _is_video_source(frames):
        from .io_y4m import open_y4m
        frames = opened = open_y4m(frames, **({"interlaced": True} if kw.get("deinterlace") else {}))
    reader = frames if hasattr(frames, "get_n_frames") else ArrayReader(frames, fps=fps)
    try:
        events = swift_counting_algorithm(reader, crop_region, roi_mask, params=params, review=review, review_text=review_text,
                                          review_stages=review_stages, **kw)
    finally:
        if opened is not None and hasattr(opened, "close"):
            opened.close()
    return ec.count_swifts(events), events


def _is_video_source(video):
    """What io_y4m.open_y4m opens: a path, "-" (standard input), a file descriptor, a binary file object."""
    if isinstance(video, (str, bytes)) or hasattr(video, "__fspath__"):
        return True
    if isinstance(video, bool) or hasattr(video, "get_n_frames"):
        return False
    return isinstance(video, int) or hasattr(video, "readinto") or hasattr(video, "read")


def plan_calls(items, n, pad_factor=2.0):
    """Which groups of windows share one swk_batch_run_groups call.  items: (key, P, nwin) per group, P = ROI pixels.  The library
    runs the IALM of a call over planes zero-padded to the call's largest P, so a call holding windows of very different sizes moves
    more bytes than separate calls would: a call is closed when padding to its largest P would make the IALM's elements more than
    pad_factor times the windows' own.  Groups with P < n run at their own P inside any call (no padding) and join the first one.
    Returns a list of calls, each a list of keys; largest ROIs first."""
    big = sorted((it for it in items if it[1] >= n), key=lambda it: -it[1])
    small = [it[0] for it in items if it[1] < n]
    calls, cur, pmax, real, wins = [], [], 0, 0, 0
    for key, P, nwin in big:
        if cur:
            padded = max(pmax, P) * (wins + nwin)
            if padded > pad_factor * (real + P * nwin):
                calls.append(cur)
                cur, pmax, real, wins = [], 0, 0, 0
        cur.append(key)
        pmax, real, wins = max(pmax, P), real + P * nwin, wins + nwin
    if cur:
        calls.append(cur)
    if small:
        if calls:
            calls[0].extend(small)
        else:
            calls.append(small)
    return calls


def schedule_videos(readers, sizes, segment, consume, in_flight=4, windows_per_call=1, queue_size=21, pad_factor=2.0):
    """The in-flight loop of count_swifts_videos, without the GPU: `in_flight` videos are open at a time; every round takes the next
    windows_per_call queue-fuls (reader.get_n_frames, padded with null frames past the end) of each open video, plan_calls splits
    them into calls, segment(groups) -> per group the popped frame lists runs each call (groups = [(video index, windows)]), and
    consume(video index, popped lists) gets them in each video's own order.  A video whose frames are all read leaves after its round
    and the next one takes its place.  sizes[v] = ROI pixels of video v (for the planner).  Returns the calls made, as lists of
    (video index, windows in the group)."""
    pending = list(range(len(readers)))[::-1]
    open_, read, log = [], {}, []
    while pending or open_:
        while pending and len(open_) < in_flight:
            v = pending.pop()
            open_.append(v)
            read[v] = 0
        taken = {}
        for v in open_:
            r = readers[v]
            windows = []
            while len(windows) < windows_per_call and read[v] < r.total_frames:
                triple = r.get_n_frames(n=queue_size)
                windows.append(triple)
                read[v] += sum(1 for k in triple[1] if k >= 0)          # null frames are not counted
            if windows:
                taken[v] = windows
        items = [(v, sizes[v], len(w)) for v, w in taken.items()]
        for call in plan_calls(items, queue_size, pad_factor):
            groups = [(v, taken[v]) for v in sorted(call, key=open_.index)]
            log.append([(v, len(w)) for v, w in groups])
            for (v, _), popped in zip(groups, segment(groups)):
                consume(v, popped)
        open_ = [v for v in open_ if read[v] < readers[v].total_frames]
    return log


def count_swifts_videos(videos, regions=None, corners=None, in_flight=4, windows_per_call=1, classifier=None, queue_size=21,
                        min_seg_size=(24, 24), device=0, fps=30.0, pad_factor=2.0, params=None, track_by_window=True, reviews=None,
                        review_text=False, review_stages=(), shape_props=False, stabilize=0, stabilize_subpel=False, deinterlace=None,
                        deinterlace_temporal=True):
    """count_swifts over a list of videos (the reference's loop over its video list, __main__.py:21), several videos at a time on one
    GPU: `in_flight` videos are open, each with its own SegmentTracker, and every GPU call (swk_batch_run_groups) segments the next
    windows_per_call queue-fuls of each of them at once, every video at its own crop region.  Each tracker still sees its video's
    frames one by one in the reference's order, so every count and event list equals count_swifts on that video alone.
    track_by_window: each tracker takes a window's frames in one library call (SegmentTracker.step_window); False steps per frame.
    videos: readers (read_frame / get_n_frames / total_frames), decoded frame arrays (oldest first) or what io_y4m.open_y4m opens (a
    .y4m path, "-", a FIFO, a descriptor, a binary file object); regions: per video
    (crop_region, roi_mask), or corners: per video the chimney's top edge (the regions then come from its first frame, :62-63).
    reviews: per video a path, a review.ReviewWriter or None -- that video's review video (swift_counting_algorithm's review=);
    review_text: the writers made here from paths also write text (its review_text=); review_stages: and show these stage images as
    panels (its review_stages=).  shape_props: as swift_counting_algorithm's; one shape call per group of a GPU call, since the
    groups' geometries differ.  stabilize and stabilize_subpel: as swift_counting_algorithm's, one StabilizingReader per video.
    deinterlace: as swift_counting_algorithm's for every video, or one value per video (None for a progressive one), with
    deinterlace_temporal; one DeinterlacingReader per interlaced video.
    Returns [(count, events), ...] in input order."""
    from .io_y4m import open_y4m
    modes = list(deinterlace) if isinstance(deinterlace, (list, tuple)) else [deinterlace] * len(videos)
    if len(modes) != len(videos):
        raise ValueError("one deinterlace mode (or None) per video")
    readers, opened = [], []                         # (what is opened here is closed again when the count is done)
    try:
        for v, mode in zip(videos, modes):
            if _is_video_source(v):
                r = open_y4m(v, **({"interlaced": True} if mode else {}))
                if hasattr(r, "close"):
                    opened.append(r)
            else:
                r = v if hasattr(v, "get_n_frames") else ArrayReader(v, fps=fps)
            if mode:
                from .deinterlace import wrap
                r = wrap(r, mode, None, deinterlace_temporal, min_seg_size, device)
            readers.append(r)
        return _count_videos(readers, regions, corners, in_flight, windows_per_call, classifier, queue_size, min_seg_size, device,
                             pad_factor, params, track_by_window, reviews, review_text, review_stages, shape_props, stabilize,
                             stabilize_subpel)
    finally:
        for r in opened:
            r.close()


def _count_videos(readers, regions, corners, in_flight, windows_per_call, classifier, queue_size, min_seg_size, device, pad_factor, params,
                  track_by_window=True, reviews=None, review_text=False, review_stages=(), shape_props=False, stabilize=0,
                  stabilize_subpel=False):
    """count_swifts_videos over readers."""
    if regions is None:
        if corners is None:
            raise ValueError("either regions or corners are needed")
        regions = []
        for r, c in zip(readers, corners):
            crop_region, roi_mask, _ = img.generate_regions(r.read_frame(0, increment=False), c)
            regions.append((crop_region, roi_mask))
    if len(regions) != len(readers):
        raise ValueError("one region pair per video")
    if stabilize_subpel and not stabilize:
        raise ValueError("stabilize_subpel refines the integer search of stabilize=S: it needs stabilize")
    if stabilize:
        readers = [_stabilized(r, crop_region, stabilize, min_seg_size, device, params, stabilize_subpel)
                   for r, (crop_region, _) in zip(readers, regions)]
    for r, (crop_region, _) in zip(readers, regions):
        if hasattr(r, "set_region"):                 # a reader of a pipe (io_y4m.Y4MStreamReader): it keeps only what this loop reads
            r.set_region(crop_region, min_seg_size)
            if hasattr(r, "ahead"):                  # (a deinterlacing reader offers set_region over files too, which do not read ahead)
                r.ahead = max(r.ahead, windows_per_call)
    trackers = [SegmentTracker(mask) for _, mask in regions]
    sizes = [(cr[1][0] - cr[0][0]) * (cr[1][1] - cr[0][1]) for cr, _ in regions]
    reviews = list(reviews) if reviews is not None else [None] * len(readers)
    if len(reviews) != len(readers):
        raise ValueError("one review (or None) per video")
    own_reviews = []
    try:
        for v, rv in enumerate(reviews):
            if rv is not None and not hasattr(rv, "write_window"):
                from .review import ReviewWriter
                reviews[v] = ReviewWriter(rv, regions[v][0], regions[v][1], getattr(readers[v], "fps", 30.0), device=device, text=review_text,
                                          stages=review_stages)
                own_reviews.append(reviews[v])
        seen = [0] * len(readers)                    # events already handed to each video's review
        removed = {}                                 # id(frame) -> the boxes the classifier removed from it, until its window is written

        stages = _review_stages(reviews)             # the stage images the reviews show: kept on the GPU by the segment path
        keep = {"stages": stages} if stages else {}  # (without them the segmenter is called as it always was)
        if shape_props:
            keep["shape_props"] = True

        def segment(groups):
            out = segment_window_groups([(w, regions[v][0]) for v, w in groups], min_seg_size, device=device, params=params,
                                        classifier=classifier, **keep)
            if classifier is not None:
                flat = [fr for per in out for popped in per for fr in popped]
                watched = [fr for (v, _), per in zip(groups, out) if reviews[v] is not None for popped in per for fr in popped]
                before = [list(fr.segments) for fr in watched]
                classifier.classify_frames(flat)
                if watched:
                    from .review import removed_boxes
                    removed.update((id(fr), gone) for fr, gone in zip(watched, removed_boxes(before, watched)))
            return out

        def consume(v, popped_lists):
            for popped in popped_lists:
                _track(trackers[v], popped, track_by_window)
                if reviews[v] is not None:
                    events = trackers[v].detected_events
                    reviews[v].write_window(popped, [removed.pop(id(fr), None) for fr in popped], events[seen[v]:])
                    seen[v] = len(events)

        schedule_videos(readers, sizes, segment, consume, in_flight=in_flight, windows_per_call=windows_per_call, queue_size=queue_size,
                        pad_factor=pad_factor)
    finally:
        for rv in own_reviews:
            rv.close()
    return [(ec.count_swifts(t.detected_events), t.detected_events) for t in trackers]
