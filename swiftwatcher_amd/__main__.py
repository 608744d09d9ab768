"""python -m swiftwatcher_amd SOURCE [SOURCE ...] (--corners X1,Y1,X2,Y2 | --attributes FILE) [--start N] [--end N]
       [--classify WEIGHTS] [--out DIR] [--shape-props] [--review PATH [--review-text] [--review-stages LIST]] [--windows-per-call K]
       [--stabilize [S] [--stabilize-subpel]] [--device D]

The reference's main() (__main__.py:13-53) without its UI: every SOURCE -- a .y4m file, or "-" for a YUV4MPEG2 stream on standard
input (`ffmpeg -i evening.mp4 -f yuv4mpegpipe - | python -m swiftwatcher_amd - --corners 812,640,1105,642`) -- is counted by
pipeline.count_swifts, one after the other.  The chimney's corners come from --corners, from --attributes (a file in the format of
the reference's attributes.json, ui.py:180-194), or, for a file, from <parent>/<stem>/attributes.json (:29-31).  Per source one JSON
line goes to standard output: {"source", "frames", "events", "count"}; --out DIR gets the reference's result tables
(io_data.export_results, :49-50; under DIR/<stem> when several sources are given).  --review PATH writes the review video of the
count (review.py: the crop region as a 4:2:0 .y4m with segments, removed segments, ROI mask and events drawn in; PATH/<stem>.y4m when
several sources are given).  PATH may be a FIFO (`--review fifo & ffmpeg -i fifo out.mp4`), not "-": standard output carries the
JSON lines.  --review-text (with --review only) writes the tables' keys into every frame of the review: a status line "F000123
00:00:04.104 S03 R01 E007" (frame number, timestamp, segments, boxes the classifier removed, events so far) and the number #k of
every event shown, k its row in the events table.  --review-stages rpca,thresh,labels (with --review only; combines with
--review-text) puts those stage images of every frame beside it as captioned panels: keys gray rpca bilateral thresh opened labels.
--shape-props measures every segment's shape on the GPU (pipeline.count_swifts' shape_props=True) and, with --out DIR, also writes
DIR/segments_shape.csv: one row per segment of every event (SHAPE_CSV_COLUMNS).
--stabilize [S] (S = 8 without a value, at most 16) is for shaken footage: every frame is cut at the integer shift of up to S pixels
that matches it best to the video's first frame (stabilize.StabilizingReader) before it is segmented; with --out DIR it also writes
DIR/stabilization.csv, one row per frame (frame_number, dy, dx, sad, sad_unshifted), and the JSON line gains
"stabilize": {"search": S, "moved_frames": k, "max_shift": m}.
--stabilize-subpel (with --stabilize) adds the quarter-pixel stage: every frame is resampled at the best of the 25 quarter-pixel
shifts around the integer one.  stabilization.csv then has three more columns -- shift_y, shift_x: the total shift in pixels with
two decimal places (-1.25), and sad_subpel -- and the "stabilize" object gains "subpel": true and "fractional_frames": k.
--deinterlace {bob,frame,weave} counts an interlaced source (header tags It / Ib; without the option it is refused by name, and a
progressive source with it is) on the pictures of its fields (deinterlace.DeinterlacingReader): bob = every field, at twice the frame
rate ("frames" is then twice the stored count), frame = each frame's first field, weave = the stored frames as they are;
--deinterlace-spatial interpolates without the temporal clamp.  The JSON line gains "deinterlace": {"mode": m, "field_order": "t" or
"b", "stored_frames": n, "frames": k}."""
import argparse
import json
import os
import sys


def parse_corners(text):
    """"X1,Y1,X2,Y2" -> ((x1, y1), (x2, y2))"""
    parts = text.replace(" ", "").split(",")
    try:
        x1, y1, x2, y2 = (int(p) for p in parts)
    except ValueError:
        raise ValueError("corners are four integers X1,Y1,X2,Y2 (got %r)" % text)
    return ((x1, y1), (x2, y2))


def corners_from_file(path):
    """ui.py:180-194: the "corners" entry of an attributes.json, [[x1, y1], [x2, y2]], as integer pairs."""
    with open(path) as fh:
        c = json.load(fh)["corners"]
    return ((int(c[0][0]), int(c[0][1])), (int(c[1][0]), int(c[1][1])))


def default_attributes(source):
    """<parent>/<stem>/attributes.json of a video file (__main__.py:29-30)."""
    return os.path.join(os.path.dirname(os.path.abspath(source)), os.path.splitext(os.path.basename(source))[0], "attributes.json")


def _review_path(text):
    if text == "-":
        raise argparse.ArgumentTypeError("standard output carries the JSON lines: give a file's or a FIFO's path")
    return text


def _stage_list(text):
    from .review import stage_keys
    try:
        return stage_keys(text)
    except ValueError as exc:
        raise argparse.ArgumentTypeError(str(exc))


def _search_range(text):
    try:
        s = int(text)
    except ValueError:
        raise argparse.ArgumentTypeError("the search range is a number of pixels (got %r)" % text)
    if not 1 <= s <= 16:
        raise argparse.ArgumentTypeError("the search range is 1..16 pixels (got %d)" % s)
    return s


def build_parser():
    p = argparse.ArgumentParser(prog="python -m swiftwatcher_amd", description="Count chimney swifts in YUV4MPEG2 videos on the MI355X.")
    p.add_argument("sources", nargs="+", metavar="SOURCE", help="a .y4m file, or - for a YUV4MPEG2 stream on standard input")
    where = p.add_mutually_exclusive_group()
    where.add_argument("--corners", metavar="X1,Y1,X2,Y2", help="the two corners of the chimney's top edge, in pixels")
    where.add_argument("--attributes", metavar="FILE", help='a JSON file with "corners": [[x1, y1], [x2, y2]]')
    p.add_argument("--start", type=int, default=0, metavar="N", help="first frame counted")
    p.add_argument("--end", type=int, default=0, metavar="N", help="frame count to stop at (0: the whole video)")
    p.add_argument("--classify", metavar="WEIGHTS", help="filter segments with the classifier of this state_dict file")
    p.add_argument("--out", metavar="DIR", help="write the result tables (CSV) here")
    p.add_argument("--shape-props", action="store_true", help="measure the segments' shapes; with --out also write segments_shape.csv")
    p.add_argument("--review", type=_review_path, metavar="PATH", help="write a review video (.y4m) of the count here")
    p.add_argument("--review-text", action="store_true", help="with --review: draw frame number, time, counts and event numbers into it")
    p.add_argument("--review-stages", type=_stage_list, default=(), metavar="LIST",
                   help="with --review: stage images shown as panels beside every frame, e.g. rpca,thresh,labels")
    p.add_argument("--stabilize", type=_search_range, nargs="?", const=8, default=0, metavar="S",
                   help="stabilize shaken footage: search shifts of up to S pixels per frame (8 without a value); with --out also write "
                        "stabilization.csv")
    p.add_argument("--stabilize-subpel", action="store_true",
                   help="with --stabilize: refine every frame's shift to a quarter pixel and resample it there")
    p.add_argument("--deinterlace", choices=("bob", "frame", "weave"), default=None,
                   help="count an interlaced source on the pictures of its fields: bob = every field at twice the frame rate, frame = "
                        "each frame's first field, weave = the stored frames as they are")
    p.add_argument("--deinterlace-spatial", action="store_true", help="with --deinterlace: spatial interpolation only, no temporal clamp")
    p.add_argument("--windows-per-call", type=int, default=1, metavar="K", help="queue-fuls segmented per GPU call")
    p.add_argument("--device", type=int, default=0, metavar="D", help="GPU index")
    return p


def plan(argv):
    """(parsed arguments, [(source, corners), ...]); usage errors leave through the parser (exit status 2)."""
    parser = build_parser()
    args = parser.parse_args(argv)
    if args.sources.count("-") > 1:
        parser.error("standard input (-) can be given once")
    if args.start < 0 or args.end < 0 or args.windows_per_call < 1:
        parser.error("--start and --end are frame numbers, --windows-per-call is at least 1")
    if args.review_text and not args.review:
        parser.error("--review-text needs --review PATH")
    if args.review_stages and not args.review:
        parser.error("--review-stages needs --review PATH")
    if args.stabilize_subpel and not args.stabilize:
        parser.error("--stabilize-subpel needs --stabilize")
    if args.deinterlace_spatial and not args.deinterlace:
        parser.error("--deinterlace-spatial needs --deinterlace")
    shared = None
    try:
        if args.corners is not None:
            shared = parse_corners(args.corners)
        elif args.attributes is not None:
            shared = corners_from_file(args.attributes)
    except (OSError, ValueError, KeyError, IndexError, TypeError) as exc:
        parser.error("no corners: %s" % exc)
    jobs = []
    for source in args.sources:
        corners = shared
        if corners is None:
            if source == "-":
                parser.error("standard input (-) needs --corners or --attributes")
            found = default_attributes(source)
            if not os.path.isfile(found):
                parser.error("%s needs --corners, --attributes or %s" % (source, found))
            try:
                corners = corners_from_file(found)
            except (OSError, ValueError, KeyError, IndexError, TypeError) as exc:
                parser.error("no corners in %s: %s" % (found, exc))
        jobs.append((source, corners))
    return args, jobs


SHAPE_CSV_COLUMNS = ("event", "frame_number", "label", "area", "centroid_r", "centroid_c", "orientation", "eccentricity",
                     "major_axis_length", "minor_axis_length", "perimeter", "extent", "euler_number")


def shape_rows(events):
    """One row (SHAPE_CSV_COLUMNS) per segment of every event; event = the event's index in the list, as in the events table."""
    rows = []
    for k, event in enumerate(events):
        for s in event:
            rows.append((k, s.parent_frame_number, s.label, s.area, s.centroid[0], s.centroid[1], s.orientation, s.eccentricity,
                         s.major_axis_length, s.minor_axis_length, s.perimeter, s.extent, s.euler_number))
    return rows


def write_shape_csv(path, events):
    """segments_shape.csv: floats written with repr, so that reading them back gives the attributes bit for bit."""
    import csv
    with open(path, "w", newline="") as fh:
        w = csv.writer(fh)
        w.writerow(SHAPE_CSV_COLUMNS)
        for row in shape_rows(events):
            w.writerow([repr(float(x)) if isinstance(x, float) else int(x) for x in row])


def main(argv=None):
    args, jobs = plan(argv)
    from . import event_classification as ec
    from . import pipeline
    from .io_data import export_results
    from .io_y4m import open_y4m
    classifier = None
    if args.classify:
        from .segment_classification import SegmentClassifier
        classifier = SegmentClassifier(args.classify, device="cuda:%d" % args.device)
    for source, corners in jobs:
        opened = None
        try:
            reader = opened = open_y4m(source, args.start, args.end, **({"interlaced": True} if args.deinterlace else {}))
            if args.deinterlace:
                from .deinterlace import DeinterlacingReader
                reader = DeinterlacingReader(reader, None, args.deinterlace, not args.deinterlace_spatial, device=args.device)
        except (OSError, ValueError) as exc:
            if hasattr(opened, "close"):             # (the source was opened and then refused: a progressive header with --deinterlace)
                opened.close()
            print("swiftwatcher_amd: cannot read %s: %s" % (source, exc), file=sys.stderr)
            return 1
        stem = "stdin" if source == "-" else os.path.splitext(os.path.basename(source))[0]
        review = args.review
        if review and len(jobs) > 1:
            os.makedirs(review, exist_ok=True)
            review = os.path.join(review, stem + ".y4m")
        counted = reader
        try:
            if args.stabilize:                                                     # (the regions of :62-63 here: the wrapper needs the crop region)
                from . import image_filtering as img
                from .stabilize import StabilizingReader
                crop_region, roi_mask, _ = img.generate_regions(reader.read_frame(0, increment=False), corners)
                counted = StabilizingReader(reader, crop_region, args.stabilize, device=args.device,
                                            **({"subpel": True} if args.stabilize_subpel else {}))
                regions = dict(crop_region=crop_region, roi_mask=roi_mask)
            else:
                regions = dict(corners=corners)
            count, events = pipeline.count_swifts(counted, classifier=classifier, device=args.device,
                                                  windows_per_call=args.windows_per_call, review=review or None, review_text=args.review_text,
                                                  review_stages=args.review_stages, **({"shape_props": True} if args.shape_props else {}),
                                                  **regions)
            frames, fps, first, last = reader.total_frames, reader.fps, reader.start_frame, reader.end_frame
        except (OSError, ValueError) as exc:
            print("swiftwatcher_amd: cannot read %s: %s" % (source, exc), file=sys.stderr)
            return 1
        finally:
            if hasattr(reader, "close"):
                reader.close()
        if args.out and events:                                                    # (__main__.py:40-50; without events there is no table)
            out_dir = args.out if len(jobs) == 1 else os.path.join(args.out, stem)
            with _stdout_to_stderr():                                              # (export_results prints its progress line)
                export_results(out_dir, ec.classify_events(events), fps, first, last)
            if args.shape_props:
                write_shape_csv(os.path.join(out_dir, "segments_shape.csv"), events)
        line = {"source": source, "frames": int(frames), "events": len(events), "count": int(count)}
        if args.stabilize:
            from .stabilize import summary, write_csv
            sub = (counted.subshifts,) if args.stabilize_subpel else ()
            if args.out:                                                           # (also for a video without events: the shifts are about frames)
                out_dir = args.out if len(jobs) == 1 else os.path.join(args.out, stem)
                os.makedirs(out_dir, exist_ok=True)
                write_csv(os.path.join(out_dir, "stabilization.csv"), counted.shifts, *sub)
            line["stabilize"] = summary(counted.shifts, args.stabilize, *sub)
        if args.deinterlace:
            line["deinterlace"] = reader.fields
        print(json.dumps(line), flush=True)
    return 0


class _stdout_to_stderr:
    def __enter__(self):
        self._saved, sys.stdout = sys.stdout, sys.stderr

    def __exit__(self, *exc):
        sys.stdout = self._saved


if __name__ == "__main__":
    sys.exit(main())
