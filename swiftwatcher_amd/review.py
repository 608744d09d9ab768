"""A review video of a count: the crop region's frames as an 8-bit 4:2:0 YUV4MPEG2 file (ffmpeg / mpv open it) with what was
counted drawn in -- the segments, the segments the classifier threw away, the ROI mask, and the tracker's events.  The reference
shows its users the same with `--export`, one overlay PNG per segment (data_structures.py:65-113); here a window's frames are
composed and converted by one GPU call (swk_render_review, include/swk.h) and leave with one device-to-host copy and one file
write.  pipeline.swift_counting_algorithm / count_swifts / count_swifts_videos feed a writer through review= / reviews=.

With text=True (review_text=True there, --review-text on the command line) every frame also carries the keys of the count's tables
as text, drawn by the same call (swk_render_review_labels, the library's 5 x 7 font: space, 0-9, A-Z and # : . - + / = %): a status
line with the frame number, the timestamp and the segment, removed-box and event counts, and the number #k of every event shown --
row k of the events table.

With stages=("rpca", "thresh", "labels") (review_stages= there, --review-stages on the command line) every frame becomes a mosaic:
the composed frame, then one panel per stage image of the same video frame -- the u8 planes swk_batch_run writes -- each with a
caption, converted by the same GPU call (swk_render_review_panels) from where the planes lie on the GPU."""
import bisect
import math

import numpy as np

from . import _lib
from ._lib import panel_layout
from .data_structures import STAGE_KEYS
from .io_y4m import FRAME_MARK, Y4MWriter

STYLE_SEGMENT, STYLE_REJECTED, STYLE_EVENT, STYLE_MASK, STYLE_TEXT, STYLE_PLATE = 1, 2, 3, 4, 5, 6
# (b, g, r, fill_alpha, line_alpha), alphas 0..256
DEFAULT_STYLES = ((0, 255, 0, 32, 256),          # 1 segments: green outline, faint green fill
                  (0, 0, 255, 0, 160),           # 2 segments the classifier removed: red outline, no fill
                  (0, 255, 255, 0, 256),         # 3 events: yellow frame border and plus signs
                  (255, 128, 0, 40, 0),          # 4 ROI mask: light blue tint
                  (255, 255, 255, 0, 256),       # 5 text ink: white
                  (0, 0, 0, 160, 0))             # 6 text plate: black, 160 / 256
STATUS_CELLS = 33                                # the status line's length while no field has widened
LABEL_BYTES = 32                                 # a label's text (swk_review_label)
DEFAULT_STAGE_GAIN = {"gray": 1, "rpca": 4, "bilateral": 4, "thresh": 4, "opened": 4, "labels": 1}          # (labels: a palette, no gain)
_STAGE_OF_NAME = {name: key for key, name in STAGE_KEYS.items()}
_CHARSET = frozenset(b" 0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ#:.-+/=%")


def stamp_text(timestamp):
    """A frame's timestamp as the status line shows it: HH:MM:SS.mmm from strftime where the timestamp has it (milliseconds cut, not
    rounded); else its string, upper-cased and cut to 12 bytes, with bytes outside the font's character set replaced by spaces."""
    if hasattr(timestamp, "strftime"):
        return timestamp.strftime("%H:%M:%S.%f")[:12]
    raw = str(timestamp).upper().encode("ascii", "replace")[:12]
    return bytes(b if b in _CHARSET else 0x20 for b in raw).decode("ascii")


def status_text(frame_number, timestamp, segments, removed, events):
    """The status line: "F%06d %s S%02d R%02d E%03d" (fields widen when the number needs it)."""
    return "F%06d %s S%02d R%02d E%03d" % (frame_number, stamp_text(timestamp), segments, removed, events)


def text_scale_for(width, height, border):
    """The default text scale of a width x height review: the largest at which the status line fits between the borders and takes no
    more than an eighth of the height, 1..4."""
    return max(1, min(4, (width - 2 * border) // (6 * STATUS_CELLS + 1), (height // 8) // 9))


def stage_keys(stages):
    """The stage keys (gray rpca bilateral thresh opened labels) of names given as keys or as Frame.processed_frames names
    (grayscale RPCA bilateral thresh_15 opened cc_labeling), in the order given; repeats stay.  An unknown name is a ValueError."""
    if isinstance(stages, str):
        stages = [part for part in stages.replace(" ", "").split(",") if part]
    out = []
    for name in stages:
        if name in STAGE_KEYS:
            out.append(name)
        elif name in _STAGE_OF_NAME:
            out.append(_STAGE_OF_NAME[name])
        else:
            raise ValueError("unknown stage %r (one of %s)" % (name, " ".join(STAGE_KEYS)))
    return tuple(out)


def stage_caption(key, gain):
    """A stage panel's caption: the key in capitals, with the gain where it is not 1 -- "RPCA X4", "LABELS"."""
    return key.upper() if key == "labels" or gain == 1 else "%s X%d" % (key.upper(), gain)


def default_stage_cols(height, width, cells):
    """Cells per mosaic row: a crop wider than high (chimney crops are about 2:1) stacks its cells vertically, any other lays them
    side by side."""
    return 1 if width > height else cells


def centroid_pixel(centroid):
    """(row, column) of the pixel a mark is drawn at: the centroid's coordinates rounded half up."""
    return int(math.floor(centroid[0] + 0.5)), int(math.floor(centroid[1] + 0.5))


class ReviewWriter:
    """ReviewWriter(path, crop_region, roi_mask, fps).write_window(popped_frames, rejected, new_events) per window, close() at the end
    (or use it as a context manager).  path may be a FIFO's: `ffmpeg -i fifo out.mp4` reads it while the count runs.

    Every frame whose frame number is >= 0 becomes one output frame of the crop region's size (null padding frames are not
    written).  Drawn, in the library's layer order (include/swk.h):
      * the ROI mask (roi_mask != 0) tinted in style 4;
      * a box in style 1 for every segment of frame.segments, in list order, then a box in style 2 for every box of the frame's
        `rejected` list (the boxes the classifier removed), in list order; boxes are the segments' bbox (r0, c0, r1, c1), half-open;
      * for every event whose frames include this one, in the order the tracker found them: a plus sign (arm MARK_ARM pixels) in
        style 3 at every centroid of the event's path (centroid_pixel: rounded half up), and a border of BORDER pixels in style 3.
        An event shows on frame event[-1].parent_frame_number + 1 -- the frame on which the tracker noticed that the segment had
        vanished -- and the event_hold - 1 frames after it, into the next windows where needed; where those frames are never written
        (null frames, the end of the video) it is dropped.

    Default palette, BGR (b, g, r, fill_alpha, line_alpha; alpha 256 = opaque, 0 = nothing):
      1 segment          (0, 255, 0, 32, 256)      green outline, faint fill
      2 rejected         (0, 0, 255, 0, 160)       red outline
      3 event            (0, 255, 255, 0, 256)     yellow border and plus signs
      4 ROI mask         (255, 128, 0, 40, 0)      light blue tint
      5 text ink         (255, 255, 255, 0, 256)   white
      6 text plate       (0, 0, 0, 160, 0)         black, 160 / 256
    styles= replaces it (at least four rows; six with text=True).  Output is 8-bit 4:2:0 only, the crop region only.

    text=True adds labels (layer 5, after the border; include/swk.h), at scale text_scale (1..8; None: text_scale_for, 2 at 424 x 212):
      * a status line, status_text: "F000123 00:00:04.104 S03 R01 E007" -- frame number, timestamp (stamp_text), S = len(frame.segments),
        R = boxes the classifier removed on this frame, E = events handed to the writer so far whose first shown frame
        (event[-1].parent_frame_number + 1) is at or before this frame number.  Style 5 on plate 6, ink origin at row
        height - BORDER - 8 scale, column BORDER + scale: the bottom-left corner, over the chimney.  A line of more than 32 bytes is
        split into consecutive labels on the same row, 6 scale 32 pixels apart (their plates overlap by one unit).
      * for every event shown on the frame, after the status line and in the events' order: "#k" in style 3 on plate 6, k the event's
        1-based ordinal in the order the writer received events (its index in tracker.detected_events plus 1), with its ink origin
        MARK_ARM + 2 scale below and right of the event's last centroid pixel, then moved up / left and then down / right so that the
        label's rectangle (rows [r - scale, r + 8 scale), columns [c - scale, c + 6 scale len)) lies inside the border; where the
        frame is too small for that, its top / left side does.
    The character set has no lower case, and the two positions are fixed.

    stages=(names) makes every output frame a mosaic (_lib.panel_layout): cell 0 is the frame above, unchanged; cell k the k-th
    named stage image of the same video frame -- names are stage keys (gray rpca bilateral thresh opened labels) or
    Frame.processed_frames names, in any order, repeats allowed.  A gray stage is shown as min(255, v * gain), gain from stage_gain
    (a dict by key) over DEFAULT_STAGE_GAIN (gray 1, the others 4: the rpca image is dark by construction, the threshold that
    follows it is 15); labels in the library's palette (_lib.review_label_palette, 0 = black).  stage_layers picks the layers drawn
    on the panels too (bit 0..3: mask, boxes, marks, border; default 14: all but the mask's tint).  Every panel carries a caption
    (stage_caption: "RPCA X4", "LABELS") in style 5 on plate 6 at text_scale, ink origin at row and column BORDER + scale -- so
    stages needs six styles.  stage_cols: cells per row (None: default_stage_cols -- 1 for a crop wider than high, else all cells
    in one row).  height / width stay the crop's; frame_height / frame_width are the written frames'.  The planes come from the
    frames: where a window's written frames carry one _lib.DevicePlanes (Frame.stage_planes; FrameQueue(keep_stages=True),
    segment_windows(stages=...)) they are read on the GPU where they lie, else Frame.processed_frames[name] is stacked on the host
    and uploaded.  The grid is fixed, the stages are the u8 ones only (no A / E float planes)."""

    MARK_ARM = 4
    BORDER = 3

    def __init__(self, path, crop_region, roi_mask, fps, device=0, styles=None, event_hold=15, text=False, text_scale=None, stages=(),
                 stage_gain=None, stage_cols=None, stage_layers=14):
        (x0, y0), (x1, y1) = crop_region
        self.crop_region = [(int(x0), int(y0)), (int(x1), int(y1))]
        self.height, self.width = int(y1) - int(y0), int(x1) - int(x0)
        self.roi_mask = np.ascontiguousarray(roi_mask, np.uint8)
        if self.roi_mask.shape != (self.height, self.width):
            raise ValueError("roi_mask must have the crop region's size (%d, %d)" % (self.height, self.width))
        self.styles = tuple(tuple(int(x) for x in row) for row in (styles if styles is not None else DEFAULT_STYLES))
        if len(self.styles) < 4 or any(len(row) != 5 for row in self.styles):
            raise ValueError("styles holds at least four rows (b, g, r, fill_alpha, line_alpha)")
        if event_hold < 1:
            raise ValueError("event_hold is at least 1 frame")
        self.text = bool(text)
        if self.text and len(self.styles) < 6:
            raise ValueError("text=True needs six styles (5: the text's ink, 6: its plate)")
        self.text_scale = int(text_scale) if text_scale is not None else text_scale_for(self.width, self.height, self.BORDER)
        if not 1 <= self.text_scale <= 8:
            raise ValueError("text_scale is 1..8")
        self.stages = stage_keys(stages)
        if self.stages and len(self.styles) < 6:
            raise ValueError("stages need six styles (5: the captions' ink, 6: their plate)")
        if len(self.stages) > _lib.MAX_PANELS:
            raise ValueError("at most %d stage panels" % _lib.MAX_PANELS)
        unknown = set(stage_gain or ()) - set(STAGE_KEYS)
        if unknown:
            raise ValueError("stage_gain is a dict by stage key (unknown: %s)" % ", ".join(sorted(unknown)))
        self.stage_gain = dict(DEFAULT_STAGE_GAIN, **{k: int(v) for k, v in (stage_gain or {}).items()})
        if any(not 1 <= g <= 255 for g in self.stage_gain.values()):
            raise ValueError("a stage gain is 1..255")
        self.stage_layers = int(stage_layers)
        if not 0 <= self.stage_layers <= 15:
            raise ValueError("stage_layers is 0..15 (bit 0..3: mask, boxes, marks, border)")
        cells = 1 + len(self.stages)
        self.stage_cols = int(stage_cols) if stage_cols is not None else default_stage_cols(self.height, self.width, cells)
        if not 1 <= self.stage_cols <= _lib.MAX_PANEL_COLS:
            raise ValueError("stage_cols is 1..%d" % _lib.MAX_PANEL_COLS)
        self.frame_height, self.frame_width = self.height, self.width
        if self.stages:
            self.frame_height, self.frame_width, self.cell_origins = panel_layout(self.height, self.width, cells, self.stage_cols)
        self.device, self.event_hold = device, int(event_hold)
        self.frames = 0
        self._pending = []               # events still to be shown: (first frame number, last frame number, ((row, column), ...), ordinal)
        self._received = 0               # events received so far: the next event's ordinal is this + 1
        self._firsts = []                # the first shown frame of every event received, ascending (the status line's E)
        self._shown = []                 # of the last plan_window: per written frame (events counted so far, ((ordinal, last point), ...))
        self._dev = self._dev_bytes = 0
        self._host = None
        hc, wc = (self.frame_height + 1) // 2, (self.frame_width + 1) // 2
        self._luma, self._chroma = self.frame_height * self.frame_width, hc * wc
        self._frame_bytes = len(FRAME_MARK) + self._luma + 2 * self._chroma
        self._writer = Y4MWriter(path, self.frame_width, self.frame_height, fps)

    # ---- what is drawn (no GPU): the render call's arguments for one window ----
    def plan_window(self, popped_frames, rejected=None, new_events=()):
        """(frames to write, boxes, marks, frame_style) of one window: the Frame objects whose number is >= 0, and the overlay as
        swk_render_review takes it, `frame` counting the written frames.  Takes the new events in and forgets those that are over."""
        for event in new_events:
            first = int(event[-1].parent_frame_number) + 1
            self._received += 1
            self._pending.append((first, first + self.event_hold - 1, tuple(centroid_pixel(s.centroid) for s in event), self._received))
            bisect.insort(self._firsts, first)
        rejected = rejected if rejected is not None else [()] * len(popped_frames)
        frames, boxes, marks, frame_style = [], [], [], []
        self._shown = []
        for frame, gone in zip(popped_frames, rejected):
            if frame.frame_number < 0:
                continue
            k = len(frames)
            frames.append(frame)
            boxes.extend((k,) + tuple(int(v) for v in s.bbox) + (STYLE_SEGMENT,) for s in frame.segments)
            boxes.extend((k,) + tuple(int(v) for v in bbox) + (STYLE_REJECTED,) for bbox in (gone or ()))
            style, shown = 0, []
            for first, last, points, ordinal in self._pending:
                if first <= frame.frame_number <= last:
                    style = STYLE_EVENT
                    marks.extend((k, r, c, STYLE_EVENT) for r, c in points)
                    shown.append((ordinal, points[-1]))
            frame_style.append(style)
            self._shown.append((bisect.bisect_right(self._firsts, frame.frame_number), tuple(shown)))
        if frames:
            newest = max(f.frame_number for f in frames)
            self._pending = [ev for ev in self._pending if ev[1] > newest]
        return frames, boxes, marks, frame_style

    def plan_labels(self, plan):
        """The labels of the window plan_window has just planned (plan = its four-tuple), as swk_render_review_labels takes them:
        tuples (frame, r, c, style, plate, scale, text), per written frame the status line's labels, then the shown events' numbers."""
        frames, boxes = plan[0], plan[1]
        removed = [0] * len(frames)
        for box in boxes:
            if box[5] == STYLE_REJECTED:
                removed[box[0]] += 1
        s, labels = self.text_scale, []
        for k, (frame, (counted, shown)) in enumerate(zip(frames, self._shown)):
            line = status_text(frame.frame_number, getattr(frame, "timestamp", ""), len(frame.segments), removed[k], counted)
            for at in range(0, len(line), LABEL_BYTES):
                labels.append((k, self.height - self.BORDER - 8 * s, self.BORDER + s + 6 * s * at, STYLE_TEXT, STYLE_PLATE, s,
                               line[at:at + LABEL_BYTES]))
            for ordinal, (row, col) in shown:
                text = "#%d" % ordinal
                r = max(min(row + self.MARK_ARM + 2 * s, self.height - self.BORDER - 8 * s), self.BORDER + s)
                c = max(min(col + self.MARK_ARM + 2 * s, self.width - self.BORDER - 6 * s * len(text)), self.BORDER + s)
                labels.append((k, r, c, STYLE_EVENT, STYLE_PLATE, s, text))
        return labels

    def plan_panels(self, frames):
        """The panels of a window's written frames, as _lib.Context.render_review_panels takes them.  Device path: all frames carry
        the same DevicePlanes (Frame.stage_planes = (planes, index)), it holds every stage asked for and the indices step by a
        constant -- the panels then name that memory (the k-th popped frame of a queue of n has index n - 1 - k: a negative frame
        stride from the oldest frame's plane).  Host path: processed_frames[name] of every frame, stacked."""
        s, at = self.text_scale, self.BORDER + self.text_scale
        held = [getattr(f, "stage_planes", None) for f in frames]
        device = None
        if all(h is not None for h in held):
            planes, first = held[0]
            step = held[1][1] - first if len(held) > 1 else 0
            if (all(h[0] is planes and h[1] == first + k * step for k, h in enumerate(held)) and (planes.Hc, planes.Wc) == (self.height, self.width)
                    and all(key in planes.stages for key in self.stages)):
                device = (planes, first, step)
        panels = []
        for key in self.stages:
            gain = self.stage_gain[key]
            if device is not None:
                planes, first, step = device
                image = planes.Hc * planes.Wc
                plane = {"ptr": planes.pointer(key) + first * image, "frame_stride": step * image, "row_stride": planes.Wc, "mem": _lib.MEM_DEVICE}
            else:
                plane = np.stack([np.asarray(f.processed_frames[STAGE_KEYS[key]], np.uint8) for f in frames])
            panels.append({"plane": plane, "kind": "labels" if key == "labels" else "gray", "gain": gain, "layers": self.stage_layers,
                           "caption": (at, at, STYLE_TEXT, STYLE_PLATE, s, stage_caption(key, gain))})
        return panels, (device[0] if device is not None else None)

    def _render(self, frames, boxes, marks, frame_style, labels=None):
        """The window's frames composed and converted on the GPU: a uint8 array of len(frames) * frame bytes, every frame as the file
        holds it (the FRAME mark, then the Y, U and V planes), in page-locked memory.  labels: None, or the window's labels."""
        from .data_structures import stack_frames
        ctx = _lib.default_context(self.device)
        stack, (rx, ry), (Hc, Wc), backwards = stack_frames([f.frame for f in frames], self.crop_region, (0, 0), ctx.staging, self.device)
        if (Hc, Wc) != (self.height, self.width):
            raise ValueError("the crop region leaves the frame")
        if backwards:
            stack = stack[::-1]
        F, fb, mark = len(frames), self._frame_bytes, len(FRAME_MARK)
        if self._dev_bytes < F * fb:
            self._free()
            self._dev, self._dev_bytes = ctx.device_alloc(F * fb + 8), F * fb
            self._host = _lib.pinned_empty((F * fb,), np.uint8, device=self.device)
        base = self._dev + 8 - mark          # the first luma row on an 8-byte boundary: rows of a width that is a multiple of 8 leave as 8-byte stores
        dst = _lib.Yuv420Dst(y=base + mark, u=base + mark + self._luma, v=base + mark + self._luma + self._chroma,
                             mem=_lib.MEM_DEVICE, layout=_lib.YUV_I420, y_row_stride=self.frame_width, y_frame_stride=fb,
                             c_row_stride=(self.frame_width + 1) // 2, c_frame_stride=fb)
        extra = {} if labels is None else {"labels": labels}          # (without text: the call as it always was)
        render = ctx.render_review
        if self.stages:
            panels, held = self.plan_panels(frames)                   # (held: the planes stay alive until the call has returned)
            render, extra["panels"], extra["cols"] = ctx.render_review_panels, panels, self.stage_cols
        render(stack, boxes=boxes, marks=marks, frame_style=frame_style, mask=self.roi_mask, styles=self.styles,
               mask_style=STYLE_MASK, mark_arm=self.MARK_ARM, border=self.BORDER, rect=(rx, ry, Wc, Hc), dst=dst, **extra)
        out = self._host[:F * fb]
        ctx._check(ctx._lib.swk_device_read(ctx._h, base, out.ctypes.data, F * fb))          # one device -> host copy
        out.reshape(F, fb)[:, :mark] = np.frombuffer(FRAME_MARK, np.uint8)
        return out

    def write_window(self, popped_frames, rejected=None, new_events=()):
        """One window's popped Frame objects, oldest first; rejected: per frame the boxes (r0, c0, r1, c1) the classifier removed, or
        None; new_events: the events the tracker found in this window (lists of Segment objects)."""
        frames, boxes, marks, frame_style = plan = self.plan_window(popped_frames, rejected, new_events)
        if not frames:
            return
        if self.text:
            out = self._render(frames, boxes, marks, frame_style, labels=self.plan_labels(plan))
        else:
            out = self._render(frames, boxes, marks, frame_style)
        self._writer._fh.write(out)          # one file write
        self._writer.frames += len(frames)
        self.frames = self._writer.frames

    def _free(self):
        if self._dev:
            _lib.default_context(self.device).device_free(self._dev)
        self._dev = self._dev_bytes = 0
        self._host = None

    def close(self):
        if self._writer is not None:
            self._writer.close()
            self._writer = None
            self._free()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def removed_boxes(before, frames):
    """Per frame the boxes of the segments a classifier removed: before = a snapshot [list(frame.segments) for frame in frames] taken
    before it filtered."""
    out = []
    for was, frame in zip(before, frames):
        kept = {id(s) for s in frame.segments}
        out.append([tuple(s.bbox) for s in was if id(s) not in kept])
    return out
