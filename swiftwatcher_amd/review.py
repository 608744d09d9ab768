"""A review video of a count: the crop region's frames as an 8-bit 4:2:0 YUV4MPEG2 file (ffmpeg / mpv open it) with what was
counted drawn in -- the segments, the segments the classifier threw away, the ROI mask, and the tracker's events.  The reference
shows its users the same with `--export`, one overlay PNG per segment (data_structures.py:65-113); here a window's frames are
composed and converted by one GPU call (swk_render_review, include/swk.h) and leave with one device-to-host copy and one file
write.  pipeline.swift_counting_algorithm / count_swifts / count_swifts_videos feed a writer through review= / reviews=."""
import math

import numpy as np

from . import _lib
from .io_y4m import FRAME_MARK, Y4MWriter

STYLE_SEGMENT, STYLE_REJECTED, STYLE_EVENT, STYLE_MASK = 1, 2, 3, 4
# (b, g, r, fill_alpha, line_alpha), alphas 0..256
DEFAULT_STYLES = ((0, 255, 0, 32, 256),          # 1 segments: green outline, faint green fill
                  (0, 0, 255, 0, 160),           # 2 segments the classifier removed: red outline, no fill
                  (0, 255, 255, 0, 256),         # 3 events: yellow frame border and plus signs
                  (255, 128, 0, 40, 0))          # 4 ROI mask: light blue tint


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
    styles= replaces it (at least four rows).  Output is 8-bit 4:2:0 only, the crop region only, and carries no text."""

    MARK_ARM = 4
    BORDER = 3

    def __init__(self, path, crop_region, roi_mask, fps, device=0, styles=None, event_hold=15):
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
        self.device, self.event_hold = device, int(event_hold)
        self.frames = 0
        self._pending = []               # events still to be shown: (first frame number, last frame number, ((row, column), ...))
        self._dev = self._dev_bytes = 0
        self._host = None
        hc, wc = (self.height + 1) // 2, (self.width + 1) // 2
        self._luma, self._chroma = self.height * self.width, hc * wc
        self._frame_bytes = len(FRAME_MARK) + self._luma + 2 * self._chroma
        self._writer = Y4MWriter(path, self.width, self.height, fps)

    # ---- what is drawn (no GPU): the render call's arguments for one window ----
    def plan_window(self, popped_frames, rejected=None, new_events=()):
        """(frames to write, boxes, marks, frame_style) of one window: the Frame objects whose number is >= 0, and the overlay as
        swk_render_review takes it, `frame` counting the written frames.  Takes the new events in and forgets those that are over."""
        for event in new_events:
            first = int(event[-1].parent_frame_number) + 1
            self._pending.append((first, first + self.event_hold - 1, tuple(centroid_pixel(s.centroid) for s in event)))
        rejected = rejected if rejected is not None else [()] * len(popped_frames)
        frames, boxes, marks, frame_style = [], [], [], []
        for frame, gone in zip(popped_frames, rejected):
            if frame.frame_number < 0:
                continue
            k = len(frames)
            frames.append(frame)
            boxes.extend((k,) + tuple(int(v) for v in s.bbox) + (STYLE_SEGMENT,) for s in frame.segments)
            boxes.extend((k,) + tuple(int(v) for v in bbox) + (STYLE_REJECTED,) for bbox in (gone or ()))
            style = 0
            for first, last, points in self._pending:
                if first <= frame.frame_number <= last:
                    style = STYLE_EVENT
                    marks.extend((k, r, c, STYLE_EVENT) for r, c in points)
            frame_style.append(style)
        if frames:
            newest = max(f.frame_number for f in frames)
            self._pending = [ev for ev in self._pending if ev[1] > newest]
        return frames, boxes, marks, frame_style

    def _render(self, frames, boxes, marks, frame_style):
        """The window's frames composed and converted on the GPU: a uint8 array of len(frames) * frame bytes, every frame as the file
        holds it (the FRAME mark, then the Y, U and V planes), in page-locked memory."""
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
                             mem=_lib.MEM_DEVICE, layout=_lib.YUV_I420, y_row_stride=self.width, y_frame_stride=fb,
                             c_row_stride=(self.width + 1) // 2, c_frame_stride=fb)
        ctx.render_review(stack, boxes=boxes, marks=marks, frame_style=frame_style, mask=self.roi_mask, styles=self.styles,
                          mask_style=STYLE_MASK, mark_arm=self.MARK_ARM, border=self.BORDER, rect=(rx, ry, Wc, Hc), dst=dst)
        out = self._host[:F * fb]
        ctx._check(ctx._lib.swk_device_read(ctx._h, base, out.ctypes.data, F * fb))          # one device -> host copy
        out.reshape(F, fb)[:, :mark] = np.frombuffer(FRAME_MARK, np.uint8)
        return out

    def write_window(self, popped_frames, rejected=None, new_events=()):
        """One window's popped Frame objects, oldest first; rejected: per frame the boxes (r0, c0, r1, c1) the classifier removed, or
        None; new_events: the events the tracker found in this window (lists of Segment objects)."""
        frames, boxes, marks, frame_style = self.plan_window(popped_frames, rejected, new_events)
        if not frames:
            return
        self._writer._fh.write(self._render(frames, boxes, marks, frame_style))          # one file write
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
