"""Stabilizing shaken footage: a frame reader that hands the counting loop every frame cut where the scene lies, not where the camera
pointed.

The segment stage assumes that pixel (r, c) of the crop region is the same point of the scene in every frame of a window; a camera
that moves one pixel between frames puts every edge of the chimney into the sparse term.  StabilizingReader wraps any reader of full
frames, and per window asks the GPU (swk_stabilize_u8, csrc/stabilize.hip) for the integer shift of every frame at which the grey of
the crop region plus its margin differs least from an anchor image, and for the frame's pixels there.  It returns them as
io_roi_stream.RoiFrame objects labelled with the UNSHIFTED origin, so FrameQueue, the batch calls, the classifier hand-over, the
tracker and the review writer see a stabilized video and need not know.

With subpel=True the call is swk_stabilize_subpel_u8: after the integer search the 25 quarter-pixel shifts around its winner are scored
on the grey resampled with a 4-tap Catmull-Rom filter, and the frame's pixels are resampled at the best one, which takes the half
pixel of residue that integer shifts leave out of the segment stage's sparse term."""
import numpy as np

from . import _lib
from .io_roi_stream import RoiFrame, RoiStreamReader, margin_rect

MAX_SEARCH = 16


def search_range(stabilize):
    """pipeline's stabilize= value -> the search range S in pixels: True = 8, False / None / 0 = off"""
    if stabilize is None or stabilize is False:
        return 0
    if stabilize is True:
        return 8
    s = int(stabilize)
    if not 0 <= s <= MAX_SEARCH:
        raise ValueError("stabilize is a search range of 0..%d pixels (got %r)" % (MAX_SEARCH, stabilize))
    return s


def search_rect(frame_hw, crop_region, search, min_seg_size=(24, 24)):
    """((ya, yb, xa, xb) of the crop region plus its margin, (sa, sb, ta, tb) of that rectangle grown by `search` on every side and
    clipped to the picture: what a window's shift search reads)"""
    Hf, Wf = frame_hw[:2]
    ya, yb, xa, xb = margin_rect(frame_hw, crop_region, min_seg_size)
    return (ya, yb, xa, xb), (max(ya - search, 0), min(yb + search, Hf), max(xa - search, 0), min(xb + search, Wf))


class StabilizingReader:
    """reader: anything with the reference FrameReader's surface that hands out FULL frames (io_frames.ArrayReader, io_y4m's file
    readers, decoded ndarrays in an ArrayReader) or a pipe's reader (io_y4m.Y4MStreamReader: it is asked, through set_region, to hold
    the crop region plus its margin plus `search` pixels; ValueError if it has already fixed a smaller rectangle).  A ROI stream file
    (io_roi_stream.RoiStreamReader) holds a fixed margin and is refused.

    get_n_frames(n) returns the wrapped reader's frame numbers and timestamps with RoiFrame(pixels, origin = (ya, xa) of the
    unshifted margin rectangle, full_shape) objects that own their pixels.  read_frame, total_frames, fps, frame_number_to_timestamp
    and the counters are the wrapped reader's (the ROI mask is made from the unshifted first frame, which is the anchor).

    Anchor: the grey margin rectangle of the first real frame handed out.  After every `reanchor` windows it is replaced by the grey of
    the newest stabilized frame of that window (dusk footage darkens over an hour: a fixed anchor would end up matching against
    another exposure); reanchor=0 never replaces it.  shifts: frame number -> (dy, dx, sad, sad_unshifted).

    subpel=True: the quarter-pixel stage follows the integer search (stabilize_subpel of the backend instead of stabilize).  The
    rectangle read per window, and the one a pipe's reader is asked to hold, grow by search + 2 instead of search: the filter's
    footprint.  shifts keeps its meaning -- the integer stage's (dy, dx, sad, sad_unshifted) -- and subshifts: frame number ->
    (Qy, Qx, sad_subpel) holds the chosen total shift in quarter pixels and its score.  The anchor is replaced by the same rule: the
    grey of the newest stabilized (here: resampled) frame, as handed out.

    backend: what makes the calls (stabilize, stabilize_subpel and bgr2gray of _lib.Context); None = the process's context on `device`."""

    def __init__(self, reader, crop_region, search=8, min_seg_size=(24, 24), reanchor=1, device=0, gray_mode=_lib.GRAY_Q14, backend=None,
                 subpel=False):
        if isinstance(reader, RoiStreamReader) or isinstance(getattr(reader, "reader", None), RoiStreamReader):
            raise ValueError("a ROI stream file (RoiStreamReader) holds the crop region plus a fixed margin of half the minimum segment "
                             "size: there are no pixels to search a shift in; stabilize the source it was written from")
        self.search = int(search)
        if not 0 <= self.search <= MAX_SEARCH:
            raise ValueError("search is 0..%d pixels (got %r)" % (MAX_SEARCH, search))
        if int(reanchor) < 0:
            raise ValueError("reanchor is a number of windows, 0 = never (got %r)" % (reanchor,))
        self.reader = reader
        self.crop_region = [tuple(int(c) for c in crop_region[0]), tuple(int(c) for c in crop_region[1])]
        self.min_seg_size = tuple(int(s) for s in min_seg_size)
        self.reanchor, self.device, self.gray_mode = int(reanchor), device, int(gray_mode)
        self._backend = backend
        self.subpel = bool(subpel)
        self.grow = self.search + 2 if self.subpel else self.search          # pixels read around the margin rectangle on every side
        self.anchor = None
        self.shifts = {}
        self.subshifts = {}
        self.windows = 0
        self._staging = None
        if hasattr(reader, "set_region"):
            grown = (self.min_seg_size[0] + 2 * self.grow, self.min_seg_size[1] + 2 * self.grow)
            try:
                reader.set_region(self.crop_region, grown)
            except ValueError as exc:
                raise ValueError("stabilize: the stream reader has already fixed the rectangle it holds, which is smaller than the crop "
                                 "region plus its margin plus %d search pixels (%s)" % (self.grow, exc))

    # ---- the wrapped reader's surface ----
    def __getattr__(self, name):                     # fps, total_frames, start_frame, end_frame, filepath, read_frame, get_frame, counters
        if name.startswith("_") or name in ("reader", "ahead"):
            raise AttributeError(name)
        if name == "set_region":                     # offered where the wrapped reader offers it (a pipe's reader; the loop then sets `ahead` too)
            getattr(self.reader, name)
            return self._same_region
        return getattr(self.reader, name)

    @property
    def ahead(self):
        return self.reader.ahead                     # (AttributeError where the wrapped reader does not read ahead)

    @ahead.setter
    def ahead(self, value):
        self.reader.ahead = value

    def _same_region(self, crop_region, min_seg_size=(24, 24)):
        """set_region of a pipe's reader as the counting loop calls it: this reader has told the pipe's reader the grown rectangle
        already and accepts its own region alone."""
        region = [tuple(int(c) for c in crop_region[0]), tuple(int(c) for c in crop_region[1])]
        if region != self.crop_region or tuple(int(s) for s in min_seg_size) != self.min_seg_size:
            raise ValueError("a StabilizingReader is made for one crop region and minimum segment size")

    def _ctx(self):
        return self._backend if self._backend is not None else _lib.default_context(self.device)

    def _buffer(self, shape):
        if self._staging is None or self._staging.shape != tuple(shape):
            self._staging = _lib.pinned_empty(tuple(shape), np.uint8, device=self.device)
        return self._staging

    def get_n_frames(self, n):
        from .data_structures import stack_frames
        frames, numbers, stamps = self.reader.get_n_frames(n)
        first = frames[0]
        full_shape = tuple(first.shape)
        if len(full_shape) != 3 or full_shape[2] != 3:
            raise ValueError("stabilization needs BGR frames (H, W, 3)")
        (ya, yb, xa, xb), (sa, sb, ta, tb) = search_rect(full_shape, self.crop_region, self.grow, self.min_seg_size)
        Ho, Wo = yb - ya, xb - xa
        real = [k for k, num in enumerate(numbers) if num >= 0]
        if self.anchor is None and not real:         # nothing but null frames before any real one: nothing to match against
            zeros = np.zeros((len(frames), Ho, Wo, 3), np.uint8)
            return [RoiFrame(zeros[k], (ya, xa), full_shape) for k in range(len(frames))], numbers, stamps
        # the search rectangle of every frame, stacked: host memory for decoded frames, a device tensor for YUV frames (converted there)
        stack, _, _, backwards = stack_frames(frames, [(ta, sa), (tb, sb)], (0, 0), self._buffer, self.device)
        if backwards:
            stack = stack[::-1]
        ctx = self._ctx()
        if self.anchor is None:
            k = real[0]
            cutout = stack[k][ya - sa:yb - sa, xa - ta:xb - ta]
            if not isinstance(cutout, np.ndarray):
                cutout = cutout.contiguous().cpu().numpy()
            self.anchor = np.ascontiguousarray(ctx.bgr2gray(np.ascontiguousarray(cutout), self.gray_mode))
        if self.subpel:
            shifts, _, pixels = ctx.stabilize_subpel(stack, (ya - sa, xa - ta, Ho, Wo), self.search, self.anchor, gray_mode=self.gray_mode)
            for k in real:
                s = shifts[k]
                self.shifts[int(numbers[k])] = (int(s["dy"]), int(s["dx"]), int(s["sad_int"]), int(s["sad_unshifted"]))
                self.subshifts[int(numbers[k])] = (int(s["qy_total"]), int(s["qx_total"]), int(s["sad"]))
        else:
            shifts, _, pixels = ctx.stabilize(stack, (ya - sa, xa - ta, Ho, Wo), self.search, self.anchor, gray_mode=self.gray_mode)
            for k in real:
                s = shifts[k]
                self.shifts[int(numbers[k])] = (int(s["dy"]), int(s["dx"]), int(s["sad"]), int(s["sad_unshifted"]))
        self.windows += 1
        if self.reanchor and real and self.windows % self.reanchor == 0:
            self.anchor = np.ascontiguousarray(ctx.bgr2gray(np.ascontiguousarray(pixels[real[-1]]), self.gray_mode))
        return [RoiFrame(pixels[k], (ya, xa), full_shape) for k in range(len(frames))], numbers, stamps


def summary(shifts, search, subshifts=None):
    """The CLI's "stabilize" entry: {"search": S, "moved_frames": frames with a shift other than (0, 0), "max_shift": the largest
    |dy| or |dx|}; with the quarter-pixel stage's subshifts also "subpel": true and "fractional_frames": frames whose chosen total
    shift is not a whole number of pixels on both axes"""
    moved = [v for v in shifts.values() if v[0] or v[1]]
    out = {"search": int(search), "moved_frames": len(moved), "max_shift": max((max(abs(v[0]), abs(v[1])) for v in moved), default=0)}
    if subshifts is not None:
        out["subpel"] = True
        out["fractional_frames"] = sum(1 for v in subshifts.values() if v[0] % 4 or v[1] % 4)
    return out


CSV_COLUMNS = ("frame_number", "dy", "dx", "sad", "sad_unshifted")
CSV_SUBPEL_COLUMNS = ("shift_y", "shift_x", "sad_subpel")


def write_csv(path, shifts, subshifts=None):
    """stabilization.csv: one row per frame, ascending frame number; with the quarter-pixel stage's subshifts three more columns: the
    chosen total shift in pixels as decimal text with two places (-1.25) and its score"""
    import csv
    with open(path, "w", newline="") as fh:
        w = csv.writer(fh)
        w.writerow(CSV_COLUMNS + (CSV_SUBPEL_COLUMNS if subshifts is not None else ()))
        for number in sorted(shifts):
            row = [int(number)] + [int(x) for x in shifts[number]]
            if subshifts is not None:
                Qy, Qx, sad = subshifts[number]
                row += [quarter_text(Qy), quarter_text(Qx), int(sad)]
            w.writerow(row)


def quarter_text(Q):
    """Q quarter pixels as pixels with two decimal places: -5 -> "-1.25" (exact: integer arithmetic)"""
    Q = int(Q)
    return "%s%d.%02d" % ("-" if Q < 0 else "", abs(Q) // 4, abs(Q) % 4 * 25)
