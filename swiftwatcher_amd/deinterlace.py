"""Interlaced video: a frame reader that hands the counting loop whole pictures made of the fields.

A stored frame of an interlaced file (camcorder 1080i: YUV4MPEG2 tags It / Ib) holds two fields taken half a frame period apart in
its even and odd rows.  DeinterlacingReader wraps a reader of such a file (io_y4m.Y4MReader / YuvReader / Y4MStreamReader, opened with
interlaced=...) and per window asks the GPU (swk_yuv_deinterlace, csrc/deinterlace.hip) for the pictures of the fields over the crop
region plus its margin: rows of the kept field as stored, the others interpolated along edges and clamped around the temporal mean, so
that whatever does not move comes out exactly as stored.  It returns them as io_roi_stream.RoiFrame objects, so FrameQueue, the batch
calls, the classifier hand-over, the tracker, shape_props and the review writer see a progressive video and need not know."""
from collections import deque

import numpy as np

from . import _lib
from .io_roi_stream import RoiFrame, margin_rect

MODES = ("bob", "frame", "weave")


def footprint_pad(subsampling):
    """(rows, columns) of luma a rectangle grows by on every side when it is deinterlaced: one chroma row and three chroma columns of
    whole chroma cells (_lib._gather_fields)"""
    sx, sy = subsampling
    return (2 << sy) - 1, (4 << sx) - 1


class DeinterlacingReader:
    """reader: an io_y4m reader opened with interlaced=... (it says which field is the earlier one: field_order "t" or "b"; a
    progressive header, "p", is a ValueError -- nothing is guessed).  crop_region may be given later, through set_region, as the
    counting loop does once it has made the regions; a pipe's reader is then asked to hold the crop region plus its margin plus
    the deinterlacer's footprint.  A stabilize.StabilizingReader can sit on top: it calls set_region with the margin it needs.

    mode "bob": every field becomes a picture -- stored frame t gives pictures 2t and 2t + 1; fps is twice the header's rate,
    total_frames twice the stored count, and frame numbers, timestamps, the once-repeated last frame, the null frames after it and
    the counters are what io_frames.ArrayReader hands out over the list of the 2N pictures (start= / end= of the wrapped reader count
    stored frames: pictures 2 start .. 2 end).  mode "frame": the first field's picture of every frame, at the header's rate.  mode
    "weave": the stored frames as they are (what the reference would see), no GPU call.

    The video is the frames the wrapped reader hands out: the first and the last of them have no neighbour in time (the definition
    then takes the frame itself), also where start= / end= cut them out of a longer file.  The wrapped reader's own end-of-video
    deliveries (the repeated last frame, null frames) are recognised by its counters and never deinterlaced.  One library call per
    window, over the stored frames whose pictures the window still lacks plus one context frame on each side where the video has
    them; of an odd number of pictures the last frame's second one waits for the next window.

    read_frame(0, increment=False): the whole first picture as a BGR array, made by one call over the file's first two whole frames
    (the second is its neighbour in time; a pipe's reader keeps both until the first window) -- what generate_regions makes the
    ROI mask from.
    temporal=False: spatial interpolation only.  fields: {"mode", "field_order", "stored_frames", "frames"} so far.
    backend: what makes the calls (yuv_deinterlace of _lib.Context); None = the process's context on `device`."""

    def __init__(self, reader, crop_region=None, mode="bob", temporal=True, min_seg_size=(24, 24), device=0, backend=None):
        if mode not in MODES:
            raise ValueError("deinterlace is one of %s (got %r)" % (", ".join(MODES), mode))
        order = getattr(reader, "field_order", None)
        if order not in ("t", "b"):
            raise ValueError("deinterlace=%r, but the header of %s says %s: nothing is guessed"
                             % (mode, getattr(reader, "filepath", reader), "progressive (Ip)" if order == "p" else "nothing about fields"))
        self.reader, self.mode, self.field_order, self.temporal = reader, mode, order, bool(temporal)
        self.device, self._backend = device, backend
        self.rate = 2 if mode == "bob" else 1
        self.fps = reader.fps * self.rate if mode != "weave" else reader.fps
        self.start_frame = reader.start_frame * self.rate
        self.next_frame_number = self.start_frame
        self.frame_shape = tuple(reader.frame_shape)
        self.last_read_frame, self.frames_read, self.read_errors = None, 0, 0
        self.crop_region, self.min_seg_size, self._rect = None, tuple(int(s) for s in min_seg_size), None
        self._ready = deque()                        # pictures made and not yet handed out
        self._pulled = []                            # stored frames read and not yet deinterlaced (at most the one read ahead as context)
        self._prev = None                            # the last stored frame deinterlaced: the next call's context
        self._stored_done = False                    # the wrapped reader has handed out its last real frame
        self._handed = False
        self.stored_frames = 0
        if crop_region is not None:
            self.set_region(crop_region, min_seg_size)

    # ---- the wrapped reader's surface ----
    def __getattr__(self, name):                     # filepath, width, height, rate, close, read_seconds, ...
        if name.startswith("_") or name in ("reader", "ahead"):
            raise AttributeError(name)
        return getattr(self.reader, name)

    @property
    def ahead(self):
        return self.reader.ahead                     # (AttributeError where the wrapped reader does not read ahead)

    @ahead.setter
    def ahead(self, value):
        self.reader.ahead = value

    @property
    def end_frame(self):
        return self.reader.end_frame * (self.rate if self.mode != "weave" else 1)

    @property
    def total_frames(self):
        return self.end_frame - self.start_frame

    @property
    def fields(self):
        return {"mode": self.mode, "field_order": self.field_order, "stored_frames": int(self.stored_frames), "frames": int(self.frames_read)}

    def frame_number_to_timestamp(self, frame_number):
        if self.mode == "weave":
            return self.reader.frame_number_to_timestamp(frame_number)
        import datetime
        from .io_data import frame_timestamp_ns
        midnight = datetime.datetime.combine(datetime.date.today(), datetime.time())
        return midnight + datetime.timedelta(microseconds=frame_timestamp_ns(frame_number, self.fps) // 1000)

    def set_region(self, crop_region, min_seg_size=(24, 24)):
        """Pictures handed out from here on hold the crop region plus half the minimum segment size (io_roi_stream.margin_rect).
        Before the first window; later only the region already set is accepted."""
        region = [tuple(int(c) for c in crop_region[0]), tuple(int(c) for c in crop_region[1])]
        size = tuple(int(s) for s in min_seg_size)
        if self._handed:
            if (region, size) != (self.crop_region, self.min_seg_size):
                raise ValueError("the region of a deinterlacing reader is set before its first window is read")
            return
        self.crop_region, self.min_seg_size = region, size
        if self.mode == "weave":
            if hasattr(self.reader, "set_region"):
                self.reader.set_region(region, size)
            return
        ya, yb, xa, xb = margin_rect(self.frame_shape, region, size)
        if yb <= ya or xb <= xa:
            raise ValueError("the crop region lies outside the %dx%d picture" % (self.frame_shape[1], self.frame_shape[0]))
        self._rect = (ya, yb, xa, xb)
        if hasattr(self.reader, "set_region"):       # a pipe's reader: it holds the margin rectangle plus the footprint
            py, px = footprint_pad(getattr(self.reader, "subsampling", (1, 1)))
            self.reader.set_region(region, (size[0] + 2 * py, size[1] + 2 * px))

    def _ctx(self):
        return self._backend if self._backend is not None else _lib.default_context(self.device)

    def read_frame(self, frame_number, increment=True):
        if self.mode == "weave":
            return self.reader.read_frame(frame_number, increment)
        if frame_number != 0 or increment:
            raise ValueError("a deinterlacing reader only offers read_frame(0, increment=False); pictures come from get_n_frames")
        first = self.reader.read_frame(0, increment=False)
        if first is None:
            return None
        second = self.reader.read_frame(1, increment=False)
        stack = [first] if second is None else [first, second]
        return self._ctx().yuv_deinterlace(stack, None, self.field_order == "t", rate=1, temporal=self.temporal, has_next=second is not None)[0]

    def get_frame(self, frame_number=None):
        if frame_number is not None and frame_number != self.next_frame_number:
            raise ValueError("a deinterlacing reader hands its pictures out in order (next: %d)" % self.next_frame_number)
        frames, numbers, stamps = self.get_n_frames(1)
        return frames[0], numbers[0], stamps[0]

    # ---- stored frames in, pictures out ----
    def _pull(self, want):
        """Reads stored frames until `want` of them wait in _pulled, or the wrapped reader has no more.  Its end-of-video deliveries
        -- the last frame once more (its read_errors goes up) and null frames (number -1) -- end the video."""
        while len(self._pulled) < want and not self._stored_done:
            n = want - len(self._pulled)
            errors = self.reader.read_errors
            frames, numbers, _ = self.reader.get_n_frames(n)
            real = [f for f, k in zip(frames, numbers) if k >= 0]
            repeated = self.reader.read_errors - errors
            if repeated:
                real = real[:len(real) - repeated]
            self._pulled.extend(real)
            if len(real) < n:
                self._stored_done = True

    def _make(self, pictures):
        """One library call: at least `pictures` more pictures into _ready (as many as their stored frames give)."""
        m = -(-pictures // self.rate)
        self._pull(m + 1)                            # (one more: the last frame's neighbour in time)
        frames = self._pulled[:m]
        if not frames:
            return
        nxt = self._pulled[m:m + 1]
        self._pulled = self._pulled[m:]
        stack = ([self._prev] if self._prev is not None else []) + frames + nxt
        full_shape = tuple(frames[0].shape)
        if self._rect is None:
            rect, origin = None, None
        else:
            ya, yb, xa, xb = self._rect
            rect, origin = (xa, ya, xb - xa, yb - ya), (ya, xa)
        bgr = self._ctx().yuv_deinterlace(stack, rect, self.field_order == "t", rate=self.rate, temporal=self.temporal,
                                          has_prev=self._prev is not None, has_next=bool(nxt))
        self._prev = frames[-1]
        self.stored_frames += len(frames)
        for k in range(len(bgr)):
            self._ready.append(bgr[k] if origin is None else RoiFrame(bgr[k], origin, full_shape))

    def _null(self):
        if self._rect is None:
            return np.zeros(self.frame_shape, np.uint8)
        ya, yb, xa, xb = self._rect
        return RoiFrame(np.zeros((yb - ya, xb - xa, 3), np.uint8), (ya, xa), self.frame_shape)

    def get_n_frames(self, n):
        if self.mode == "weave":
            out = self.reader.get_n_frames(n)
            self._handed = True
            self.next_frame_number, self.frames_read, self.read_errors = (self.reader.next_frame_number, self.reader.frames_read,
                                                                          self.reader.read_errors)
            self.last_read_frame = self.reader.last_read_frame
            return out
        self._handed = True
        # number by number as io_frames.ArrayReader.get_frame decides (io_video.py:40-59); the pictures the window lacks are made when
        # the first of them is asked for (end_frame is read again for every number: a pipe's grows while its video goes on)
        frames, numbers, stamps = [], [], []
        for i in range(n):
            k = self.next_frame_number
            if not self.start_frame <= k <= self.end_frame:
                frames.append(self._null()); numbers.append(-1); stamps.append("00:00:00.000")          # (:40-44)
                continue
            self.next_frame_number += 1
            if not self._ready and not (self._stored_done and not self._pulled):
                self._make(n - i)
            if self._ready:
                frame = self._ready.popleft()
                self.last_read_frame, self.frame_shape = frame, tuple(frame.shape)
                self.frames_read += 1
            else:
                frame = self.last_read_frame                                                           # (:51-53)
                self.read_errors += 1
            frames.append(frame); numbers.append(k); stamps.append(self.frame_number_to_timestamp(k))
        return frames, numbers, stamps


def wrap(reader, mode, crop_region=None, temporal=True, min_seg_size=(24, 24), device=0):
    """The reader itself if it deinterlaces already or mode is None / False, else a DeinterlacingReader around it."""
    if not mode or isinstance(reader, DeinterlacingReader):
        return reader
    return DeinterlacingReader(reader, crop_region, mode, temporal, min_seg_size, device=device)
