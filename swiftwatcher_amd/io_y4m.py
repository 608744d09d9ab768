"""YUV4MPEG2 (.y4m) videos: the uncompressed container every decoder can write (`ffmpeg -i in.mp4 out.y4m`) -- a one-line header,
then per frame the six bytes "FRAME\\n" and the Y, U and V planes of the picture.  No codec is involved: the file is memory-mapped
and a frame is views of the mapping (Yuv420Frame for 8-bit 4:2:0 limited range, YuvFrame for every other format).

The reference sees BGR frames (cv2.VideoCapture, io_video.py:85-125).  A Yuv420Frame / YuvFrame stands in for one: it has the BGR
frame's shape and dtype, np.asarray(frame) and frame[rows, columns] give the BGR pixels -- converted on the host by the definition
in include/swk.h (swk_yuv420_to_bgr: cv2.cvtColor(yuv, COLOR_YUV2BGR_I420) of OpenCV 4.1.0 restated; swk_yuv_to_bgr: the same
formula for every subsampling, 8..16 bits and both ranges; PARITY UNPINNED) -- so crop_frame, generate_regions on the first frame,
Segment.segment_image and export_segments work unchanged.  The counting loop never converts a whole frame:
data_structures.stack_frames uploads the ROI's luma and chroma samples and converts on the GPU (csrc/yuv.hip), bit for bit the
same pixels.

open_y4m(path) picks the reader.  Y4MReader: 8-bit 4:2:0, progressive; it refuses everything else by name.  YuvReader: C420*,
C422, C444, C411 and Cmono, with the suffixes p9, p10, p12, p14, p16 (mono9, mono10, mono12, mono16: little-endian 16-bit samples),
limited range or, with XCOLORRANGE=FULL, full range.  C444alpha, mixed field order (Im) and FRAME lines with parameters are refused by
name, and so are interlaced files (It, Ib) unless the reader is made with interlaced=: it then hands out the stored, woven frames
and says which field is the earlier one (field_order), for deinterlace.DeinterlacingReader to make pictures of.

A source that can only be read once, front to back, and whose length nobody knows -- "-" (standard input), a FIFO, a descriptor, a
binary file object: `ffmpeg -i in.mp4 -f yuv4mpegpipe - | python -m swiftwatcher_amd - --corners ...` -- gets Y4MStreamReader: the
same formats and refusals, the same frames, numbers, timestamps and counters call by call, total_frames / end_frame as properties
that look one FRAME marker ahead.  Told the crop region, it hands out Yuv420RectFrame / YuvRectFrame, which hold only the rectangle
the counting loop reads and index in full-frame coordinates: the bytes it holds do not grow with the video."""
import datetime
import os
import stat
import sys
import threading
import time
from collections import deque

import numpy as np

from .io_frames import ArrayReader

MAGIC = b"YUV4MPEG2"
FRAME_MARK = b"FRAME\n"
CHROMA_420 = ("420", "420jpeg", "420mpeg2", "420paldv")          # one memory layout; the siting only matters to an interpolating converter

# ITU-R BT.601 limited range in 20-bit fixed point (OpenCV 4.1.0, YUV420p2RGB8Invoker)
_CY, _CUB, _CUG, _CVG, _CVR, _SHIFT = 1220542, 2116026, -409993, -852492, 1673527, 20


def yuv420_rect_to_bgr(y, u, v, r0, r1, c0, c1):
    """BGR pixels [r0, r1) x [c0, c1) of one 4:2:0 picture (y (H, W), u and v (ceil(H/2), ceil(W/2)), uint8), on the host.  The
    chroma terms are formed once per chroma sample and gathered per pixel; all in int32 (largest magnitude 5.7e8)."""
    rows, cols = max(r1 - r0, 0), max(c1 - c0, 0)
    out = np.empty((rows, cols, 3), np.uint8)
    if rows == 0 or cols == 0:
        return out
    cr0, cc0 = r0 >> 1, c0 >> 1
    uu = u[cr0:((r1 - 1) >> 1) + 1, cc0:((c1 - 1) >> 1) + 1].astype(np.int32) - 128
    vv = v[cr0:((r1 - 1) >> 1) + 1, cc0:((c1 - 1) >> 1) + 1].astype(np.int32) - 128
    half = 1 << (_SHIFT - 1)
    terms = (half + _CUB * uu, half + _CVG * vv + _CUG * uu, half + _CVR * vv)          # B, G, R
    ri = ((np.arange(r0, r1) >> 1) - cr0)[:, None]
    ci = ((np.arange(c0, c1) >> 1) - cc0)[None, :]
    luma = np.maximum(y[r0:r1, c0:c1].astype(np.int32) - 16, 0) * _CY
    for k, t in enumerate(terms):
        np.clip((luma + t[ri, ci]) >> _SHIFT, 0, 255, out=out[..., k], casting="unsafe")
    return out


class Yuv420Frame:
    """One 8-bit 4:2:0 picture standing in for the BGR frame a reference reader would have returned: y (H, W), u and v
    (ceil(H/2), ceil(W/2)) are views of the file's mapping (or any uint8 arrays).  Looks like the (H, W, 3) uint8 BGR array where
    the loop looks at it: shape, dtype, ndim, np.asarray(frame), frame[rows, columns]."""
    __slots__ = ("y", "u", "v", "shape")
    dtype = np.dtype(np.uint8)
    ndim = 3

    def __init__(self, y, u, v):
        H, W = y.shape
        if u.shape != ((H + 1) // 2, (W + 1) // 2) or v.shape != u.shape:
            raise ValueError("chroma planes of a %dx%d 4:2:0 picture are %dx%d" % (W, H, (W + 1) // 2, (H + 1) // 2))
        self.y, self.u, self.v, self.shape = y, u, v, (H, W, 3)

    @classmethod
    def null(cls, height, width):
        """The reference's null frame (all-zero BGR, io_video.py:40-44): Y = 0, U = V = 128 converts to (0, 0, 0)."""
        ch, cw = (height + 1) // 2, (width + 1) // 2
        return cls(np.zeros((height, width), np.uint8), np.full((ch, cw), 128, np.uint8), np.full((ch, cw), 128, np.uint8))

    def __len__(self):
        return self.shape[0]

    def __array__(self, dtype=None, copy=None):
        bgr = yuv420_rect_to_bgr(self.y, self.u, self.v, 0, self.shape[0], 0, self.shape[1])
        return bgr if dtype is None else bgr.astype(dtype, copy=False)

    def __getitem__(self, key):
        """frame[r0:r1, c0:c1] (and frame[r0:r1]): the BGR pixels of that rectangle alone; anything else indexes the whole BGR frame."""
        rows, cols = (key, slice(None)) if isinstance(key, slice) else (key if isinstance(key, tuple) and len(key) == 2 else (None, None))
        if isinstance(rows, slice) and isinstance(cols, slice):
            r0, r1, rs = rows.indices(self.shape[0])
            c0, c1, cs = cols.indices(self.shape[1])
            if rs == 1 and cs == 1:
                return yuv420_rect_to_bgr(self.y, self.u, self.v, r0, r1, c0, c1)
        return np.asarray(self)[key]


# (CY, CUB, CUG, CVG, CVR) of include/swk.h: BT.601 in 20-bit fixed point, limited range (OpenCV's) and full range
_LIMITED = (_CY, _CUB, _CUG, _CVG, _CVR)
_FULL = (1048576, 1858077, -360853, -748826, 1470104)


def yuv_rect_to_bgr(y, u, v, r0, r1, c0, c1, sx=1, sy=1, bits=8, full_range=False):
    """BGR pixels [r0, r1) x [c0, c1) of one picture by the definition of swk_yuv_to_bgr (include/swk.h), on the host in int64:
    y (H, W), u and v (ceil(H / 2^sy), ceil(W / 2^sx)) or both None (mono), uint8 or uint16 samples of `bits` bits taken as stored."""
    rows, cols = max(r1 - r0, 0), max(c1 - c0, 0)
    out = np.empty((rows, cols, 3), np.uint8)
    if rows == 0 or cols == 0:
        return out
    k = bits - 8
    cy, cub, cug, cvg, cvr = _FULL if full_range else _LIMITED
    half, shift = 1 << (_SHIFT - 1 + k), _SHIFT + k
    luma = y[r0:r1, c0:c1].astype(np.int64)
    if not full_range:
        luma = np.maximum(luma - (16 << k), 0)
    luma *= cy
    if u is None:
        np.clip((luma + half) >> shift, 0, 255, out=out[..., 0], casting="unsafe")
        out[..., 1] = out[..., 0]
        out[..., 2] = out[..., 0]
        return out
    cr0, cc0 = r0 >> sy, c0 >> sx
    uu = u[cr0:((r1 - 1) >> sy) + 1, cc0:((c1 - 1) >> sx) + 1].astype(np.int64) - (128 << k)
    vv = v[cr0:((r1 - 1) >> sy) + 1, cc0:((c1 - 1) >> sx) + 1].astype(np.int64) - (128 << k)
    terms = (half + cub * uu, half + cvg * vv + cug * uu, half + cvr * vv)          # B, G, R
    ri = ((np.arange(r0, r1) >> sy) - cr0)[:, None]
    ci = ((np.arange(c0, c1) >> sx) - cc0)[None, :]
    for j, t in enumerate(terms):
        np.clip((luma + t[ri, ci]) >> shift, 0, 255, out=out[..., j], casting="unsafe")
    return out


class YuvFrame:
    """One planar YUV picture of any format of swk_yuv_to_bgr standing in for the BGR frame a reference reader would have returned:
    y (H, W), u and v (ceil(H / 2^sy), ceil(W / 2^sx)) or None for a mono picture; uint8 samples at bits = 8, uint16 (LSB-aligned)
    above.  Looks like the (H, W, 3) uint8 BGR array where the loop looks at it, as Yuv420Frame does."""
    __slots__ = ("y", "u", "v", "shape", "sx", "sy", "bits", "full_range")
    dtype = np.dtype(np.uint8)
    ndim = 3

    def __init__(self, y, u=None, v=None, subsampling=(1, 1), bits=8, full_range=False):
        H, W = y.shape
        sx, sy = (0, 0) if u is None else (int(subsampling[0]), int(subsampling[1]))
        if not (8 <= bits <= 16 and 0 <= sx <= 2 and 0 <= sy <= 1):
            raise ValueError("bits must be 8..16 and the chroma shifts (0..2, 0..1)")
        want = np.uint16 if bits > 8 else np.uint8
        if (u is None) != (v is None) or any(p is not None and p.dtype != want for p in (y, u, v)):
            raise ValueError("a %d-bit picture has %s planes: y alone (mono), or y, u and v" % (bits, np.dtype(want).name))
        cshape = (((H - 1) >> sy) + 1, ((W - 1) >> sx) + 1)
        if u is not None and (u.shape != cshape or v.shape != cshape):
            raise ValueError("chroma planes of this %dx%d picture are %dx%d" % (W, H, cshape[1], cshape[0]))
        self.y, self.u, self.v, self.shape = y, u, v, (H, W, 3)
        self.sx, self.sy, self.bits, self.full_range = sx, sy, int(bits), bool(full_range)

    @property
    def format(self):
        """What two frames must share to be staged and converted in one call."""
        return (self.u is None, self.sx, self.sy, self.bits, self.full_range)

    @classmethod
    def null(cls, height, width, subsampling=(1, 1), bits=8, full_range=False, mono=False):
        """The reference's null frame (all-zero BGR, io_video.py:40-44): Y = 0, U = V = 128 << (bits - 8) converts to (0, 0, 0)."""
        dt = np.uint16 if bits > 8 else np.uint8
        y = np.zeros((height, width), dt)
        if mono:
            return cls(y, None, None, (0, 0), bits, full_range)
        cshape = (((height - 1) >> subsampling[1]) + 1, ((width - 1) >> subsampling[0]) + 1)
        return cls(y, np.full(cshape, 128 << (bits - 8), dt), np.full(cshape, 128 << (bits - 8), dt), subsampling, bits, full_range)

    def __len__(self):
        return self.shape[0]

    def _rect(self, r0, r1, c0, c1):
        return yuv_rect_to_bgr(self.y, self.u, self.v, r0, r1, c0, c1, self.sx, self.sy, self.bits, self.full_range)

    def __array__(self, dtype=None, copy=None):
        bgr = self._rect(0, self.shape[0], 0, self.shape[1])
        return bgr if dtype is None else bgr.astype(dtype, copy=False)

    def __getitem__(self, key):
        """frame[r0:r1, c0:c1] (and frame[r0:r1]): the BGR pixels of that rectangle alone; anything else indexes the whole BGR frame."""
        rows, cols = (key, slice(None)) if isinstance(key, slice) else (key if isinstance(key, tuple) and len(key) == 2 else (None, None))
        if isinstance(rows, slice) and isinstance(cols, slice):
            r0, r1, rs = rows.indices(self.shape[0])
            c0, c1, cs = cols.indices(self.shape[1])
            if rs == 1 and cs == 1:
                return self._rect(r0, r1, c0, c1)
        return np.asarray(self)[key]


_SUBSAMPLING = {"420": (1, 1), "422": (1, 0), "444": (0, 0), "411": (2, 0)}
_DEPTHS = {"": 8, "p9": 9, "p10": 10, "p12": 12, "p14": 14, "p16": 16}
_MONO_DEPTHS = {"mono": 8, "mono9": 9, "mono10": 10, "mono12": 12, "mono16": 16}


def _chroma_format(value):
    """(mono, sx, sy, bits) of the value of a C tag, None for one that is not supported (C444alpha among them)."""
    if value in _MONO_DEPTHS:
        return (True, 0, 0, _MONO_DEPTHS[value])
    if value in CHROMA_420:
        return (False, 1, 1, 8)
    if value[:3] in _SUBSAMPLING and value[3:] in _DEPTHS:
        return (False,) + _SUBSAMPLING[value[:3]] + (_DEPTHS[value[3:]],)
    return None


def _parse_header(line, general=False, interlaced=None):
    """(width, height, fps numerator, denominator) of a YUV4MPEG2 stream header line (without its newline).  general: every format
    of open_y4m is accepted, and the result ends with its (mono, sx, sy, bits, full_range).  interlaced: None refuses It / Ib by
    name; any other value accepts them, and the result ends with the field order, "p" (I?, Ip or no I tag), "t" or "b".  Im (mixed)
    is always refused."""
    tags = line.split(b" ")
    if tags[0] != MAGIC:
        raise ValueError("not a YUV4MPEG2 file")
    width = height = rate = None
    fmt, full, order = (False, 1, 1, 8), False, "p"
    for raw in tags[1:]:
        if not raw:
            continue
        tag = raw.decode("ascii", "replace")
        kind, value = tag[0], tag[1:]
        try:
            if kind == "W":
                width = int(value)
            elif kind == "H":
                height = int(value)
            elif kind == "F":
                num, den = value.split(":")
                rate = (int(num), int(den))
            elif kind == "I":
                if value in ("t", "b") and interlaced is None:
                    raise ValueError("interlaced YUV4MPEG2 files are not supported (tag %s) unless they are deinterlaced: "
                                     "deinterlace= / --deinterlace" % tag)
                if value == "m":
                    raise ValueError("interlaced YUV4MPEG2 files are not supported (tag %s): mixed field order" % tag)
                if value not in ("?", "p", "t", "b"):          # (any other value, worded as it always was)
                    raise ValueError("interlaced YUV4MPEG2 files are not supported (tag %s)" % tag)
                order = "p" if value == "?" else value
            elif kind == "C" and general:
                fmt = _chroma_format(value)
                if fmt is None:
                    raise ValueError("this YUV4MPEG2 pixel format is not supported (tag %s)" % tag)
            elif kind == "C":
                if value not in CHROMA_420:
                    raise ValueError("only 8-bit 4:2:0 YUV4MPEG2 files are supported (tag %s)" % tag)
            elif kind == "X" and general and value.startswith("COLORRANGE="):
                if value[11:] not in ("FULL", "LIMITED"):
                    raise ValueError("unknown YUV4MPEG2 colour range (tag %s)" % tag)
                full = value[11:] == "FULL"
            elif kind in "AX":
                pass                                  # pixel aspect, and comments such as ffmpeg's XYSCSS= / XCOLORRANGE=
            else:
                raise ValueError("unknown YUV4MPEG2 header tag %s" % tag)
        except ValueError as exc:
            if "YUV4MPEG2" in str(exc):
                raise
            raise ValueError("malformed YUV4MPEG2 header tag %s" % tag)
    for name, got in (("W", width), ("H", height), ("F", rate)):
        if got is None:
            raise ValueError("the YUV4MPEG2 header has no %s tag" % name)
    if width < 1 or height < 1 or rate[0] < 1 or rate[1] < 1:
        raise ValueError("the YUV4MPEG2 header needs positive W, H and F (got W%d H%d F%d:%d)" % (width, height, rate[0], rate[1]))
    out = (width, height, rate[0], rate[1]) + ((fmt + (full,),) if general else ())
    return out if interlaced is None else out + (order,)


class _Frames:
    """The frames of a mapped .y4m file as a sequence of Yuv420Frame: every frame has the same size, so offsets are arithmetic."""

    def __init__(self, mapping, first, width, height, count):
        self.mapping, self.first, self.width, self.height, self.count = mapping, first, width, height, count
        self.luma = width * height
        self.chroma = ((width + 1) // 2) * ((height + 1) // 2)
        self.step = len(FRAME_MARK) + self.luma + 2 * self.chroma

    def __len__(self):
        return self.count

    def __getitem__(self, k):
        if not 0 <= k < self.count:
            raise IndexError(k)
        at = self.first + k * self.step + len(FRAME_MARK)
        ch, cw = (self.height + 1) // 2, (self.width + 1) // 2
        m = self.mapping
        return Yuv420Frame(m[at:at + self.luma].reshape(self.height, self.width),
                           m[at + self.luma:at + self.luma + self.chroma].reshape(ch, cw),
                           m[at + self.luma + self.chroma:at + self.luma + 2 * self.chroma].reshape(ch, cw))


class Y4MReader(ArrayReader):
    """ArrayReader over a memory-mapped YUV4MPEG2 file: get_frame / get_n_frames with the reference FrameReader's bookkeeping
    (io_video.py:13-82; the frame one past the end is served once by the last good frame, null frames after that), frames handed
    out as Yuv420Frame views of the mapping -- only the pages the ROI touches are ever read from disk.  fps comes from the header."""

    def __init__(self, path, start=0, end=0, interlaced=None):
        with open(path, "rb") as fh:
            head = fh.read(4096)
        if not head.startswith(MAGIC):
            raise ValueError("not a YUV4MPEG2 file: %s" % path)
        eol = head.find(b"\n")
        if eol < 0:
            raise ValueError("the YUV4MPEG2 header line does not end: %s" % path)
        width, height, num, den, self.field_order = (_parse_header(head[:eol], interlaced=interlaced) + ("p",))[:5]
        mapping = np.memmap(path, dtype=np.uint8, mode="r")
        first = eol + 1
        frames = _Frames(mapping, first, width, height, 0)
        body = mapping.size - first
        if body >= len(FRAME_MARK) and bytes(mapping[first:first + 5]) == b"FRAME" and mapping[first + 5] != 0x0A:
            raise ValueError("FRAME headers with parameters are not supported: %s" % path)
        if body % frames.step:
            raise ValueError("%s is truncated: %d bytes after the header are not whole frames of %d bytes" % (path, body, frames.step))
        frames.count = body // frames.step
        if frames.count and bytes(mapping[first:first + len(FRAME_MARK)]) != FRAME_MARK:
            raise ValueError("no FRAME marker after the header: %s" % path)
        self.width, self.height, self.rate = width, height, (num, den)
        ArrayReader.__init__(self, frames, fps=num / den, start=start, end=end, filepath=path)
        self.frame_shape = (height, width, 3)

    def get_frame(self, frame_number=None):
        if frame_number is None:
            frame_number = self.next_frame_number
        if not self.start_frame <= frame_number <= self.end_frame:
            return Yuv420Frame.null(self.height, self.width), -1, "00:00:00.000"          # (:40-44)
        return ArrayReader.get_frame(self, frame_number)


class _YuvFrames:
    """The frames of a mapped .y4m file of any supported format as a sequence of YuvFrame: equal sizes, so offsets are arithmetic."""

    def __init__(self, mapping, first, width, height, fmt, count):
        self.mapping, self.first, self.width, self.height, self.count = mapping, first, width, height, count
        self.mono, self.sx, self.sy, self.bits, self.full_range = fmt
        self.sample = 2 if self.bits > 8 else 1
        self.cshape = (((height - 1) >> self.sy) + 1, ((width - 1) >> self.sx) + 1)
        self.luma = width * height * self.sample
        self.chroma = 0 if self.mono else self.cshape[0] * self.cshape[1] * self.sample
        self.step = len(FRAME_MARK) + self.luma + 2 * self.chroma

    def __len__(self):
        return self.count

    def _plane(self, at, nbytes, shape):
        raw = self.mapping[at:at + nbytes]
        if self.sample == 2:
            raw = raw.view("<u2")          # (at an odd file offset an unaligned view: numpy reads it correctly, staging copies bytes)
        return raw.reshape(shape)

    def __getitem__(self, k):
        if not 0 <= k < self.count:
            raise IndexError(k)
        at = self.first + k * self.step + len(FRAME_MARK)
        y = self._plane(at, self.luma, (self.height, self.width))
        if self.mono:
            return YuvFrame(y, None, None, (0, 0), self.bits, self.full_range)
        return YuvFrame(y, self._plane(at + self.luma, self.chroma, self.cshape),
                        self._plane(at + self.luma + self.chroma, self.chroma, self.cshape), (self.sx, self.sy), self.bits, self.full_range)


class YuvReader(ArrayReader):
    """Y4MReader's bookkeeping over a memory-mapped YUV4MPEG2 file of any format open_y4m accepts, frames handed out as YuvFrame
    views of the mapping.  full_range: None = what the header says (XCOLORRANGE=FULL, else limited), True / False override it."""

    def __init__(self, path, start=0, end=0, full_range=None, interlaced=None):
        with open(path, "rb") as fh:
            head = fh.read(4096)
        if not head.startswith(MAGIC):
            raise ValueError("not a YUV4MPEG2 file: %s" % path)
        eol = head.find(b"\n")
        if eol < 0:
            raise ValueError("the YUV4MPEG2 header line does not end: %s" % path)
        width, height, num, den, fmt, self.field_order = (_parse_header(head[:eol], general=True, interlaced=interlaced) + ("p",))[:6]
        if full_range is not None:
            fmt = fmt[:4] + (bool(full_range),)
        mapping = np.memmap(path, dtype=np.uint8, mode="r")
        first = eol + 1
        frames = _YuvFrames(mapping, first, width, height, fmt, 0)
        body = mapping.size - first
        if body >= len(FRAME_MARK) and bytes(mapping[first:first + 5]) == b"FRAME" and mapping[first + 5] != 0x0A:
            raise ValueError("FRAME headers with parameters are not supported: %s" % path)
        if body % frames.step:
            raise ValueError("%s is truncated: %d bytes after the header are not whole frames of %d bytes" % (path, body, frames.step))
        frames.count = body // frames.step
        if frames.count and bytes(mapping[first:first + len(FRAME_MARK)]) != FRAME_MARK:
            raise ValueError("no FRAME marker after the header: %s" % path)
        self.width, self.height, self.rate = width, height, (num, den)
        self.mono, self.subsampling, self.bits, self.full_range = fmt[0], (fmt[1], fmt[2]), fmt[3], fmt[4]
        ArrayReader.__init__(self, frames, fps=num / den, start=start, end=end, filepath=path)
        self.frame_shape = (height, width, 3)

    def get_frame(self, frame_number=None):
        if frame_number is None:
            frame_number = self.next_frame_number
        if not self.start_frame <= frame_number <= self.end_frame:
            return YuvFrame.null(self.height, self.width, self.subsampling, self.bits, self.full_range, self.mono), -1, "00:00:00.000"
        return ArrayReader.get_frame(self, frame_number)


# ---------------------------------------------------------------------------------------------------- reading from a pipe
def _held_error(r0, r1, c0, c1, oy, ox, h, w):
    return IndexError("rows %d:%d, columns %d:%d leave the held rectangle (rows %d:%d, columns %d:%d)" % (r0, r1, c0, c1, oy, oy + h, ox, ox + w))


class _RectFrame:
    """What Yuv420RectFrame and YuvRectFrame share: the planes hold luma rows [oy, oy + h) x columns [ox, ox + w) of the picture and
    the chroma samples that cover them; (oy, ox) lies on the chroma grid, so a pixel's chroma sample is found the same way in the
    held planes as in the whole ones.  Indexed in full-frame coordinates like io_roi_stream.RoiFrame."""
    __slots__ = ()

    def _holds_all(self):
        return self.origin == (0, 0) and self.y.shape == self.shape[:2]

    def __array__(self, dtype=None, copy=None):
        if not self._holds_all():
            raise _held_error(0, self.shape[0], 0, self.shape[1], self.origin[0], self.origin[1], *self.y.shape)
        bgr = self._held_rect(0, self.shape[0], 0, self.shape[1])
        return bgr if dtype is None else bgr.astype(dtype, copy=False)

    def __getitem__(self, key):
        """frame[r0:r1, c0:c1] in full-frame coordinates: the BGR pixels the whole picture's frame would give; IndexError for a
        rectangle that leaves the held one."""
        if isinstance(key, slice):
            key = (key, slice(None))
        if not (isinstance(key, tuple) and len(key) >= 2 and isinstance(key[0], slice) and isinstance(key[1], slice)):
            if self._holds_all():
                return np.asarray(self)[key]
            raise TypeError("a frame that holds a rectangle is indexed with two slices in full-frame coordinates: frame[y0:y1, x0:x1]")
        if key[0].step not in (None, 1) or key[1].step not in (None, 1):
            raise TypeError("strided access to a frame that holds a rectangle")
        r0, r1, _ = key[0].indices(self.shape[0])
        c0, c1, _ = key[1].indices(self.shape[1])
        oy, ox = self.origin
        h, w = self.y.shape
        if r1 > r0 and c1 > c0 and (r0 < oy or c0 < ox or r1 > oy + h or c1 > ox + w):
            raise _held_error(r0, r1, c0, c1, oy, ox, h, w)
        out = self._held_rect(r0, r1, c0, c1)
        return out[(slice(None), slice(None)) + tuple(key[2:])] if len(key) > 2 else out


class Yuv420RectFrame(_RectFrame, Yuv420Frame):
    """A Yuv420Frame that holds one rectangle of its picture: y (h, w) from the even origin (oy, ox), u and v (ceil(h/2), ceil(w/2))."""
    __slots__ = ("origin",)

    def __init__(self, y, u, v, origin, full_shape):
        oy, ox = int(origin[0]), int(origin[1])
        h, w = y.shape
        H, W = int(full_shape[0]), int(full_shape[1])
        if oy & 1 or ox & 1 or oy < 0 or ox < 0 or oy + h > H or ox + w > W:
            raise ValueError("the held rectangle starts on even rows and columns inside the %dx%d picture" % (W, H))
        if u.shape != ((h + 1) // 2, (w + 1) // 2) or v.shape != u.shape:
            raise ValueError("chroma planes of a %dx%d 4:2:0 rectangle are %dx%d" % (w, h, (w + 1) // 2, (h + 1) // 2))
        self.y, self.u, self.v, self.shape, self.origin = y, u, v, (H, W, 3), (oy, ox)

    def _held_rect(self, r0, r1, c0, c1):
        oy, ox = self.origin
        return yuv420_rect_to_bgr(self.y, self.u, self.v, r0 - oy, r1 - oy, c0 - ox, c1 - ox)


class YuvRectFrame(_RectFrame, YuvFrame):
    """A YuvFrame that holds one rectangle of its picture: y (h, w) from the origin (oy, ox), a multiple of (2^sy, 2^sx), u and v
    (ceil(h / 2^sy), ceil(w / 2^sx)) or None."""
    __slots__ = ("origin",)

    def __init__(self, y, u, v, origin, full_shape, subsampling=(1, 1), bits=8, full_range=False):
        YuvFrame.__init__(self, y, u, v, subsampling, bits, full_range)          # (checks the planes against each other)
        oy, ox = int(origin[0]), int(origin[1])
        h, w = y.shape
        H, W = int(full_shape[0]), int(full_shape[1])
        if oy & ((1 << self.sy) - 1) or ox & ((1 << self.sx) - 1) or oy < 0 or ox < 0 or oy + h > H or ox + w > W:
            raise ValueError("the held rectangle starts on the chroma grid inside the %dx%d picture" % (W, H))
        self.shape, self.origin = (H, W, 3), (oy, ox)

    def _held_rect(self, r0, r1, c0, c1):
        oy, ox = self.origin
        return yuv_rect_to_bgr(self.y, self.u, self.v, r0 - oy, r1 - oy, c0 - ox, c1 - ox, self.sx, self.sy, self.bits, self.full_range)


def held_rect(frame_hw, crop_region, min_seg_size=(24, 24), subsampling=(1, 1)):
    """(ya, yb, xa, xb) of the luma pixels a frame must hold for the counting loop over crop_region: the crop region plus half the
    minimum segment size (io_roi_stream.margin_rect), its origin moved up and left onto the chroma grid (what
    data_structures._stack_yuv420 / _stack_yuv stage)."""
    from .io_roi_stream import margin_rect
    ya, yb, xa, xb = margin_rect(frame_hw, crop_region, min_seg_size)
    sx, sy = subsampling
    return (ya >> sy) << sy, yb, (xa >> sx) << sx, xb


class _ByteSource:
    """Bytes in order from "-" (standard input), a file descriptor, a path (a FIFO) or a binary file object with readinto or read.
    fill() loops over short reads; seconds / bytes: time spent in, and bytes got from, the source's read calls."""

    def __init__(self, source):
        self._own = None
        if isinstance(source, str) and source == "-":
            fh, self.name = sys.stdin.buffer, "<stdin>"
        elif isinstance(source, int):
            fh = self._own = os.fdopen(source, "rb", buffering=0, closefd=False)          # (closing the wrapper leaves the descriptor open)
            self.name = "<descriptor %d>" % source
        elif isinstance(source, (str, bytes)) or hasattr(source, "__fspath__"):
            fh = self._own = open(source, "rb", buffering=0)
            self.name = os.fsdecode(source)
        else:
            fh, self.name = source, str(getattr(source, "name", None) or "<%s>" % type(source).__name__)
        self._readinto, self._read = getattr(fh, "readinto", None), getattr(fh, "read", None)
        if self._readinto is None and self._read is None:
            raise TypeError("a YUV4MPEG2 stream needs a binary file object with readinto or read")
        self.seconds, self.bytes = 0.0, 0
        try:          # a pipe of the default 64 KiB wakes reader and writer 48 times per 1080p frame: ask for 1 MiB (refusals do not matter)
            import fcntl
            fd = fh.fileno()
            if stat.S_ISFIFO(os.fstat(fd).st_mode):
                fcntl.fcntl(fd, getattr(fcntl, "F_SETPIPE_SZ", 1031), 1 << 20)
        except Exception:
            pass

    def fill(self, buf):
        """Reads until buf (a writable buffer of bytes) is full or the source ends; returns the bytes got."""
        view = memoryview(buf).cast("B")
        want, got = len(view), 0
        t0 = time.perf_counter()
        while got < want:
            if self._readinto is not None:
                k = self._readinto(view[got:])
            else:
                data = self._read(want - got)
                k = None if data is None else len(data)
                if k:
                    view[got:got + k] = data
            if k is None:
                raise ValueError("a YUV4MPEG2 stream needs a blocking source: %s has no data ready" % self.name)
            if k == 0:
                break
            got += k
        self.seconds += time.perf_counter() - t0
        self.bytes += got
        return got

    def close(self):
        if self._own is not None:
            self._own.close()
            self._own = None


class Y4MStreamReader:
    """The reference FrameReader's surface and bookkeeping (io_video.py:13-82) over a YUV4MPEG2 source that can only be read once,
    front to back, and whose length nobody knows: a pipe (`ffmpeg ... -f yuv4mpegpipe - | ...`), a FIFO, a descriptor, a file object.
    For the same bytes every get_n_frames call returns what the file readers' (Y4MReader / YuvReader) return, counters included.

    total_frames / end_frame are properties: exact once the source has ended or when end= was given, else the number of frames
    known to exist -- and reading them looks one FRAME marker ahead (it may block), so they are at least one more than the frames
    handed out while the video goes on.  `while queue.frames_processed < reader.total_frames` therefore decides like over a file.

    crop_region (here or by set_region before the first window): frames are handed out as Yuv420RectFrame / YuvRectFrame holding
    held_rect(...) only; whole frames (Yuv420Frame / YuvFrame) otherwise.  The first frame stays available in full through
    read_frame(0, increment=False) until the first window has been handed out (generate_regions needs it).

    ahead: windows read by a background thread beyond the one handed out (counted in frames of the last get_n_frames(n)); 0 reads
    in the caller's thread, and never more than one FRAME marker beyond the last frame handed out.  read_seconds / read_bytes: time
    in, and bytes from, the source's read calls."""

    def __init__(self, source, start=0, end=0, full_range=None, crop_region=None, min_seg_size=(24, 24), ahead=1, interlaced=None):
        self._src = _ByteSource(source)
        self.filepath = source if isinstance(source, (str, bytes)) or hasattr(source, "__fspath__") else self._src.name
        try:
            head = bytearray(len(MAGIC))
            if self._src.fill(head) < len(MAGIC) or bytes(head) != MAGIC:
                raise ValueError("not a YUV4MPEG2 file: %s" % self._src.name)
            one = bytearray(1)
            while self._src.fill(one) == 1 and one != b"\n":
                head += one
                if len(head) >= 4096:
                    break
            if one != b"\n":
                raise ValueError("the YUV4MPEG2 header line does not end: %s" % self._src.name)
            width, height, num, den, fmt, self.field_order = (_parse_header(bytes(head), general=True, interlaced=interlaced) + ("p",))[:6]
        except BaseException:
            self._src.close()
            raise
        self._header_bytes = len(head) + 1
        if full_range is not None:
            fmt = fmt[:4] + (bool(full_range),)
        self.width, self.height, self.rate, self.fps = width, height, (num, den), num / den
        self.mono, self.subsampling, self.bits, self.full_range = fmt[0], (fmt[1], fmt[2]), fmt[3], fmt[4]
        self._plain420 = fmt[:4] == (False, 1, 1, 8) and not fmt[4]          # the formats open_y4m gives Y4MReader: Yuv420Frame
        self._sample = 2 if self.bits > 8 else 1
        sx, sy = self.subsampling
        self._cshape = (((height - 1) >> sy) + 1, ((width - 1) >> sx) + 1)
        self._luma = width * height * self._sample
        self._chroma = 0 if self.mono else self._cshape[0] * self._cshape[1] * self._sample
        self._body_bytes = self._luma + 2 * self._chroma
        self.start_frame, self._end = int(start), int(end)
        self.next_frame_number = self.start_frame
        self.frame_shape = (height, width, 3)
        self.last_read_frame, self.frames_read, self.read_errors = None, 0, 0
        self._midnight = datetime.datetime.combine(datetime.date.today(), datetime.time())
        self.ahead = max(int(ahead), 0)
        # where the source stands: pictures consumed, whether the next one's FRAME marker is consumed too, whether it has ended
        self._decoded, self._marked, self._eof, self._fail = 0, False, False, None
        self._scratch = None                       # one whole picture: what is read past (frames before start, pixels outside the rectangle)
        self._first, self._first_wanted = None, True
        self._second, self._keep_second = None, self.field_order in ("t", "b")          # (an interlaced video's first picture needs two frames)
        # the producer's own counters (it runs ahead of what has been handed out): next number, frames read, read errors, last frame, shape
        self._cur = [self.start_frame, 0, 0, None, self.frame_shape]
        self._cv = threading.Condition()
        self._items, self._cap = deque(), 1
        self._thread, self._done, self._stop, self._closed = None, False, False, False
        self._handed = False
        self.crop_region, self.min_seg_size, self._rect = None, tuple(min_seg_size), None
        if crop_region is not None:
            self.set_region(crop_region, min_seg_size)

    # ---- what is kept of a picture ----
    def set_region(self, crop_region, min_seg_size=(24, 24)):
        """Frames handed out from here on hold only what the counting loop over crop_region reads (held_rect).  Before the first
        window; later only the region already set is accepted."""
        region = [tuple(int(c) for c in crop_region[0]), tuple(int(c) for c in crop_region[1])]
        size = tuple(int(s) for s in min_seg_size)
        if self._handed or self._thread is not None:
            if (region, size) != (self.crop_region, self.min_seg_size):
                raise ValueError("the region of a stream reader is set before its first window is read")
            return
        self.crop_region, self.min_seg_size = region, size
        ya, yb, xa, xb = held_rect((self.height, self.width), region, size, self.subsampling)
        if yb <= ya or xb <= xa:
            raise ValueError("the crop region lies outside the %dx%d picture" % (self.width, self.height))
        self._rect = (ya, yb, xa, xb)

    def _planes(self, buf):
        """(y, u, v) views of a buffer that holds one whole picture."""
        def plane(at, nbytes, shape):
            raw = buf[at:at + nbytes]
            return (raw.view("<u2") if self._sample == 2 else raw).reshape(shape)
        y = plane(0, self._luma, (self.height, self.width))
        if self.mono:
            return y, None, None
        return y, plane(self._luma, self._chroma, self._cshape), plane(self._luma + self._chroma, self._chroma, self._cshape)

    def _rect_shapes(self):
        ya, yb, xa, xb = self._rect
        sx, sy = self.subsampling
        return (yb - ya, xb - xa), (((yb - 1) >> sy) + 1 - (ya >> sy), ((xb - 1) >> sx) + 1 - (xa >> sx))

    def _rect_frame(self, y, u, v):
        origin = (self._rect[0], self._rect[2])
        if self._plain420:
            return Yuv420RectFrame(y, u, v, origin, self.frame_shape)
        return YuvRectFrame(y, u, v, origin, self.frame_shape, self.subsampling, self.bits, self.full_range)

    def _held(self, planes):
        """The frame handed out for a picture whose whole planes are `planes`: they themselves, or a copy of the rectangle."""
        y, u, v = planes
        if self._rect is None:
            if self._plain420:
                return Yuv420Frame(y, u, v)
            return YuvFrame(y, u, v, self.subsampling, self.bits, self.full_range)
        ya, yb, xa, xb = self._rect
        sx, sy = self.subsampling
        (lh, lw), (ch, cw) = self._rect_shapes()
        dt = y.dtype
        block = np.empty(lh * lw + (0 if self.mono else 2 * ch * cw), dt)          # one allocation per frame
        hy = block[:lh * lw].reshape(lh, lw)
        np.copyto(hy, y[ya:yb, xa:xb])
        if self.mono:
            return self._rect_frame(hy, None, None)
        hu = block[lh * lw:lh * lw + ch * cw].reshape(ch, cw)
        hv = block[lh * lw + ch * cw:].reshape(ch, cw)
        np.copyto(hu, u[ya >> sy:(ya >> sy) + ch, xa >> sx:(xa >> sx) + cw])
        np.copyto(hv, v[ya >> sy:(ya >> sy) + ch, xa >> sx:(xa >> sx) + cw])
        return self._rect_frame(hy, hu, hv)

    def _null(self):
        """The reference's null frame (io_video.py:40-44) in the form this reader's frames have."""
        if self._rect is None:
            if self._plain420:
                return Yuv420Frame.null(self.height, self.width)
            return YuvFrame.null(self.height, self.width, self.subsampling, self.bits, self.full_range, self.mono)
        (lh, lw), cshape = self._rect_shapes()
        dt = np.uint16 if self._sample == 2 else np.uint8
        y = np.zeros((lh, lw), dt)
        if self.mono:
            return self._rect_frame(y, None, None)
        return self._rect_frame(y, np.full(cshape, 128 << (self.bits - 8), dt), np.full(cshape, 128 << (self.bits - 8), dt))

    # ---- the source, picture by picture (one thread at a time: the read-ahead thread while it runs, else the caller's) ----
    def _known(self):
        return self._decoded + (1 if self._marked else 0)

    def _wake(self):
        with self._cv:
            self._cv.notify_all()

    def _mark(self):
        """Consumes the next picture's FRAME marker; False when the source has ended in front of it.  A marker that is cut or wrong
        counts as a picture: reading that picture raises."""
        if self._eof:
            return False
        if self._marked:
            return True
        mark = bytearray(len(FRAME_MARK))
        got = self._src.fill(mark)
        if got == 0:
            self._eof = True
            self._wake()
            return False
        if got < len(FRAME_MARK):
            self._fail = ValueError("%s ends inside the FRAME marker of frame %d: %d of its %d bytes arrived"
                                    % (self._src.name, self._decoded, got, len(FRAME_MARK)))
        elif bytes(mark[:5]) == b"FRAME" and mark[5] != 0x0A:
            self._fail = ValueError("FRAME headers with parameters are not supported: %s" % self._src.name)
        elif bytes(mark) != FRAME_MARK:
            self._fail = ValueError("no FRAME marker %s: %s" % ("after the header" if self._decoded == 0 else "in front of frame %d" % self._decoded,
                                                                self._src.name))
        self._marked = True
        self._wake()
        return True

    def _body(self, keep):
        """Consumes the marked picture's planes; keep: returns the frame to hand out, else the picture is read past."""
        if self._fail is not None:
            raise self._fail
        first = self._decoded == 0 and self._first_wanted
        second = self._decoded == 1 and self._first_wanted and self._keep_second
        if first or second or (keep and self._rect is None):
            buf = np.empty(self._body_bytes, np.uint8)          # a frame that is held whole owns its buffer
        else:
            if self._scratch is None:
                self._scratch = np.empty(self._body_bytes, np.uint8)
            buf = self._scratch
        got = self._src.fill(buf)
        if got < self._body_bytes:
            plane = "luma" if got < self._luma else "chroma"
            self._fail = ValueError("%s ends inside frame %d (in its %s): %d of its %d bytes arrived"
                                    % (self._src.name, self._decoded, plane, got, self._body_bytes))
            raise self._fail
        planes = self._planes(buf)
        if first:
            self._first = planes
        if second:
            self._second = planes
        self._marked = False
        self._decoded += 1
        self._wake()
        return self._held(planes) if keep else None

    def _seek(self, k):
        """Reads past the pictures in front of picture k and consumes its marker; False when the source ends before it."""
        while self._mark():
            if self._decoded >= k:
                return True
            self._body(False)
        return False

    def _picture(self, k):
        """The frame to hand out for picture k (the pictures are asked for in order), None when the source ends before it."""
        if k < self._decoded:
            if k == 0 and self._first is not None:          # read early by read_frame(0, increment=False)
                return self._held(self._first)
            if k == 1 and self._second is not None:
                return self._held(self._second)
            raise ValueError("a stream cannot go back to frame %d" % k)
        return self._body(True) if self._seek(k) else None

    def _produce(self):
        """The next (frame, number, timestamp, counters after it) of get_frame's sequence (io_video.py:40-59), None when a null frame
        follows.  Counters change only once the frame is there."""
        nxt, nread, nerr, last, shape = self._cur
        if nxt < self.start_frame or (self._end > 0 and nxt > self._end):
            return None
        frame = self._picture(nxt)
        if frame is None and self._end == 0 and nxt > self._decoded:          # (the source has ended: _decoded is the frame count)
            return None
        stamp = self.frame_number_to_timestamp(nxt)
        if frame is None:
            frame, nerr = last, nerr + 1                                       # :51-53
        else:
            last, nread, shape = frame, nread + 1, frame.shape
        self._cur = [nxt + 1, nread, nerr, last, shape]
        return frame, nxt, stamp, (nxt + 1, nread, nerr, last, shape)

    # ---- reading ahead ----
    def _run(self):
        try:
            while True:
                with self._cv:
                    self._cv.wait_for(lambda: self._stop or len(self._items) < max(self._cap, 1))
                    if self._stop:
                        break
                item = self._produce()
                if item is None:
                    break
                with self._cv:
                    self._items.append(item)
                    self._cv.notify_all()
        except BaseException as exc:                  # surfaces in the get_n_frames call that needed the frame
            with self._cv:
                self._items.append(exc)
        finally:
            with self._cv:
                self._done = True
                self._cv.notify_all()

    def _take(self):
        if self._thread is not None:
            with self._cv:
                self._cv.wait_for(lambda: self._items or self._done)
                if self._items:
                    item = self._items[0]
                    if isinstance(item, BaseException):
                        raise item
                    self._items.popleft()
                    self._cv.notify_all()
                    return item
        return self._produce()          # no thread, or it has finished: null frames follow (or the error it met)

    # ---- the reference reader's surface ----
    @property
    def end_frame(self):
        if self._end > 0:
            return self._end
        want = self.next_frame_number + 1
        if self._thread is not None and not self._done:
            with self._cv:
                self._cv.wait_for(lambda: self._eof or self._done or self._known() >= want)
        if (self._thread is None or self._done) and not self._eof and self._fail is None and self._known() < want:
            try:
                self._seek(want - 1)
            except ValueError:
                pass                                  # a picture that cannot be read: get_n_frames raises when it is asked for
        return self._known()

    @property
    def total_frames(self):
        return self.end_frame - self.start_frame

    def frame_number_to_timestamp(self, frame_number):
        from .io_data import frame_timestamp_ns
        return self._midnight + datetime.timedelta(microseconds=frame_timestamp_ns(frame_number, self.fps) // 1000)

    def read_frame(self, frame_number, increment=True):
        """The video's first frame in full, until the first window has been handed out (swift_counting_algorithm reads it for
        generate_regions); None when the video has no frame.  A stream has no other frame to offer out of turn -- but the second one
        of an interlaced video (read_frame(1, increment=False)), which its first picture needs."""
        if frame_number == 1 and self._keep_second and not (increment or self._handed or self._thread is not None):
            if self.read_frame(0, increment=False) is not None and self._second is None and self._decoded == 1 and self._seek(1):
                self._body(False)
            return None if self._second is None else self._whole(self._second)
        if frame_number != 0 or increment or self._handed or self._thread is not None:
            raise ValueError("a stream reader only offers read_frame(0, increment=False), before its first window")
        if self._first is None and self._decoded == 0 and self._seek(0):
            self._body(False)
        return None if self._first is None else self._whole(self._first)

    def _whole(self, planes):
        y, u, v = planes
        if self._plain420:
            return Yuv420Frame(y, u, v)
        return YuvFrame(y, u, v, self.subsampling, self.bits, self.full_range)

    def _hand(self, item):
        if item is None:
            return self._null(), -1, "00:00:00.000"          # (:40-44)
        frame, number, stamp, (self.next_frame_number, self.frames_read, self.read_errors, self.last_read_frame, self.frame_shape) = item
        return frame, number, stamp

    def get_frame(self, frame_number=None):
        if frame_number is not None and frame_number != self.next_frame_number:
            raise ValueError("a stream reader hands its frames out in order (next: %d)" % self.next_frame_number)
        frames, numbers, stamps = self.get_n_frames(1)
        return frames[0], numbers[0], stamps[0]

    def get_n_frames(self, n):
        if self._closed:
            raise ValueError("the stream reader is closed")
        if self.ahead > 0 and self._thread is None:
            self._cap = self.ahead * int(n)
            self._thread = threading.Thread(target=self._run, name="swk-y4m-read", daemon=True)
            self._thread.start()
        elif self._thread is not None:
            with self._cv:
                self._cap = max(self.ahead, 1) * int(n)
                self._cv.notify_all()
        frames, numbers, stamps = [], [], []
        for _ in range(n):
            f, k, t = self._hand(self._take())
            frames.append(f); numbers.append(k); stamps.append(t)
        self._handed = True
        self._first, self._first_wanted = None, False
        if self.next_frame_number > 1:               # (a second frame read early stays until it has been handed out)
            self._second = None
        return frames, numbers, stamps

    @property
    def read_seconds(self):
        return self._src.seconds

    @property
    def read_bytes(self):
        return self._src.bytes

    def close(self):
        """Stops the read-ahead thread and closes what the reader opened itself (not standard input, not a file object or a
        descriptor it was given)."""
        if self._closed:
            return
        self._closed = True
        with self._cv:
            self._stop = True
            self._cv.notify_all()
        if self._thread is not None:
            self._thread.join(2.0)
        if self._thread is None or not self._thread.is_alive():          # (a thread still waiting in read keeps its descriptor)
            self._src.close()
        self._items.clear()
        self._first = self._second = self._scratch = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

def _is_stream(source):
    """True for a source open_y4m reads front to back: "-", a file descriptor, a binary file object, the path of a FIFO."""
    if isinstance(source, bool):
        return False
    if isinstance(source, int) or (isinstance(source, str) and source == "-"):
        return True
    if isinstance(source, (str, bytes)) or hasattr(source, "__fspath__"):
        try:
            return stat.S_ISFIFO(os.stat(source).st_mode)
        except OSError:
            return False          # (the file reader names what is wrong with the path)
    return hasattr(source, "readinto") or hasattr(source, "read")


def open_y4m(source, start=0, end=0, full_range=None, crop_region=None, min_seg_size=(24, 24), ahead=1, interlaced=None):
    """The reader of a YUV4MPEG2 video.  The path of a regular file: Y4MReader for an 8-bit 4:2:0 limited-range progressive file,
    YuvReader for every other supported format (crop_region, min_seg_size and ahead do not apply to them).  A source that can only
    be read once, front to back -- the path of a FIFO, "-" (standard input), a file descriptor, a binary file object --:
    Y4MStreamReader.  full_range: None = what the header says, True / False override it.  interlaced: None refuses interlaced files
    (It / Ib) by name; any other value accepts them -- the reader's field_order is then "p", "t" or "b", and its frames are the stored,
    woven frames (deinterlace.DeinterlacingReader makes pictures of them)."""
    if _is_stream(source):
        return Y4MStreamReader(source, start, end, full_range, crop_region, min_seg_size, ahead, interlaced)
    path = source
    with open(path, "rb") as fh:
        head = fh.read(4096)
    if not head.startswith(MAGIC):
        raise ValueError("not a YUV4MPEG2 file: %s" % path)
    eol = head.find(b"\n")
    if eol < 0:
        raise ValueError("the YUV4MPEG2 header line does not end: %s" % path)
    fmt = _parse_header(head[:eol], general=True, interlaced=interlaced)[4]
    full = fmt[4] if full_range is None else bool(full_range)
    if fmt[:4] == (False, 1, 1, 8) and not full:
        return Y4MReader(path, start, end, interlaced)
    return YuvReader(path, start, end, full, interlaced)


class Y4MWriter:
    """Writes a YUV4MPEG2 file of progressive frames (interlaced="t" / "b": of woven frames whose top / bottom field is the earlier one,
    tagged It / Ib): append(y, u, v) per frame (append(y) for mono), close() (or use it as a context
    manager).  fps: a number (30, 29.97...: stored as the nearest fraction) or a (numerator, denominator) pair.  chroma: "420",
    "422", "444", "411" or "mono"; bits: 8, 9, 10, 12, 14 or 16 (uint16 planes, LSB-aligned, written little-endian); full_range adds
    XCOLORRANGE=FULL.  The defaults write 8-bit 4:2:0."""

    def __init__(self, path, width, height, fps, chroma="420", bits=8, full_range=False, interlaced="p"):
        from fractions import Fraction
        if interlaced not in ("p", "t", "b"):
            raise ValueError('interlaced is "p" (progressive), "t" (top field first) or "b" (bottom field first)')
        if isinstance(fps, (tuple, list)):
            num, den = int(fps[0]), int(fps[1])
        else:
            frac = Fraction(fps).limit_denominator(100000)
            num, den = frac.numerator, frac.denominator
        if width < 1 or height < 1 or num < 1 or den < 1:
            raise ValueError("width, height and fps must be positive")
        if chroma == "mono":
            tag = {v: k for k, v in _MONO_DEPTHS.items()}.get(bits)
        else:
            suffix = {v: k for k, v in _DEPTHS.items()}.get(bits)
            tag = None if chroma not in _SUBSAMPLING or suffix is None else ("420jpeg" if (chroma, bits) == ("420", 8) else chroma + suffix)
        if tag is None:
            raise ValueError("no YUV4MPEG2 tag for chroma %r at %r bits" % (chroma, bits))
        self.width, self.height, self.frames = int(width), int(height), 0
        self.mono, self.bits = chroma == "mono", int(bits)
        self.sx, self.sy = (0, 0) if self.mono else _SUBSAMPLING[chroma]
        self._fh = open(path, "wb")
        self._fh.write(b"%s W%d H%d F%d:%d I%s A0:0 C%s%s\n" % (MAGIC, self.width, self.height, num, den, interlaced.encode("ascii"),
                                                               tag.encode("ascii"), b" XCOLORRANGE=FULL" if full_range else b""))

    def append(self, y, u=None, v=None):
        ch, cw = ((self.height - 1) >> self.sy) + 1, ((self.width - 1) >> self.sx) + 1
        given = (y,) if self.mono else (y, u, v)
        if any(p is None for p in given) or (self.mono and (u is not None or v is not None)):
            raise ValueError("a mono frame is y alone, any other frame y, u and v")
        planes = [np.ascontiguousarray(p, "<u2" if self.bits > 8 else np.uint8) for p in given]
        if planes[0].shape != (self.height, self.width) or any(p.shape != (ch, cw) for p in planes[1:]):
            raise ValueError("a %dx%d frame needs y (%d, %d) and u, v (%d, %d)" % (self.width, self.height, self.height, self.width, ch, cw))
        self._fh.write(FRAME_MARK)
        for p in planes:
            self._fh.write(p.tobytes())
        self.frames += 1

    def append_bgr(self, frames, ctx=None):
        """BGR frames (F, H, W, 3) or one (H, W, 3), uint8 (a numpy array, or a torch tensor on the context's GPU), converted to 4:2:0 on
        the GPU (swk_bgr_to_yuv420: cv2's COLOR_BGR2YUV_I420 restated, chroma from each cell's top-left pixel) and appended.  For an
        8-bit 4:2:0 writer.  ctx: a _lib.Context (None: GPU 0's default context)."""
        if self.mono or (self.sx, self.sy) != (1, 1) or self.bits != 8:
            raise ValueError("append_bgr writes 8-bit 4:2:0")
        if len(frames.shape) == 3:
            frames = frames[None]
        if tuple(frames.shape[1:]) != (self.height, self.width, 3):
            raise ValueError("a %dx%d writer needs BGR frames (%d, %d, 3)" % (self.width, self.height, self.height, self.width))
        if ctx is None:
            from . import _lib
            ctx = _lib.default_context(0)
        y, u, v = ctx.bgr_to_yuv420(frames)
        for k in range(len(y)):
            self.append(y[k], u[k], v[k])

    def close(self):
        if self._fh is not None:
            self._fh.close()
            self._fh = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
