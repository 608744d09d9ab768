"""YUV4MPEG2 (.y4m) videos: the uncompressed container every decoder can write (`ffmpeg -i in.mp4 out.y4m`) -- a one-line header,
then per frame the six bytes "FRAME\\n" and the Y, U and V planes of an 8-bit 4:2:0 picture.  No codec is involved: the file is
memory-mapped and a frame is three views of the mapping (Yuv420Frame).

The reference sees BGR frames (cv2.VideoCapture, io_video.py:85-125).  A Yuv420Frame stands in for one: it has the BGR frame's
shape and dtype, np.asarray(frame) and frame[rows, columns] give the BGR pixels -- converted on the host, with the arithmetic of
cv2.cvtColor(yuv, COLOR_YUV2BGR_I420) of OpenCV 4.1.0 restated (include/swk.h, swk_yuv420_to_bgr; PARITY UNPINNED) -- so crop_frame,
generate_regions on the first frame, Segment.segment_image and export_segments work unchanged.  The counting loop never converts a
whole frame: data_structures.stack_frames uploads the ROI's luma and chroma (1.5 bytes per pixel instead of 3) and converts on the
GPU (csrc/yuv.hip), bit for bit the same pixels.

Supported: 8-bit 4:2:0, progressive.  4:2:2, 4:4:4, mono, more than 8 bits and interlaced files are refused by name."""
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


def _parse_header(line):
    """(width, height, fps numerator, denominator) of a YUV4MPEG2 stream header line (without its newline)."""
    tags = line.split(b" ")
    if tags[0] != MAGIC:
        raise ValueError("not a YUV4MPEG2 file")
    width = height = rate = None
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
                if value not in ("?", "p"):
                    raise ValueError("interlaced YUV4MPEG2 files are not supported (tag %s)" % tag)
            elif kind == "C":
                if value not in CHROMA_420:
                    raise ValueError("only 8-bit 4:2:0 YUV4MPEG2 files are supported (tag %s)" % tag)
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
    return width, height, rate[0], rate[1]


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

    def __init__(self, path, start=0, end=0):
        with open(path, "rb") as fh:
            head = fh.read(4096)
        if not head.startswith(MAGIC):
            raise ValueError("not a YUV4MPEG2 file: %s" % path)
        eol = head.find(b"\n")
        if eol < 0:
            raise ValueError("the YUV4MPEG2 header line does not end: %s" % path)
        width, height, num, den = _parse_header(head[:eol])
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


class Y4MWriter:
    """Writes a YUV4MPEG2 file of 8-bit 4:2:0 progressive frames: append(y, u, v) per frame, close() (or use it as a context
    manager).  fps: a number (30, 29.97...: stored as the nearest fraction) or a (numerator, denominator) pair."""

    def __init__(self, path, width, height, fps):
        from fractions import Fraction
        if isinstance(fps, (tuple, list)):
            num, den = int(fps[0]), int(fps[1])
        else:
            frac = Fraction(fps).limit_denominator(100000)
            num, den = frac.numerator, frac.denominator
        if width < 1 or height < 1 or num < 1 or den < 1:
            raise ValueError("width, height and fps must be positive")
        self.width, self.height, self.frames = int(width), int(height), 0
        self._fh = open(path, "wb")
        self._fh.write(b"%s W%d H%d F%d:%d Ip A0:0 C420jpeg\n" % (MAGIC, self.width, self.height, num, den))

    def append(self, y, u, v):
        ch, cw = (self.height + 1) // 2, (self.width + 1) // 2
        planes = [np.ascontiguousarray(p, np.uint8) for p in (y, u, v)]
        if planes[0].shape != (self.height, self.width) or planes[1].shape != (ch, cw) or planes[2].shape != (ch, cw):
            raise ValueError("a %dx%d frame needs y (%d, %d) and u, v (%d, %d)" % (self.width, self.height, self.height, self.width, ch, cw))
        self._fh.write(FRAME_MARK)
        for p in planes:
            self._fh.write(p.tobytes())
        self.frames += 1

    def close(self):
        if self._fh is not None:
            self._fh.close()
            self._fh = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
