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
limited range or, with XCOLORRANGE=FULL, full range.  Interlaced files, C444alpha and FRAME lines with parameters are refused by
name."""
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


def _parse_header(line, general=False):
    """(width, height, fps numerator, denominator) of a YUV4MPEG2 stream header line (without its newline).  general: every format
    of open_y4m is accepted, and the result ends with its (mono, sx, sy, bits, full_range)."""
    tags = line.split(b" ")
    if tags[0] != MAGIC:
        raise ValueError("not a YUV4MPEG2 file")
    width = height = rate = None
    fmt, full = (False, 1, 1, 8), False
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
    if general:
        return width, height, rate[0], rate[1], fmt + (full,)
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

    def __init__(self, path, start=0, end=0, full_range=None):
        with open(path, "rb") as fh:
            head = fh.read(4096)
        if not head.startswith(MAGIC):
            raise ValueError("not a YUV4MPEG2 file: %s" % path)
        eol = head.find(b"\n")
        if eol < 0:
            raise ValueError("the YUV4MPEG2 header line does not end: %s" % path)
        width, height, num, den, fmt = _parse_header(head[:eol], general=True)
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


def open_y4m(path, start=0, end=0, full_range=None):
    """The reader of a .y4m file: Y4MReader for an 8-bit 4:2:0 limited-range progressive file, YuvReader for every other supported
    format.  full_range: None = what the header says, True / False override it."""
    with open(path, "rb") as fh:
        head = fh.read(4096)
    if not head.startswith(MAGIC):
        raise ValueError("not a YUV4MPEG2 file: %s" % path)
    eol = head.find(b"\n")
    if eol < 0:
        raise ValueError("the YUV4MPEG2 header line does not end: %s" % path)
    fmt = _parse_header(head[:eol], general=True)[4]
    full = fmt[4] if full_range is None else bool(full_range)
    if fmt[:4] == (False, 1, 1, 8) and not full:
        return Y4MReader(path, start, end)
    return YuvReader(path, start, end, full)


class Y4MWriter:
    """Writes a YUV4MPEG2 file of progressive frames: append(y, u, v) per frame (append(y) for mono), close() (or use it as a context
    manager).  fps: a number (30, 29.97...: stored as the nearest fraction) or a (numerator, denominator) pair.  chroma: "420",
    "422", "444", "411" or "mono"; bits: 8, 9, 10, 12, 14 or 16 (uint16 planes, LSB-aligned, written little-endian); full_range adds
    XCOLORRANGE=FULL.  The defaults write 8-bit 4:2:0."""

    def __init__(self, path, width, height, fps, chroma="420", bits=8, full_range=False):
        from fractions import Fraction
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
        self._fh.write(b"%s W%d H%d F%d:%d Ip A0:0 C%s%s\n" % (MAGIC, self.width, self.height, num, den, tag.encode("ascii"),
                                                              b" XCOLORRANGE=FULL" if full_range else b""))

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

    def close(self):
        if self._fh is not None:
            self._fh.close()
            self._fh = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
