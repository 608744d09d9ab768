"""io_y4m.Y4MStreamReader (a YUV4MPEG2 source read once, front to back, length unknown) against the file readers over the same
bytes, call by call; its look-ahead discipline, its rectangle-holding frames, its refusals; the argument parsing of
python -m swiftwatcher_amd.  No GPU."""
import hashlib
import io
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMATS = {"420": dict(chroma="420", bits=8, full_range=False), "422p10": dict(chroma="422", bits=10, full_range=False),
           "mono_full": dict(chroma="mono", bits=8, full_range=True)}
COUNTS = (1, 20, 21, 22, 42, 43)
N = 21


def _write(path, fmt, count, W=36, H=22, seed=0):
    from swiftwatcher_amd.io_y4m import Y4MWriter, _SUBSAMPLING
    rng = np.random.default_rng(seed + count)
    kw = FORMATS[fmt]
    hi = 1 << kw["bits"]
    dt = np.uint16 if kw["bits"] > 8 else np.uint8
    with Y4MWriter(path, W, H, (30000, 1001), **kw) as w:
        for _ in range(count):
            y = rng.integers(0, hi, (H, W)).astype(dt)
            if kw["chroma"] == "mono":
                w.append(y)
            else:
                sx, sy = _SUBSAMPLING[kw["chroma"]]
                cs = (((H - 1) >> sy) + 1, ((W - 1) >> sx) + 1)
                w.append(y, rng.integers(0, hi, cs).astype(dt), rng.integers(0, hi, cs).astype(dt))
    with open(path, "rb") as fh:
        return fh.read()


@pytest.fixture(scope="module")
def clips(tmp_path_factory):
    """{(format, frame count): (path, bytes)} at 36 x 22"""
    d = tmp_path_factory.mktemp("y4m_stream")
    out = {}
    for fmt in FORMATS:
        for count in COUNTS:
            path = str(d / ("%s_%d.y4m" % (fmt, count)))
            out[fmt, count] = (path, _write(path, fmt, count))
    return out


def _pixels(frame):
    return None if frame is None else np.asarray(frame)


def _state(reader, names):
    return tuple(getattr(reader, k) for k in names)


STATE = ("next_frame_number", "frames_read", "read_errors", "frame_shape", "start_frame", "fps", "width", "height", "rate")


def _play(reader, names, n=N):
    """The counting loop's reads: windows until `frames_processed < total_frames` turns false."""
    log, processed = [], 0
    while processed < reader.total_frames:
        frames, numbers, stamps = reader.get_n_frames(n)
        processed += sum(1 for k in numbers if k >= 0)          # FrameQueue.pop_frame: null frames are not counted
        log.append(([(type(f).__name__, _pixels(f)) for f in frames], list(numbers), [str(s) for s in stamps], _state(reader, names),
                    (processed, reader.total_frames, reader.end_frame)))
        assert len(log) < 10
    return log


def _same_log(got, want, length_known=False):
    """Every window's triples and counters; total_frames / end_frame after every call: the file's where the length is known (end=
    given, or the source has ended), else the frames known to exist -- at least one more than those handed out, never too many."""
    assert len(got) == len(want)
    for (gf, gn, gs, gc, (processed, total, end)), (wf, wn, ws, wc, (_, wtotal, wend)) in zip(got, want):
        assert gn == wn and gs == ws and gc == wc
        start = gc[STATE.index("start_frame")]
        assert total == end - start
        if length_known or processed >= wtotal:
            assert (total, end) == (wtotal, wend)
        else:
            assert processed + 1 <= total <= wtotal
        for (gt, gp), (wt, wp) in zip(gf, wf):
            assert gt == wt
            assert (gp is None and wp is None) or np.array_equal(gp, wp)


def _names(file_reader):
    return STATE + tuple(k for k in ("mono", "subsampling", "bits", "full_range") if hasattr(file_reader, k))


# ------------------------------------------------------------------------------------------ 1. equality with the file reader
@pytest.mark.parametrize("ahead", [0, 1])
@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("fmt", list(FORMATS))
def test_equals_the_file_reader_call_by_call(clips, fmt, count, ahead):
    from swiftwatcher_amd.io_y4m import Y4MStreamReader, open_y4m
    path, data = clips[fmt, count]
    on_file = open_y4m(path)
    names = _names(on_file)
    want = _play(on_file, names)
    stream = open_y4m(io.BytesIO(data), ahead=ahead)
    assert isinstance(stream, Y4MStreamReader)
    got = _play(stream, names)
    _same_log(got, want)
    assert len(got) == -(-count // N) and stream.total_frames == count
    # past the loop's end: the frame one past the end once, if it has not been served yet, then null frames numbered -1
    f, w = stream.get_n_frames(3), on_file.get_n_frames(3)
    assert f[1] == w[1] and [str(s) for s in f[2]] == [str(s) for s in w[2]] and _state(stream, names) == _state(on_file, names)
    assert all(np.array_equal(_pixels(a), _pixels(b)) for a, b in zip(f[0], w[0]))
    assert f[1][1:] == [-1, -1] and f[2][2] == "00:00:00.000" and not np.asarray(f[0][2]).any()
    stream.close()


@pytest.mark.parametrize("ahead", [0, 2])
@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("fmt", list(FORMATS))
def test_start_and_end(clips, fmt, count, ahead):
    from swiftwatcher_amd.io_y4m import open_y4m
    path, data = clips[fmt, count]
    on_file = open_y4m(path, start=5, end=30)
    names = _names(on_file)
    want = _play(on_file, names)
    source = io.BytesIO(data)
    stream = open_y4m(source, start=5, end=30, ahead=ahead)
    assert stream.total_frames == 25 and stream.end_frame == 30
    _same_log(_play(stream, names), want, length_known=True)
    stream.close()
    if count > 31:          # frames 5 .. 30 are served (the range test is inclusive): the source has not reached its end
        step = (len(data) - stream._header_bytes) // count
        assert source.tell() == stream._header_bytes + 31 * step < len(data)


# ------------------------------------------------------------------------------------------ 2. source kinds
def _feed(fd, data, chunk):
    try:
        for at in range(0, len(data), chunk):
            os.write(fd, data[at:at + chunk])
    except OSError:
        pass
    finally:
        os.close(fd)


@pytest.mark.parametrize("chunk", [1, 7, 4097])
@pytest.mark.parametrize("kind", ["descriptor", "file object"])
def test_os_pipe_with_short_reads(clips, chunk, kind):
    from swiftwatcher_amd.io_y4m import open_y4m
    path, data = clips["422p10", 22]
    on_file = open_y4m(path)
    names = _names(on_file)
    want = _play(on_file, names)
    r, w = os.pipe()
    feeder = threading.Thread(target=_feed, args=(w, data, chunk), daemon=True)
    feeder.start()
    source = r if kind == "descriptor" else os.fdopen(r, "rb", buffering=0)
    stream = open_y4m(source)
    _same_log(_play(stream, names), want)
    stream.close()
    feeder.join(10)
    assert not feeder.is_alive()
    if kind == "descriptor":
        os.fstat(r)                  # a descriptor that was handed in is left open
        os.close(r)
    else:
        assert not source.closed     # so is a file object
        source.close()


def test_object_with_read_only(clips):
    from swiftwatcher_amd.io_y4m import open_y4m

    class OnlyRead:
        def __init__(self, data):
            self._fh = io.BytesIO(data)

        def read(self, n):
            return self._fh.read(min(n, 1000))          # short reads

    path, data = clips["420", 43]
    on_file = open_y4m(path)
    names = _names(on_file)
    stream = open_y4m(OnlyRead(data))
    _same_log(_play(stream, names), _play(on_file, names))
    stream.close()


def test_fifo_path(clips, tmp_path):
    from swiftwatcher_amd.io_y4m import Y4MStreamReader, open_y4m
    path, data = clips["mono_full", 42]
    fifo = str(tmp_path / "video.y4m")
    os.mkfifo(fifo)

    def feed():
        _feed(os.open(fifo, os.O_WRONLY), data, 5000)
    feeder = threading.Thread(target=feed, daemon=True)
    feeder.start()
    on_file = open_y4m(path)
    names = _names(on_file)
    stream = open_y4m(fifo)
    assert isinstance(stream, Y4MStreamReader) and stream.filepath == fifo
    _same_log(_play(stream, names), _play(on_file, names))
    stream.close()
    feeder.join(10)
    assert not feeder.is_alive()


CHILD = r"""
import hashlib, sys
import numpy as np
from swiftwatcher_amd import io_y4m
reader = io_y4m.open_y4m("-")
h, processed, windows = hashlib.sha256(), 0, 0
while processed < reader.total_frames:
    frames, numbers, stamps = reader.get_n_frames(21)
    processed += sum(1 for k in numbers if k >= 0)
    windows += 1
    for f, k in zip(frames, numbers):
        h.update(np.asarray(f).tobytes())
        h.update(str(k).encode())
reader.close()
assert not sys.stdin.buffer.closed
print(type(reader).__name__, windows, reader.total_frames, reader.frames_read, reader.read_errors, h.hexdigest())
"""


def test_standard_input_in_a_child_process(clips):
    from swiftwatcher_amd.io_y4m import open_y4m
    path, _ = clips["420", 43]
    on_file = open_y4m(path)
    h, windows = hashlib.sha256(), 0
    for frames, numbers, _, _, _ in _play(on_file, STATE):
        windows += 1
        for (_, px), k in zip(frames, numbers):
            h.update(px.tobytes())
            h.update(str(k).encode())
    with open(path, "rb") as fh:
        done = subprocess.run([sys.executable, "-c", CHILD], stdin=fh, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert done.returncode == 0, done.stderr
    assert done.stdout.split() == ["Y4MStreamReader", str(windows), "43", str(on_file.frames_read), str(on_file.read_errors), h.hexdigest()]


# ------------------------------------------------------------------------------------------ 3. look-ahead discipline
class _Counting:
    def __init__(self, data):
        self._fh, self.consumed = io.BytesIO(data), 0

    def readinto(self, buf):
        got = self._fh.readinto(buf)
        self.consumed += got
        return got


@pytest.mark.parametrize("count", [22, 42])
@pytest.mark.parametrize("fmt", list(FORMATS))
def test_reads_no_more_than_one_frame_ahead(clips, fmt, count):
    from swiftwatcher_amd.io_y4m import open_y4m
    _, data = clips[fmt, count]
    source = _Counting(data)
    stream = open_y4m(source, ahead=0)
    header = stream._header_bytes
    step = (len(data) - header) // count
    assert source.consumed == header
    handed = 0
    for n in (1, 4, 21, 21):
        assert stream.total_frames >= min(handed + 1, count)
        assert source.consumed <= header + handed * step + 6 <= header + (handed + 1) * step          # one FRAME marker ahead
        _, numbers, _ = stream.get_n_frames(n)
        handed = min(handed + n, count)
        assert stream.frames_read == handed
        assert source.consumed <= header + handed * step + 6
    assert stream.total_frames == count and source.consumed == len(data)
    stream.close()


# ------------------------------------------------------------------------------------------ 4. rectangle frames
RECTS = [([(5, 3), (21, 15)], (6, 6)), ([(20, 10), (37, 23)], (6, 6)), ([(9, 7), (30, 20)], (24, 24)), ([(1, 1), (8, 6)], (2, 2))]


@pytest.mark.parametrize("ahead", [0, 1])
@pytest.mark.parametrize("crop,min_seg", RECTS)
@pytest.mark.parametrize("fmt", list(FORMATS))
def test_frames_hold_the_grown_rectangle(tmp_path, fmt, crop, min_seg, ahead):
    from swiftwatcher_amd.io_roi_stream import margin_rect
    from swiftwatcher_amd.io_y4m import held_rect, open_y4m
    W, H, count = 37, 23, 8
    path = str(tmp_path / "odd.y4m")
    data = _write(path, fmt, count, W, H, seed=3)
    on_file = open_y4m(path)
    stream = open_y4m(io.BytesIO(data), crop_region=crop, min_seg_size=min_seg, ahead=ahead)
    first = stream.read_frame(0, increment=False)
    assert type(first) is type(on_file.read_frame(0, increment=False)) and np.array_equal(np.asarray(first), np.asarray(on_file.read_frame(0, increment=False)))
    sx, sy = stream.subsampling
    ya, yb, xa, xb = margin_rect((H, W), crop, min_seg)
    ly0, lx0 = (ya >> sy) << sy, (xa >> sx) << sx
    assert held_rect((H, W), crop, min_seg, (sx, sy)) == (ly0, yb, lx0, xb)
    for _ in range(2):
        got, numbers, _ = stream.get_n_frames(5)
        want, wnumbers, _ = on_file.get_n_frames(5)
        assert numbers == wnumbers
        for g, w in zip(got, want):
            full = np.asarray(w)
            assert g.shape == full.shape == (H, W, 3) and g.origin == (ly0, lx0)
            assert g.y.shape == (yb - ly0, xb - lx0)
            if g.u is not None:
                assert g.u.shape == g.v.shape == (((yb - 1) >> sy) + 1 - (ya >> sy), ((xb - 1) >> sx) + 1 - (xa >> sx))
            held = sum(p.nbytes for p in (g.y, g.u, g.v) if p is not None)
            whole = sum(p.nbytes for p in (w.y, w.u, w.v) if p is not None)
            assert held <= whole and (held < whole or (ly0, yb, lx0, xb) == (0, H, 0, W))
            for r0, r1, c0, c1 in [(ya, yb, xa, xb), (crop[0][1], crop[1][1], crop[0][0], crop[1][0]), (ya + 1, ya + 2, xb - 1, xb),
                                   (ly0, yb, lx0, xb), (yb - 1, yb, xa, xa + 1)]:
                assert np.array_equal(g[r0:r1, c0:c1], full[r0:r1, c0:c1]), (r0, r1, c0, c1)
            assert g[ya:ya, xa:xb].shape == (0, xb - xa, 3)
            outside = [(ly0 - 1, yb, xa, xb)] * (ly0 > 0) + [(ya, yb + 1, xa, xb)] * (yb < H) + [(ya, yb, lx0 - 1, xb)] * (lx0 > 0) + \
                      [(ya, yb, xa, xb + 1)] * (xb < W)
            everything = (ly0, yb, lx0, xb) == (0, H, 0, W)          # (a region whose margin reaches every edge: the frame holds all)
            assert outside or everything
            for r0, r1, c0, c1 in outside:
                with pytest.raises(IndexError):
                    g[r0:r1, c0:c1]
            if everything:
                assert np.array_equal(np.asarray(g), full)
            else:
                with pytest.raises(IndexError):
                    np.asarray(g)
    with pytest.raises(ValueError):          # the first frame is let go with the first window
        stream.read_frame(0, increment=False)
    stream.close()


def test_set_region_before_the_first_window(tmp_path):
    from swiftwatcher_amd.io_y4m import Yuv420Frame, Yuv420RectFrame, open_y4m
    data = _write(str(tmp_path / "c.y4m"), "420", 6, 37, 23)
    stream = open_y4m(io.BytesIO(data), ahead=0)
    assert type(stream.read_frame(0, increment=False)) is Yuv420Frame
    stream.set_region([(5, 3), (21, 15)], (6, 6))
    frames, numbers, _ = stream.get_n_frames(3)
    assert numbers == [0, 1, 2] and all(type(f) is Yuv420RectFrame and f.origin == (0, 2) for f in frames)
    stream.set_region([(5, 3), (21, 15)], (6, 6))          # the same region again is accepted
    with pytest.raises(ValueError):
        stream.set_region([(4, 3), (21, 15)], (6, 6))
    null = stream.get_n_frames(8)[0][-1]
    assert type(null) is Yuv420RectFrame and not null[3:15, 5:21].any()


# ------------------------------------------------------------------------------------------ 5. refusals
def _layout(data, count):
    header = data.index(b"\n") + 1
    return header, (len(data) - header) // count


@pytest.mark.parametrize("ahead", [0, 1])
@pytest.mark.parametrize("where,word", [("luma", "luma"), ("chroma", "chroma"), ("marker", "FRAME marker")])
def test_a_stream_that_ends_inside_a_frame(clips, where, word, ahead):
    from swiftwatcher_amd.io_y4m import open_y4m
    _, data = clips["420", 22]
    header, step = _layout(data, 22)
    luma = 36 * 22
    cut = header + 3 * step + {"luma": 6 + 100, "chroma": 6 + luma + 50, "marker": 3}[where]
    stream = open_y4m(io.BytesIO(data[:cut]), ahead=ahead)
    assert stream.total_frames >= 1                             # the length is not an error by itself
    frames, numbers, _ = stream.get_n_frames(3)                 # the three whole frames are served
    assert numbers == [0, 1, 2]
    assert stream.total_frames >= 4
    arrived = {"luma": 100, "chroma": luma + 50, "marker": 3}[where]
    with pytest.raises(ValueError, match=r"frame 3\b.*\b%d of its %d bytes" % (arrived, 6 if where == "marker" else step - 6)) as err:
        stream.get_n_frames(21)
    assert word in str(err.value)
    with pytest.raises(ValueError):                             # and again: never silently
        stream.get_n_frames(1)
    stream.close()


def test_refused_streams(clips):
    from swiftwatcher_amd.io_y4m import open_y4m
    path, data = clips["420", 20]
    header, step = _layout(data, 20)
    with_params = data[:header + step] + b"FRAME Ip\n" + data[header + step + 6:]
    stream = open_y4m(io.BytesIO(with_params), ahead=0)
    assert stream.get_n_frames(1)[1] == [0]
    with pytest.raises(ValueError, match="FRAME headers with parameters are not supported"):
        stream.get_n_frames(1)
    no_marker = data[:header] + b"XRAME\n" + data[header + 6:]
    with pytest.raises(ValueError, match="no FRAME marker after the header"):
        open_y4m(io.BytesIO(no_marker)).get_n_frames(1)
    for bad, message in [(data.replace(b" Ip ", b" It ", 1), "interlaced YUV4MPEG2 files are not supported"),
                         (data.replace(b"C420jpeg", b"C444alpha", 1), "this YUV4MPEG2 pixel format is not supported"),
                         (b"RIFF" + data, "not a YUV4MPEG2 file"), (b"YUV4", "not a YUV4MPEG2 file"),
                         (data[:header - 1], "header line does not end")]:
        with pytest.raises(ValueError, match=message):
            open_y4m(io.BytesIO(bad))
        bad_path = path + ".bad"
        with open(bad_path, "wb") as fh:
            fh.write(bad)
        with pytest.raises(ValueError, match=message):          # the file readers say the same
            open_y4m(bad_path)
    with pytest.raises(TypeError):
        open_y4m(object())


def test_a_regular_file_is_read_as_before(clips):
    from swiftwatcher_amd.io_y4m import Y4MReader, YuvReader, open_y4m
    assert type(open_y4m(clips["420", 20][0], crop_region=[(1, 1), (9, 9)], ahead=3)) is Y4MReader
    assert type(open_y4m(clips["422p10", 20][0])) is YuvReader


# ------------------------------------------------------------------------------------------ 6. the entry point's arguments
def test_entry_point_arguments(tmp_path, capsys):
    import json
    from swiftwatcher_amd import __main__ as cli
    assert cli.parse_corners("812,640,1105,642") == ((812, 640), (1105, 642))
    assert cli.parse_corners(" 1, 2,3 ,4") == ((1, 2), (3, 4))
    for bad in ("1,2,3", "1,2,3,x", ""):
        with pytest.raises(ValueError):
            cli.parse_corners(bad)
    args, jobs = cli.plan(["-", "--corners", "10,20,30,21", "--end", "40", "--windows-per-call", "2", "--out", "o"])
    assert jobs == [("-", ((10, 20), (30, 21)))] and (args.start, args.end, args.windows_per_call, args.out, args.device) == (0, 40, 2, "o", 0)
    attributes = tmp_path / "a.json"
    attributes.write_text(json.dumps({"name": "x", "corners": [[3.0, "4"], [50, 6]]}))
    args, jobs = cli.plan(["a.y4m", "-", "--attributes", str(attributes)])
    assert jobs == [("a.y4m", ((3, 4), (50, 6))), ("-", ((3, 4), (50, 6)))]
    # <parent>/<stem>/attributes.json of a file source
    video = tmp_path / "evening.y4m"
    (tmp_path / "evening").mkdir()
    (tmp_path / "evening" / "attributes.json").write_text(json.dumps({"corners": [[7, 8], [90, 10]]}))
    assert cli.plan([str(video)])[1] == [(str(video), ((7, 8), (90, 10)))]
    for argv in (["-"], ["-", "-", "--corners", "1,2,3,4"], [str(tmp_path / "other.y4m")], ["-", "--corners", "1,2,3"],
                 ["-", "--corners", "1,2,3,4", "--attributes", str(attributes)], []):
        with pytest.raises(SystemExit) as err:
            cli.plan(argv)
        assert err.value.code == 2, argv
    capsys.readouterr()
