"""The YUV formats beyond 8-bit 4:2:0 (swiftwatcher_amd/io_y4m.py: open_y4m, YuvReader, YuvFrame, the writer's keywords) without a
GPU: the definition's own properties, header rules, frame bookkeeping, and the host-side conversion of YuvFrame against the
restatement tests/yuv_formats_ref.py.  Every comparison is bit for bit."""
import numpy as np
import pytest

import yuv_formats_ref as ref
import yuv_ref

# C tag -> (mono, (sx, sy), bits)
TAGS = {"420": (False, (1, 1), 8), "420jpeg": (False, (1, 1), 8), "420mpeg2": (False, (1, 1), 8), "420paldv": (False, (1, 1), 8),
        "422": (False, (1, 0), 8), "444": (False, (0, 0), 8), "411": (False, (2, 0), 8), "mono": (True, (0, 0), 8)}
for _d in (9, 10, 12, 14, 16):
    for _name, _ss in (("420", (1, 1)), ("422", (1, 0)), ("444", (0, 0))):
        TAGS["%sp%d" % (_name, _d)] = (False, _ss, _d)
for _d in (9, 10, 12, 16):
    TAGS["mono%d" % _d] = (True, (0, 0), _d)


def _planes(rng, count, H, W, ss=(1, 1), bits=8, mono=False):
    dt = np.uint16 if bits > 8 else np.uint8
    y = rng.integers(0, 1 << bits, (count, H, W)).astype(dt)
    if mono:
        return y, None, None
    cs = ref.chroma_shape(H, W, *ss)
    return y, rng.integers(0, 1 << bits, (count,) + cs).astype(dt), rng.integers(0, 1 << bits, (count,) + cs).astype(dt)


def _raw_file(path, header, planes, mark=b"FRAME\n"):
    y, u, v = planes
    with open(path, "wb") as fh:
        fh.write(header)
        for k in range(len(y)):
            fh.write(mark + b"".join(p[k].astype(p.dtype.newbyteorder("<")).tobytes() for p in (y, u, v) if p is not None))
    return str(path)


def _write(path, planes, chroma, bits, full_range=False, fps=(30000, 1001)):
    from swiftwatcher_amd.io_y4m import Y4MWriter
    y, u, v = planes
    with Y4MWriter(str(path), y.shape[2], y.shape[1], fps, chroma=chroma, bits=bits, full_range=full_range) as w:
        for k in range(len(y)):
            if u is None:
                w.append(y[k])
            else:
                w.append(y[k], u[k], v[k])
    return str(path)


# ------------------------------------------------------------------------------------------------------- the definition
def test_reference_equals_the_420_restatement_at_8_bit_limited():
    rng = np.random.default_rng(1)
    for H, W in [(4, 6), (3, 5), (33, 47)]:
        y, u, v = _planes(rng, 2, H, W)
        assert np.array_equal(ref.bgr(y, u, v), yuv_ref.bgr(y, u, v))
        rect = (1, 1, W - 2, H - 1)
        assert np.array_equal(ref.bgr(y, u, v, rect), yuv_ref.bgr(y, u, v, rect))
    Y, U, V = np.meshgrid(np.arange(0, 256, 3), np.arange(0, 256, 5), np.arange(0, 256, 7), indexing="ij")
    assert all(np.array_equal(a, b) for a, b in zip(ref.pixels(Y, U, V), yuv_ref.pixels(Y, U, V)))
    assert ref.LIMITED == (yuv_ref.CY, yuv_ref.CUB, yuv_ref.CUG, yuv_ref.CVG, yuv_ref.CVR)


@pytest.mark.parametrize("full_range", [False, True], ids=["limited", "full"])
@pytest.mark.parametrize("bits", [9, 10, 12, 14, 16])
def test_samples_shifted_up_convert_to_the_8_bit_bytes(bits, full_range):
    Y, U, V = np.meshgrid(np.arange(256), np.arange(0, 256, 3), np.arange(0, 256, 5), indexing="ij")
    k = bits - 8
    want = ref.pixels(Y, U, V, 8, full_range)
    got = ref.pixels(Y << k, U << k, V << k, bits, full_range)
    assert all(np.array_equal(a, b) for a, b in zip(got, want))


def test_full_range_grey_axis_and_10_bit_limited_end_points():
    Y = np.arange(256)
    for c in ref.pixels(Y, np.full(256, 128), np.full(256, 128), 8, True):
        assert np.array_equal(c, Y)
    assert [int(c[0]) for c in ref.pixels([64], [512], [512], 10, False)] == [0, 0, 0]
    assert [int(c[0]) for c in ref.pixels([940], [512], [512], 10, False)] == [255, 255, 255]
    assert [int(c[0]) for c in ref.pixels([63], [512], [512], 10, False)] == [0, 0, 0]
    # samples are taken as stored: a 10-bit picture may hold a value above 1023
    assert [int(c[0]) for c in ref.pixels([4000], [512], [512], 10, False)] == [255, 255, 255]


# ------------------------------------------------------------------------------------------------------- YuvFrame
@pytest.mark.parametrize("full_range", [False, True], ids=["limited", "full"])
@pytest.mark.parametrize("bits", [8, 10, 16])
@pytest.mark.parametrize("ss", [(0, 0), (1, 0), (1, 1), (2, 0)])
@pytest.mark.parametrize("H,W", [(1, 1), (3, 5), (5, 9), (33, 47)])
def test_frame_converts_like_the_restatement(H, W, ss, bits, full_range):
    from swiftwatcher_amd.io_y4m import YuvFrame
    y, u, v = _planes(np.random.default_rng(H * W + bits), 1, H, W, ss, bits)
    f = YuvFrame(y[0], u[0], v[0], ss, bits, full_range)
    want = ref.bgr(y[0], u[0], v[0], None, ss, bits, full_range)
    assert f.shape == (H, W, 3) and f.dtype == np.uint8 and f.ndim == 3 and len(f) == H
    got = np.asarray(f)
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    for r0, r1, c0, c1 in [(0, H, 0, W), (H // 2, H, W // 3, W), (1, H - 1, 1, W - 1), (0, 1, 0, 1), (H - 1, H, W - 1, W), (2, 2, 0, W)]:
        assert np.array_equal(f[r0:r1, c0:c1], want[r0:r1, c0:c1]), (r0, r1, c0, c1)
    assert np.array_equal(f[1:], want[1:]) and np.array_equal(f[::2, ::-1], want[::2, ::-1]) and np.array_equal(f[0], want[0])
    assert np.array_equal(f[-3:, -4:], want[-3:, -4:])


@pytest.mark.parametrize("bits", [8, 12])
def test_mono_frame_and_null_frames(bits):
    from swiftwatcher_amd.io_y4m import YuvFrame
    y, _, _ = _planes(np.random.default_rng(bits), 1, 7, 10, bits=bits, mono=True)
    for full in (False, True):
        f = YuvFrame(y[0], bits=bits, full_range=full)
        want = ref.bgr(y[0], bits=bits, full_range=full)
        mid = np.full((7, 10), 128 << (bits - 8), y.dtype)
        assert np.array_equal(want, ref.bgr(y[0], mid, mid, None, (0, 0), bits, full))          # mono is U = V = 128 << k
        assert np.array_equal(np.asarray(f), want) and np.array_equal(f[2:6, 3:9], want[2:6, 3:9])
        assert (want[..., 0] == want[..., 1]).all() and (want[..., 1] == want[..., 2]).all()
        for ss, mono in [((1, 1), False), ((0, 0), False), ((2, 0), False), ((0, 0), True)]:
            n = YuvFrame.null(5, 7, ss, bits, full, mono)
            assert n.shape == (5, 7, 3) and not np.asarray(n).any() and (n.u is None) == mono
    with pytest.raises(ValueError):
        YuvFrame(y[0], y[0][:4, :5], y[0][:3, :5], (1, 1), bits)
    with pytest.raises(ValueError):
        YuvFrame(y[0].astype(np.uint8 if bits > 8 else np.uint16), bits=bits)


# ------------------------------------------------------------------------------------------------------- open_y4m: header rules
@pytest.mark.parametrize("tag", sorted(TAGS))
def test_every_accepted_tag(tmp_path, tag):
    from swiftwatcher_amd.io_y4m import Y4MReader, YuvFrame, YuvReader, open_y4m
    mono, ss, bits = TAGS[tag]
    planes = _planes(np.random.default_rng(len(tag)), 3, 5, 7, ss, bits, mono)
    path = _raw_file(tmp_path / "a.y4m", b"YUV4MPEG2 W7 H5 F25:1 Ip A1:1 C%s XYSCSS=FOO\n" % tag.encode(), planes)
    r = open_y4m(path)
    if (mono, ss, bits) == (False, (1, 1), 8):
        assert type(r) is Y4MReader
        r = open_y4m(path, full_range=True)
    assert type(r) is YuvReader and r.total_frames == 3 and r.frame_shape == (5, 7, 3) and r.rate == (25, 1) and r.fps == 25.0
    assert (r.mono, r.subsampling, r.bits) == (mono, ss, bits)
    full = r.full_range
    frames, numbers, _ = r.get_n_frames(3)
    assert numbers == [0, 1, 2]
    for k, f in enumerate(frames):
        assert isinstance(f, YuvFrame) and not hasattr(f, "roi") and (f.sx, f.sy) == ss and f.bits == bits and f.full_range == full
        assert np.array_equal(f.y, planes[0][k]) and not f.y.flags.owndata
        if mono:
            assert f.u is None and f.v is None
        else:
            assert np.array_equal(f.u, planes[1][k]) and np.array_equal(f.v, planes[2][k])
        want = ref.bgr(planes[0][k], None if mono else planes[1][k], None if mono else planes[2][k], None, ss, bits, full)
        assert np.array_equal(np.asarray(f), want)


@pytest.mark.parametrize("header,names", [
    (b"YUV4MPEG2 W6 H4 F25:1 C444alpha\n", "C444alpha"),
    (b"YUV4MPEG2 W6 H4 F25:1 C420p11\n", "C420p11"),
    (b"YUV4MPEG2 W6 H4 F25:1 C410\n", "C410"),
    (b"YUV4MPEG2 W6 H4 F25:1 Cmono14\n", "Cmono14"),
    (b"YUV4MPEG2 W6 H4 F25:1 C422jpeg\n", "C422jpeg"),
    (b"YUV4MPEG2 W6 H4 F25:1 It C422\n", "It"),
    (b"YUV4MPEG2 W6 H4 F25:1 Ib C420p10\n", "Ib"),
    (b"YUV4MPEG2 W6 H4 F25:1 Im Cmono\n", "Im"),
    (b"YUV4MPEG2 W6 H4 F25:1 C444 XCOLORRANGE=WIDE\n", "XCOLORRANGE=WIDE"),
    (b"YUV4MPEG2 W6 H4 F25:1 C444 Q7\n", "Q7"),
    (b"YUV4MPEG2 H4 F25:1 C444\n", "W"),
    (b"YUV4MPEG2 W6 H4 C444\n", "F"),
    (b"YUV4MPEG1 W6 H4 F25:1 C444\n", "YUV4MPEG2"),
])
def test_headers_refused_by_name(tmp_path, header, names):
    from swiftwatcher_amd.io_y4m import open_y4m
    planes = _planes(np.random.default_rng(3), 1, 4, 6, (0, 0), 16)          # (more bytes than any of these formats needs)
    with pytest.raises(ValueError) as err:
        open_y4m(_raw_file(tmp_path / "bad.y4m", header, planes))
    assert names in str(err.value)


@pytest.mark.parametrize("tag", ["422", "444p10", "mono", "420p16", "411", "mono12"])
def test_truncation_by_the_formats_own_frame_size_and_frame_parameters(tmp_path, tag):
    from swiftwatcher_amd.io_y4m import open_y4m
    mono, ss, bits = TAGS[tag]
    planes = _planes(np.random.default_rng(4), 3, 5, 7, ss, bits, mono)
    header = b"YUV4MPEG2 W7 H5 F25:1 C%s\n" % tag.encode()
    good = _raw_file(tmp_path / "good.y4m", header, planes)
    data = open(good, "rb").read()
    ch, cw = ref.chroma_shape(5, 7, *ss)
    step = 6 + (35 + (0 if mono else 2 * ch * cw)) * (2 if bits > 8 else 1)
    assert len(data) == len(header) + 3 * step and open_y4m(good).total_frames == 3
    for cut in (1, 7, step - 1):
        short = tmp_path / ("short%d.y4m" % cut)
        short.write_bytes(data[:-cut])
        with pytest.raises(ValueError) as err:
            open_y4m(str(short))
        assert "truncated" in str(err.value) and str(step) in str(err.value)
    whole = tmp_path / "two.y4m"
    whole.write_bytes(data[:-step])
    assert open_y4m(str(whole)).total_frames == 2
    with pytest.raises(ValueError) as err:
        open_y4m(_raw_file(tmp_path / "p.y4m", header, planes, mark=b"FRAME Ip\n"))
    assert "FRAME" in str(err.value)
    with pytest.raises(ValueError):
        open_y4m(_raw_file(tmp_path / "q.y4m", header, planes, mark=b"FRAMF\n"))


def test_range_tag_and_keyword(tmp_path):
    from swiftwatcher_amd.io_y4m import Y4MReader, YuvReader, open_y4m
    planes = _planes(np.random.default_rng(5), 2, 4, 6)
    files = {rng: _raw_file(tmp_path / ("%s.y4m" % rng), b"YUV4MPEG2 W6 H4 F25:1 Ip C420jpeg XYSCSS=420JPEG%s\n" % tag, planes)
             for rng, tag in [("full", b" XCOLORRANGE=FULL"), ("limited", b" XCOLORRANGE=LIMITED"), ("absent", b"")]}
    want = {full: ref.bgr(*planes, full_range=full) for full in (False, True)}
    assert not np.array_equal(want[False], want[True])
    for name, keyword, full in [("full", None, True), ("limited", None, False), ("absent", None, False),
                                ("full", False, False), ("limited", True, True), ("absent", True, True), ("full", True, True),
                                ("absent", False, False)]:
        r = open_y4m(files[name], full_range=keyword)
        assert type(r) is (YuvReader if full else Y4MReader), (name, keyword)
        frames = r.get_n_frames(2)[0]
        assert all(np.array_equal(np.asarray(f), want[full][k]) for k, f in enumerate(frames)), (name, keyword)
    # the 8-bit 4:2:0 reader itself keeps today's result for a file marked full range
    assert np.array_equal(np.asarray(Y4MReader(files["full"]).get_n_frames(1)[0][0]), want[False][0])
    # another format: the tag and the keyword decide the same way
    p10 = _planes(np.random.default_rng(6), 1, 4, 6, (1, 0), 10)
    path = _raw_file(tmp_path / "p10.y4m", b"YUV4MPEG2 W6 H4 F25:1 C422p10 XCOLORRANGE=FULL\n", p10)
    assert open_y4m(path).full_range and not open_y4m(path, full_range=False).full_range
    assert np.array_equal(np.asarray(open_y4m(path, full_range=False).get_n_frames(1)[0][0]), ref.bgr(p10[0][0], p10[1][0], p10[2][0], None, (1, 0), 10))


def test_open_y4m_hands_8_bit_420_limited_files_to_the_old_reader(tmp_path):
    from swiftwatcher_amd.io_y4m import Y4MReader, Y4MWriter, Yuv420Frame, open_y4m
    y, u, v = _planes(np.random.default_rng(7), 4, 5, 7)
    path = str(tmp_path / "a.y4m")
    with Y4MWriter(path, 7, 5, 30) as w:
        for k in range(4):
            w.append(y[k], u[k], v[k])
    a, b = open_y4m(path, start=1, end=3), Y4MReader(path, start=1, end=3)
    assert type(a) is Y4MReader and (a.start_frame, a.end_frame, a.total_frames, a.fps) == (b.start_frame, b.end_frame, b.total_frames, b.fps)
    fa, na, sa = a.get_n_frames(5)
    fb, nb, sb = b.get_n_frames(5)
    assert na == nb and sa == sb
    for x, z in zip(fa, fb):
        assert isinstance(x, Yuv420Frame) and np.array_equal(x.y, z.y) and np.array_equal(x.u, z.u) and np.array_equal(x.v, z.v)
    with pytest.raises(ValueError):
        open_y4m(__file__)


# ------------------------------------------------------------------------------------------------------- the writer
def test_writer_defaults_write_todays_bytes(tmp_path):
    from swiftwatcher_amd.io_y4m import Y4MWriter
    y, u, v = _planes(np.random.default_rng(8), 2, 5, 7)
    with Y4MWriter(str(tmp_path / "a.y4m"), 7, 5, (30000, 1001)) as w:
        for k in range(2):
            w.append(y[k], u[k], v[k])
    want = b"YUV4MPEG2 W7 H5 F30000:1001 Ip A0:0 C420jpeg\n" + b"".join(b"FRAME\n" + y[k].tobytes() + u[k].tobytes() + v[k].tobytes() for k in range(2))
    assert (tmp_path / "a.y4m").read_bytes() == want
    with Y4MWriter(str(tmp_path / "b.y4m"), 7, 5, (30000, 1001), chroma="420", bits=8, full_range=False) as w:
        for k in range(2):
            w.append(y[k], u[k], v[k])
    assert (tmp_path / "b.y4m").read_bytes() == want


@pytest.mark.parametrize("chroma,bits,full", [("420", 8, True), ("420", 10, False), ("422", 8, False), ("422", 10, True), ("444", 8, False),
                                              ("444", 16, True), ("411", 8, False), ("mono", 8, False), ("mono", 10, True), ("420", 9, False),
                                              ("422", 12, False), ("444", 14, False), ("mono", 16, False), ("mono", 9, False), ("mono", 12, True)])
def test_other_formats_round_trip_through_writer_and_reader(tmp_path, chroma, bits, full):
    from swiftwatcher_amd.io_y4m import Y4MWriter, YuvReader, open_y4m
    mono = chroma == "mono"
    ss = (0, 0) if mono else ref.SUBSAMPLINGS[chroma]
    planes = _planes(np.random.default_rng(bits), 3, 5, 9, ss, bits, mono)
    r = open_y4m(_write(tmp_path / "a.y4m", planes, chroma, bits, full))
    assert type(r) is YuvReader and (r.mono, r.subsampling, r.bits, r.full_range) == (mono, ss, bits, full) and r.rate == (30000, 1001)
    frames = r.get_n_frames(3)[0]
    for k, f in enumerate(frames):
        assert np.array_equal(f.y, planes[0][k]) and f.y.dtype == planes[0].dtype
        assert mono or (np.array_equal(f.u, planes[1][k]) and np.array_equal(f.v, planes[2][k]))
    for bad in (dict(chroma="410"), dict(bits=11), dict(chroma="mono", bits=14), dict(chroma="411", bits=7)):
        with pytest.raises(ValueError):
            Y4MWriter(str(tmp_path / "bad.y4m"), 9, 5, 30, **bad)
    with pytest.raises(ValueError):
        with Y4MWriter(str(tmp_path / "c.y4m"), 9, 5, 30, chroma=chroma, bits=bits) as w:
            w.append(planes[0][0][:, :4]) if mono else w.append(planes[0][0], planes[1][0])


# ------------------------------------------------------------------------------------------------------- bookkeeping
@pytest.mark.parametrize("chroma,bits", [("422", 10), ("mono", 8), ("444", 8)])
def test_past_the_end_last_frame_once_then_null_frames(tmp_path, chroma, bits):
    from swiftwatcher_amd.io_frames import ArrayReader
    from swiftwatcher_amd.io_y4m import YuvFrame, open_y4m
    mono = chroma == "mono"
    ss = (0, 0) if mono else ref.SUBSAMPLINGS[chroma]
    y, u, v = _planes(np.random.default_rng(9), 4, 3, 5, ss, bits, mono)
    path = _write(tmp_path / "a.y4m", (y, u, v), chroma, bits)
    r = open_y4m(path)
    frames, numbers, stamps = r.get_n_frames(7)
    assert numbers == [0, 1, 2, 3, 4, -1, -1]
    assert r.read_errors == 1 and r.frames_read == 4
    assert np.array_equal(frames[4].y, y[3])
    assert stamps[5] == stamps[6] == "00:00:00.000"
    for f in frames[5:]:
        assert isinstance(f, YuvFrame) and f.shape == (3, 5, 3) and f.format == frames[0].format
        assert not np.asarray(f).any()          # the reference's null frame: all-zero BGR
    a = ArrayReader(list(ref.bgr(y, u, v, None, ss, bits)), fps=r.fps)
    frames_a, numbers_a, stamps_a = a.get_n_frames(7)
    assert numbers_a == numbers and stamps_a == stamps and (a.read_errors, a.frames_read) == (r.read_errors, r.frames_read)
    for fy, fa in zip(frames, frames_a):
        assert np.array_equal(np.asarray(fy), fa)
    r2 = open_y4m(path, start=1, end=2)
    assert r2.total_frames == 1 and r2.get_n_frames(3)[1] == [1, 2, -1]
    first = r.read_frame(0, increment=False)
    assert np.array_equal(first.y, y[0])


def test_forward_transform_makes_clips_that_come_back():
    """bgr_to_planes only makes material; still, a flat grey picture must come back exactly in every format."""
    grey = np.full((1, 6, 8, 3), 77, np.uint8)
    for ss in ref.SUBSAMPLINGS.values():
        for bits in (8, 10, 16):
            for full in (False, True):
                y, u, v = ref.bgr_to_planes(grey, ss, bits, full)
                assert u.shape == (1,) + ref.chroma_shape(6, 8, *ss)
                assert np.abs(ref.bgr(y, u, v, None, ss, bits, full).astype(int) - 77).max() <= 1
    y, u, v = ref.bgr_to_planes(grey, bits=10, mono=True)
    assert u is None and v is None and y.dtype == np.uint16
