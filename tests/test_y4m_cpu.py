"""YUV4MPEG2 reader / writer and the 4:2:0 frame type (swiftwatcher_amd/io_y4m.py), without a GPU: header rules, frame
bookkeeping, and the host-side BGR conversion of Yuv420Frame against the scalar restatement (tests/yuv_ref.py)."""
import numpy as np
import pytest

import yuv_ref


def _planes(rng, count, H, W):
    ch, cw = (H + 1) // 2, (W + 1) // 2
    return (rng.integers(0, 256, (count, H, W), dtype=np.uint8), rng.integers(0, 256, (count, ch, cw), dtype=np.uint8),
            rng.integers(0, 256, (count, ch, cw), dtype=np.uint8))


def _write(path, y, u, v, fps=(30000, 1001)):
    from swiftwatcher_amd.io_y4m import Y4MWriter
    with Y4MWriter(str(path), y.shape[2], y.shape[1], fps) as w:
        for k in range(len(y)):
            w.append(y[k], u[k], v[k])
    return str(path)


def _raw_file(path, header, y, u, v, mark=b"FRAME\n"):
    with open(path, "wb") as fh:
        fh.write(header)
        for k in range(len(y)):
            fh.write(mark + y[k].tobytes() + u[k].tobytes() + v[k].tobytes())
    return str(path)


def test_reference_formula_reproduces_the_hand_vectors():
    for (Y, U, V), expect in yuv_ref.HAND_VECTORS:
        got = tuple(int(c) for c in yuv_ref.pixels(Y, U, V))
        assert got == expect, ((Y, U, V), got, expect)
    one = yuv_ref.bgr(np.array([[81]], np.uint8), np.array([[90]], np.uint8), np.array([[240]], np.uint8))
    assert one.shape == (1, 1, 3) and one.dtype == np.uint8 and one[0, 0].tolist() == [0, 0, 254]
    # every intermediate fits int32 (the product computes there)
    assert 239 * yuv_ref.CY + (1 << 19) + 127 * yuv_ref.CUB < 2 ** 31
    assert (1 << 19) + 127 * (yuv_ref.CVG + yuv_ref.CUG) > -2 ** 31


@pytest.mark.parametrize("W,H,count", [(6, 4, 3), (5, 3, 4), (160, 110, 5)])
def test_writer_reader_round_trip(tmp_path, W, H, count):
    from swiftwatcher_amd.io_y4m import Y4MReader, Yuv420Frame
    y, u, v = _planes(np.random.default_rng(W * H), count, H, W)
    r = Y4MReader(_write(tmp_path / "a.y4m", y, u, v))
    assert r.total_frames == count and len(r.frames) == count
    assert r.fps == 30000 / 1001 and r.rate == (30000, 1001)
    assert r.frame_shape == (H, W, 3)
    frames, numbers, stamps = r.get_n_frames(count)
    assert numbers == list(range(count))
    for k, f in enumerate(frames):
        assert isinstance(f, Yuv420Frame) and not hasattr(f, "roi")
        assert f.shape == (H, W, 3) and f.dtype == np.uint8 and f.ndim == 3
        assert np.array_equal(f.y, y[k]) and np.array_equal(f.u, u[k]) and np.array_equal(f.v, v[k])
        assert not f.y.flags.owndata          # a view of the mapping
    # timestamps are the ArrayReader's
    from swiftwatcher_amd.io_frames import ArrayReader
    plain = ArrayReader([np.zeros((H, W, 3), np.uint8)] * count, fps=30000 / 1001)
    assert stamps == plain.get_n_frames(count)[2]
    first = r.read_frame(0, increment=False)
    assert np.array_equal(first.y, y[0])


def test_fps_forms_of_the_writer(tmp_path):
    from swiftwatcher_amd.io_y4m import Y4MReader
    y, u, v = _planes(np.random.default_rng(1), 1, 4, 6)
    assert Y4MReader(_write(tmp_path / "a.y4m", y, u, v, fps=30)).rate == (30, 1)
    assert Y4MReader(_write(tmp_path / "b.y4m", y, u, v, fps=30000 / 1001)).rate == (30000, 1001)
    from swiftwatcher_amd.io_y4m import Y4MWriter
    with pytest.raises(ValueError):
        with Y4MWriter(str(tmp_path / "c.y4m"), 6, 4, 30) as w:
            w.append(y[0], u[0][:, :2], v[0])


@pytest.mark.parametrize("header", [
    b"YUV4MPEG2 W6 H4 F30000:1001 Ip A1:1 C420jpeg XYSCSS=420JPEG XCOLORRANGE=LIMITED\n",        # what ffmpeg writes
    b"YUV4MPEG2 W6 H4 F30000:1001\n",                                                            # C and I absent
    b"YUV4MPEG2 H4 W6 F30000:1001 I? C420\n",
    b"YUV4MPEG2 W6 H4 F30000:1001 Ip A128:117 C420mpeg2\n",
    b"YUV4MPEG2 W6 H4 F30000:1001 Ip C420paldv XFOO\n",
])
def test_headers_accepted(tmp_path, header):
    from swiftwatcher_amd.io_y4m import Y4MReader
    y, u, v = _planes(np.random.default_rng(2), 2, 4, 6)
    r = Y4MReader(_raw_file(tmp_path / "h.y4m", header, y, u, v))
    assert r.total_frames == 2 and r.rate == (30000, 1001)
    f = r.get_n_frames(2)[0][1]
    assert np.array_equal(f.y, y[1]) and np.array_equal(f.u, u[1]) and np.array_equal(f.v, v[1])


@pytest.mark.parametrize("header,names", [
    (b"YUV4MPEG2 W6 H4 F25:1 C422\n", "C422"),
    (b"YUV4MPEG2 W6 H4 F25:1 C444\n", "C444"),
    (b"YUV4MPEG2 W6 H4 F25:1 Cmono\n", "Cmono"),
    (b"YUV4MPEG2 W6 H4 F25:1 C420p10\n", "C420p10"),
    (b"YUV4MPEG2 W6 H4 F25:1 It\n", "It"),
    (b"YUV4MPEG2 W6 H4 F25:1 Ib C420jpeg\n", "Ib"),
    (b"YUV4MPEG2 W6 H4 F25:1 Im\n", "Im"),
    (b"YUV4MPEG2 W6 H4 F25:1 Q7\n", "Q7"),
    (b"YUV4MPEG2 H4 F25:1\n", "W"),
    (b"YUV4MPEG2 W6 F25:1\n", "H"),
    (b"YUV4MPEG2 W6 H4\n", "F"),
    (b"YUV4MPEG2 W6 H4 F25\n", "F25"),
    (b"YUV4MPEG1 W6 H4 F25:1\n", "YUV4MPEG2"),
])
def test_headers_refused_by_name(tmp_path, header, names):
    from swiftwatcher_amd.io_y4m import Y4MReader
    y, u, v = _planes(np.random.default_rng(3), 1, 4, 6)
    with pytest.raises(ValueError) as err:
        Y4MReader(_raw_file(tmp_path / "bad.y4m", header, y, u, v))
    assert names in str(err.value)


def test_truncated_file_and_parameterised_frame_line(tmp_path):
    from swiftwatcher_amd.io_y4m import Y4MReader
    y, u, v = _planes(np.random.default_rng(4), 3, 4, 6)
    good = _write(tmp_path / "good.y4m", y, u, v)
    data = open(good, "rb").read()
    for cut in (1, 7, 36):
        short = tmp_path / ("short%d.y4m" % cut)
        short.write_bytes(data[:-cut])
        with pytest.raises(ValueError) as err:
            Y4MReader(str(short))
        assert "truncated" in str(err.value)
    with pytest.raises(ValueError) as err:
        Y4MReader(_raw_file(tmp_path / "p.y4m", b"YUV4MPEG2 W6 H4 F25:1\n", y, u, v, mark=b"FRAME Ip\n"))
    assert "FRAME" in str(err.value)
    with pytest.raises(ValueError):
        Y4MReader(_raw_file(tmp_path / "q.y4m", b"YUV4MPEG2 W6 H4 F25:1\n", y, u, v, mark=b"FRAMF\n"))


def test_past_the_end_last_frame_once_then_null_frames(tmp_path):
    from swiftwatcher_amd.io_y4m import Y4MReader, Yuv420Frame
    y, u, v = _planes(np.random.default_rng(5), 4, 3, 5)
    r = Y4MReader(_write(tmp_path / "a.y4m", y, u, v))
    frames, numbers, stamps = r.get_n_frames(7)
    assert numbers == [0, 1, 2, 3, 4, -1, -1]
    assert r.read_errors == 1 and r.frames_read == 4
    assert np.array_equal(frames[4].y, y[3]) and np.array_equal(frames[4].u, u[3]) and np.array_equal(frames[4].v, v[3])
    assert stamps[5] == stamps[6] == "00:00:00.000"
    for f in frames[5:]:
        assert isinstance(f, Yuv420Frame) and f.shape == (3, 5, 3)
        assert not f.y.any() and (f.u == 128).all() and (f.v == 128).all()
        assert not np.asarray(f).any()          # the reference's null frame: all-zero BGR
    # the ArrayReader over the restated BGR frames keeps the same books
    from swiftwatcher_amd.io_frames import ArrayReader
    a = ArrayReader(list(yuv_ref.bgr(y, u, v)), fps=r.fps)
    frames_a, numbers_a, stamps_a = a.get_n_frames(7)
    assert numbers_a == numbers and stamps_a == stamps and (a.read_errors, a.frames_read) == (r.read_errors, r.frames_read)
    for fy, fa in zip(frames, frames_a):
        assert np.array_equal(np.asarray(fy), fa)
    # start / end
    r2 = Y4MReader(_write(tmp_path / "b.y4m", y, u, v), start=1, end=2)
    assert r2.total_frames == 1 and r2.get_n_frames(3)[1] == [1, 2, -1]


@pytest.mark.parametrize("H,W", [(4, 6), (3, 5), (7, 10), (110, 160), (33, 47)])
def test_frame_converts_like_the_restatement(H, W):
    from swiftwatcher_amd.io_y4m import Yuv420Frame
    y, u, v = _planes(np.random.default_rng(H * 1000 + W), 1, H, W)
    f = Yuv420Frame(y[0], u[0], v[0])
    want = yuv_ref.bgr(y[0], u[0], v[0])
    whole = np.asarray(f)
    assert whole.dtype == np.uint8 and whole.shape == (H, W, 3) and np.array_equal(whole, want)
    assert np.array_equal(np.array(f), want) and np.asarray(f, dtype=np.float32).dtype == np.float32
    slices = [(slice(0, H), slice(0, W)), (slice(1, H), slice(1, W)), (slice(0, H - 1), slice(0, W - 1)), (slice(1, 2), slice(2, 3)),
              (slice(H - 1, H), slice(W - 1, W)), (slice(H - 2, None), slice(W - 3, None)), (slice(2, 2), slice(0, W)),
              (slice(None), slice(1, 4)), (slice(-3, -1), slice(-4, None)), (slice(1, H + 9), slice(0, W + 9))]
    for rs, cs in slices:
        got = f[rs, cs]
        assert got.dtype == np.uint8 and np.array_equal(got, want[rs, cs]), (rs, cs)
    assert np.array_equal(f[1:3], want[1:3])
    assert np.array_equal(f[1], want[1]) and np.array_equal(f[::2, ::-1], want[::2, ::-1]) and np.array_equal(f[..., 1], want[..., 1])
    assert len(f) == H


def test_every_chroma_and_extreme_luma_on_the_host():
    from swiftwatcher_amd.io_y4m import Yuv420Frame
    uu, vv = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    rng = np.random.default_rng(9)
    y = rng.integers(0, 256, (512, 512), dtype=np.uint8)
    y[::7, ::5] = 255
    y[1::7, 1::5] = 0
    y[2::7, 2::5] = 16
    f = Yuv420Frame(y, uu, vv)
    assert np.array_equal(np.asarray(f), yuv_ref.bgr(y, uu, vv))


def test_regions_and_segment_images_from_a_yuv_frame():
    """generate_regions on the first frame, crop_frame and Segment.segment_image see the BGR frame the 4:2:0 frame stands for."""
    from swiftwatcher_amd import image_filtering as img, synthetic
    from swiftwatcher_amd.data_structures import Segment, _Cut
    from swiftwatcher_amd.io_y4m import Yuv420Frame
    crop = [(60, 50), (60 + 212, 50 + 106)]
    clip = synthetic.full_frames(3, 1, crop, frame_hw=(220, 341), birds=3)
    y, u, v = yuv_ref.bgr_to_yuv420(clip)
    f = Yuv420Frame(y[0], u[0], v[0])
    restated = yuv_ref.bgr(y[0], u[0], v[0])
    corners = [(90, 150), (240, 152)]
    got = img.generate_regions(f, corners)
    want = img.generate_regions(restated, corners)
    assert got[0] == want[0] and np.array_equal(got[1], want[1])
    assert np.array_equal(img.crop_frame(f, crop), img.crop_frame(restated, crop))
    seg = Segment.__new__(Segment)
    seg._image = _Cut((f, (3, 5, 9, 12), (24, 24), crop))
    ref = Segment.__new__(Segment)
    ref._image = _Cut((restated, (3, 5, 9, 12), (24, 24), crop))
    assert seg.segment_image.shape == (24, 24, 3) and np.array_equal(seg.segment_image, ref.segment_image)
