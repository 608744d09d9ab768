"""The deinterlacer without a GPU: the two restatements of its definition (tests/deinterlace_ref.py) against each other and against the
consequences include/swk.h states; the designed planes; the kernel's own sample code built for the host (tests/deinterlace_host.py);
YUV4MPEG2 headers of interlaced files; DeinterlacingReader's bookkeeping with the restatement as its backend; and what the adaptive
deinterlacer buys the segment stage on an interlaced scene."""
import io
import itertools
import os

import numpy as np
import pytest

import deinterlace_cases as cases
import deinterlace_ref as ref


# ------------------------------------------------------------------------------------------------ the restatements
def _random_stacks():
    for d, (H, W), k in itertools.product((8, 10, 16), ((1, 5), (2, 9), (5, 1), (5, 2), (4, 7), (7, 12)), range(2)):
        r = cases.rng("stack", d, H, W, k)
        P = r.integers(0, 1 << d, size=(3, H, W), dtype=np.int64)
        if k:
            P = (P >> (d - 2)) << (d - 2)
        yield d, P


def test_the_two_restatements_agree():
    for d, P in _random_stacks():
        for tff, temporal, parity0 in itertools.product((0, 1), (0, 1), (0, 1)):
            a = ref.pictures(P, tff, 2, temporal, parity0=parity0, fn=ref.picture_scalar)
            b = ref.pictures(P, tff, 2, temporal, parity0=parity0)
            assert np.array_equal(a, b), (d, P.shape, tff, temporal, parity0)


@pytest.mark.parametrize("d", [8, 10, 16])
def test_range_and_stillness(d):
    """the result lies in 0 .. 2^d - 1; on all 0 and all 2^d - 1 it is that; where the three frames agree the picture is the stored one"""
    top = (1 << d) - 1
    for dd, P in _random_stacks():
        if dd != d:
            continue
        for tff, temporal in itertools.product((0, 1), (0, 1)):
            out = ref.pictures(P, tff, 2, temporal)
            assert out.min() >= 0 and out.max() <= top
        still = np.repeat(P[:1], 3, axis=0)
        assert np.array_equal(ref.pictures(still, 1), np.repeat(still, 2, axis=0))
    for v in (0, top):
        P = np.full((3, 5, 9), v, np.int64)
        for temporal in (0, 1):
            assert (ref.pictures(P, 1, 2, temporal) == v).all()
    # the extremes against each other: every sum at its largest, still inside the range (and inside int32: 3 * 65535)
    r = cases.rng("extremes", d)
    P = r.integers(0, 2, size=(3, 6, 11)).astype(np.int64) * top
    out = ref.pictures(P, 1)
    assert out.min() >= 0 and out.max() <= top and np.array_equal(out, ref.pictures(P, 1, fn=ref.picture_scalar))


def test_footprint():
    """a sample depends on frames t - 1, t, t + 1 at rows y - 1 .. y + 1 and columns x - 3 .. x + 3 only"""
    r = cases.rng("footprint")
    P = r.integers(0, 256, size=(5, 9, 15), dtype=np.int64)
    t, y, x = 2, 4, 7
    for tff, second in itertools.product((0, 1), (0, 1)):
        keep = ref.kept_parity(tff, second)
        base = ref.picture(P, t, keep, second)[y, x]
        inside = np.zeros(P.shape, bool)
        inside[t - 1:t + 2, y - 1:y + 2, x - 3:x + 4] = True
        Q = np.where(inside, P, 255 - P)          # every sample outside the footprint changed
        assert ref.picture(Q, t, keep, second)[y, x] == base
    # ... and on its four far corners (direction -2 pairs column x - 3 above with x + 1 below, ..., x - 1 above with x + 3 below):
    # for each there is a plane on which changing that sample alone changes the result
    for row, col in ((0, -3), (0, 3), (2, -3), (2, 3)):
        found = False
        for k in range(2000):
            Q = cases.rng("corner", k).integers(0, 4, size=(1, 3, 9), dtype=np.int64) * 60
            base = ref.sample(Q, 0, 1, 4, 0, 0, temporal=False)
            Q[0, row, 4 + col] = 180 - Q[0, row, 4 + col]
            if ref.sample(Q, 0, 1, 4, 0, 0, temporal=False) != base:
                found = True
                break
        assert found, (row, col)


# ------------------------------------------------------------------------------------------------ designed planes
@pytest.mark.parametrize("j", [-2, -1, 0, 1, 2])
def test_designed_direction_wins(j):
    P, x, want = cases.direction_plane(j)
    pred, chosen = ref.directions(P[0, 0], P[0, 2])
    assert chosen[x] == want
    up, dn = P[0, 0], P[0, 2]
    assert pred[x] == (up[x + j] + dn[x - j]) >> 1 == ref.sample(P, 0, 1, x, 0, 0, temporal=False)


def test_equal_score_is_not_taken():
    P, x = cases.tie_plane()
    up, dn = P[0, 0], P[0, 2]
    _, chosen = ref.directions(up, dn)
    assert chosen[x] == 0 and ref.sample(P, 0, 1, x, 0, 0, temporal=False) == (up[x] + dn[x]) >> 1


def test_minus_two_is_not_reached_past_a_losing_minus_one():
    P, x = cases.unreached_plane()
    up, dn = P[0, 0], P[0, 2]
    _, chosen = ref.directions(up, dn)
    assert chosen[x] == 0 and ref.sample(P, 0, 1, x, 0, 0, temporal=False) == (up[x] + dn[x]) >> 1


@pytest.mark.parametrize("side", ["low", "high"])
def test_clamp_sides(side):
    P, want = cases.clamp_planes(side)
    out = ref.picture(P, 1, 0, 0)          # tff, the middle frame's first field: rows 0 and 2 kept
    assert (out[1] == want).all() and (ref.picture(P, 1, 0, 0, temporal=False)[1] == 100).all()
    assert (want > 100) if side == "low" else (want < 100)


def test_field_order():
    """bff over frames whose rows are swapped pairwise is tff over the original fields: the same fields come out in the same order,
    each at the other parity"""
    r = cases.rng("order")
    P = r.integers(0, 256, size=(3, 8, 11), dtype=np.int64)
    swapped = P.reshape(3, 4, 2, 11)[:, :, ::-1].reshape(3, 8, 11)          # rows 0 <-> 1, 2 <-> 3, ...
    a = ref.pictures(P, 1, temporal=False)
    b = ref.pictures(swapped, 0, temporal=False)
    # tff keeps P's even rows first; bff over `swapped` keeps its odd rows first, which are P's even rows
    assert np.array_equal(a[:, 0::2][::2], b[:, 1::2][::2]) and np.array_equal(a[:, 1::2][1::2], b[:, 0::2][1::2])
    # parity0 = 1 turns the rule round: tff with parity0 = 1 keeps the rows bff keeps with parity0 = 0
    for second in (0, 1):
        assert np.array_equal(ref.picture(P, 1, ref.kept_parity(1, second), second, parity0=1),
                              ref.picture(P, 1, ref.kept_parity(0, second), second, parity0=0))


# ------------------------------------------------------------------------------------------------ the kernel's code on the host
@pytest.fixture(scope="module")
def host(tmp_path_factory):
    import deinterlace_host
    return deinterlace_host.build(tmp_path_factory.mktemp("deint_host"))


def test_kernel_code_on_the_host(host):
    """deint_quad, the function k_deint_plane calls, walked over planes on the host: every width and height the GPU test uses, 1- and
    2-byte samples, MSB-aligned words, interleaved samples, whole planes and rectangles, described whole or staged as a host source is"""
    import deinterlace_host as dh
    cyc, ncombos = cases.param_cycle()
    n = 0
    for W, H in itertools.product((1, 2, 3, 6, 7, 8, 9, 61, 62, 63, 64, 65, 66, 67), (1, 2, 3, 4, 5, 16, 17)):
        count, params = next(cyc)
        r = cases.rng("host", W, H)
        bits = (8, 10, 16)[n % 3]
        msb = (16 - bits) if bits > 8 and n % 2 else 0
        step = 2 if n % 5 == 0 else 1
        vals = r.integers(0, 1 << bits, size=(count, H, W) + ((2,) if step == 2 else ()), dtype=np.int64)
        if n % 4 == 0:
            vals = (vals >> (bits - 2)) << (bits - 2)
        stored = (vals << msb).astype(np.uint16 if bits > 8 else np.uint8)
        px0, py0 = int(r.integers(0, W)), int(r.integers(0, H))
        rect = (0, 0, W, H) if n % 3 == 0 else (px0, py0, int(r.integers(1, W - px0 + 1)), int(r.integers(1, H - py0 + 1)))
        which, parity0 = n % 2 if step == 2 else 0, (n // 2) % 2
        got = dh.plane(host, stored, rect, step=step, which=which, msb=msb, staged=n % 2 == 1, parity0=parity0, **params)
        want = ref.pictures(vals[..., which] if step == 2 else vals, parity0=parity0, **params)
        assert cases.same(got, want[:, rect[1]:rect[1] + rect[3], rect[0]:rect[0] + rect[2]]), (W, H, bits, msb, step, rect, params)
        n += 1
    assert n >= ncombos
    for name, P in cases.DESIGNED:
        for tff, temporal in itertools.product((0, 1), (0, 1)):
            got = dh.plane(host, P.astype(np.uint8), (0, 0, P.shape[2], P.shape[1]), tff=tff, temporal=temporal)
            assert cases.same(got, ref.pictures(P, tff, 2, temporal)), (name, tff, temporal)


# ------------------------------------------------------------------------------------------------ YUV4MPEG2 headers
def test_header_parsing_and_refusals():
    from swiftwatcher_amd.io_y4m import _parse_header
    base = b"YUV4MPEG2 W16 H12 F25:1 %s A0:0 C420jpeg"
    assert _parse_header(base % b"Ip") == (16, 12, 25, 1)                                          # as it always was
    for tag, order in ((b"Ip", "p"), (b"I?", "p"), (b"It", "t"), (b"Ib", "b")):
        assert _parse_header(base % tag, interlaced=True) == (16, 12, 25, 1, order)
        assert _parse_header(base % tag, general=True, interlaced="bob")[-1] == order
    assert _parse_header(b"YUV4MPEG2 W16 H12 F25:1", interlaced=True)[-1] == "p"
    for tag in (b"It", b"Ib"):
        with pytest.raises(ValueError, match="interlaced YUV4MPEG2 files are not supported") as exc:
            _parse_header(base % tag)
        assert "--deinterlace" in str(exc.value) and tag.decode() in str(exc.value)
    for kw in (dict(), dict(interlaced=True)):
        with pytest.raises(ValueError, match="interlaced YUV4MPEG2 files are not supported .tag Im.: mixed field order"):
            _parse_header(base % b"Im", **kw)
        with pytest.raises(ValueError, match="interlaced YUV4MPEG2 files are not supported .tag Ix."):          # (worded as it always was)
            _parse_header(base % b"Ix", **kw)


def _stored(N, H=20, W=28, seed=0):
    r = cases.rng("stored", N, H, W, seed)
    return (r.integers(0, 256, size=(N, H, W), dtype=np.uint8), r.integers(0, 256, size=(N, (H + 1) // 2, (W + 1) // 2), dtype=np.uint8),
            r.integers(0, 256, size=(N, (H + 1) // 2, (W + 1) // 2), dtype=np.uint8))


def _write(path, planes, order="t", fps=25, **kw):
    from swiftwatcher_amd.io_y4m import Y4MWriter
    y, u, v = planes
    with Y4MWriter(str(path), y.shape[2], y.shape[1], fps, interlaced=order, **kw) as w:
        for k in range(len(y)):
            w.append(y[k], u[k], v[k])
    return str(path)


def test_writer_tags_and_default_refusal(tmp_path):
    from swiftwatcher_amd.io_y4m import Y4MWriter, open_y4m, Y4MStreamReader
    planes = _stored(2)
    heads = {}
    for order in ("p", "t", "b"):
        heads[order] = open(_write(tmp_path / ("%s.y4m" % order), planes, order), "rb").readline()
    assert heads["p"] == b"YUV4MPEG2 W28 H20 F25:1 Ip A0:0 C420jpeg\n"          # what it writes today
    assert heads["t"] == heads["p"].replace(b" Ip ", b" It ") and heads["b"] == heads["p"].replace(b" Ip ", b" Ib ")
    with pytest.raises(ValueError):
        Y4MWriter(str(tmp_path / "x.y4m"), 28, 20, 25, interlaced="m")
    for order in ("t", "b"):
        path = str(tmp_path / ("%s.y4m" % order))
        with pytest.raises(ValueError, match="interlaced YUV4MPEG2 files are not supported"):
            open_y4m(path)
        with pytest.raises(ValueError, match="interlaced YUV4MPEG2 files are not supported"):
            Y4MStreamReader(io.BytesIO(open(path, "rb").read()))
        assert open_y4m(path, interlaced=True).field_order == order
        s = open_y4m(io.BytesIO(open(path, "rb").read()), interlaced=True)
        assert s.field_order == order
        s.close()
    assert open_y4m(str(tmp_path / "p.y4m"), interlaced=True).field_order == "p"
    mixed = open(str(tmp_path / "t.y4m"), "rb").read().replace(b" It ", b" Im ", 1)
    (tmp_path / "m.y4m").write_bytes(mixed)
    with pytest.raises(ValueError, match="mixed field order"):
        open_y4m(str(tmp_path / "m.y4m"), interlaced=True)


def test_a_pipe_keeps_the_second_frame_until_it_is_handed_out(tmp_path):
    """read_frame(1, increment=False) of an interlaced pipe reads two frames early; windows of one frame still get both, and the
    third as usual; a progressive pipe offers no second frame"""
    from swiftwatcher_amd.io_y4m import open_y4m
    planes = _stored(4, seed=5)
    for order in ("t", "p"):
        data = open(_write(tmp_path / ("%s.y4m" % order), planes, order), "rb").read()
        s = open_y4m(io.BytesIO(data), interlaced=True)
        if order == "p":
            with pytest.raises(ValueError, match="only offers"):
                s.read_frame(1, increment=False)
        else:
            assert np.array_equal(s.read_frame(1, increment=False).y, planes[0][1]) and np.array_equal(s.read_frame(0, increment=False).y, planes[0][0])
        for k in range(4):
            (f,), (n,), _ = s.get_n_frames(1)
            assert n == k and np.array_equal(f.y, planes[0][k]) and np.array_equal(f.v, planes[2][k]), (order, k)
        assert s._first is None and s._second is None
        s.close()


# ------------------------------------------------------------------------------------------------ the reader
class RefBackend:
    """Context.yuv_deinterlace over io_y4m frames, by the restatement: the frames' rectangle is gathered as the library wrapper
    gathers it, so what the reader crops is checked against the whole-frame reference below."""
    calls = 0

    def yuv_deinterlace(self, frames, rect, tff, rate=2, temporal=True, has_prev=False, has_next=False):
        from swiftwatcher_amd import _lib
        (Y, U, V), (sub, bits, full), inner, parity0 = _lib._gather_fields(frames, rect)
        self.calls += 1
        i64 = lambda a: None if a is None else a.astype(np.int64)          # noqa: E731
        return ref.call_bgr(i64(Y), i64(U), i64(V), subsampling=sub, bits=bits, full_range=full, rect=inner, tff=tff, rate=rate,
                            temporal=temporal, has_prev=has_prev, has_next=has_next, parity0=parity0)


def _whole_reference(planes, order="t", rate=2, temporal=True):
    y, u, v = (p.astype(np.int64) for p in planes)
    return ref.call_bgr(y, u, v, subsampling=(1, 1), tff=order == "t", rate=rate, temporal=temporal)


def _cut(frame, rect):
    ya, yb, xa, xb = rect
    return np.asarray(frame[ya:yb, xa:xb])


CROP = [(6, 4), (20, 14)]          # (x0, y0), (x1, y1); with min_seg_size (4, 4) the margin rectangle is rows 2..16, columns 4..22
MSS = (4, 4)
RECT = (2, 16, 4, 22)


def _same_as_array_reader(reader, pics, fps, start, end, window, rect, calls=6, pipe=False):
    """`reader` against io_frames.ArrayReader over the pictures (a list indexed by picture number), call by call.  pipe: nobody knows
    the length of the video while it goes on -- total_frames is then the number known to exist, more than what was handed out, and
    exact once the source has ended (io_y4m.Y4MStreamReader)."""
    from swiftwatcher_amd.io_frames import ArrayReader
    want = ArrayReader(pics, fps=fps, start=start, end=end)
    assert (reader.fps, reader.start_frame) == (want.fps, want.start_frame)
    if not pipe:
        assert (reader.end_frame, reader.total_frames) == (want.end_frame, want.total_frames)
    for _ in range(calls):
        gf, gn, gs = reader.get_n_frames(window)
        wf, wn, ws = want.get_n_frames(window)
        assert gn == wn and gs == ws
        for a, b, k in zip(gf, wf, wn):
            assert np.array_equal(_cut(a, rect), _cut(b, rect)), k
        assert (reader.next_frame_number, reader.frames_read, reader.read_errors) == (want.next_frame_number, want.frames_read, want.read_errors)
        if pipe and want.next_frame_number < want.end_frame:
            assert reader.next_frame_number - reader.start_frame < reader.total_frames <= want.total_frames
        else:
            assert reader.total_frames == want.total_frames


@pytest.mark.parametrize("N", [1, 2, 10, 11])
@pytest.mark.parametrize("window", [1, 7, 21])
def test_bob_bookkeeping_is_array_readers(tmp_path, N, window):
    from swiftwatcher_amd.deinterlace import DeinterlacingReader
    from swiftwatcher_amd.io_y4m import open_y4m
    planes = _stored(N, seed=N)
    path = _write(tmp_path / "v.y4m", planes, "t")
    pics = list(_whole_reference(planes))
    calls = (2 * N + 2) // window + 3
    for source in (path, io.BytesIO(open(path, "rb").read())):
        wrapped = open_y4m(source, interlaced=True)
        backend = RefBackend()
        reader = DeinterlacingReader(wrapped, CROP, "bob", min_seg_size=MSS, backend=backend)
        _same_as_array_reader(reader, pics, 50.0, 0, 0, window, RECT, calls, pipe=source is not path)
        assert reader.fields == {"mode": "bob", "field_order": "t", "stored_frames": N, "frames": 2 * N}
        assert backend.calls <= -(-2 * N // window) + 1          # one library call per window that needed pictures
        if hasattr(wrapped, "close"):
            wrapped.close()


@pytest.mark.parametrize("start,end", [(2, 0), (0, 7), (3, 8), (2, 10)])
def test_bob_bookkeeping_with_start_and_end(tmp_path, start, end):
    """start= / end= of the wrapped reader count stored frames; the video is what it hands out (frame `end` included where the file
    has it, as the reference's inclusive range test has it): its first and last frame have no neighbour"""
    from swiftwatcher_amd.deinterlace import DeinterlacingReader
    from swiftwatcher_amd.io_y4m import open_y4m
    N = 10
    planes = _stored(N, seed=7)
    path = _write(tmp_path / "v.y4m", planes, "b")
    last = min(end, N - 1) if end else N - 1
    seen = tuple(p[start:last + 1] for p in planes)
    never = np.zeros((20, 28, 3), np.uint8)          # (pictures outside the range are never read)
    pics = [never] * (2 * start) + list(_whole_reference(seen, "b")) + [never] * (2 * (N - 1 - last))
    for source in (path, io.BytesIO(open(path, "rb").read())):
        wrapped = open_y4m(source, start, end, interlaced=True)
        reader = DeinterlacingReader(wrapped, CROP, "bob", min_seg_size=MSS, backend=RefBackend())
        _same_as_array_reader(reader, pics, 50.0, 2 * start, 2 * end, 7, RECT, calls=5, pipe=source is not path and not end)
        if hasattr(wrapped, "close"):
            wrapped.close()


def test_weave_and_frame_modes(tmp_path):
    from swiftwatcher_amd.deinterlace import DeinterlacingReader
    from swiftwatcher_amd.io_y4m import open_y4m, yuv420_rect_to_bgr
    N = 5
    planes = _stored(N, seed=3)
    path = _write(tmp_path / "v.y4m", planes, "t")
    backend = RefBackend()
    weave = DeinterlacingReader(open_y4m(path, interlaced=True), CROP, "weave", min_seg_size=MSS, backend=backend)
    stored = [yuv420_rect_to_bgr(planes[0][k], planes[1][k], planes[2][k], 0, 20, 0, 28) for k in range(N)]
    _same_as_array_reader(weave, stored, 25.0, 0, 0, 4, (0, 20, 0, 28), calls=3)
    assert backend.calls == 0 and weave.fields["mode"] == "weave"
    frame = DeinterlacingReader(open_y4m(path, interlaced=True), CROP, "frame", min_seg_size=MSS, backend=backend)
    _same_as_array_reader(frame, list(_whole_reference(planes)[0::2]), 25.0, 0, 0, 4, RECT, calls=3)
    assert list(_whole_reference(planes, rate=1).reshape(N, -1)[:, 0]) == list(_whole_reference(planes)[0::2].reshape(N, -1)[:, 0])
    spatial = DeinterlacingReader(open_y4m(path, interlaced=True), CROP, "bob", temporal=False, min_seg_size=MSS, backend=backend)
    _same_as_array_reader(spatial, list(_whole_reference(planes, temporal=False)), 50.0, 0, 0, 21, RECT, calls=2)
    with pytest.raises(ValueError, match="progressive"):
        DeinterlacingReader(open_y4m(_write(tmp_path / "p.y4m", planes, "p"), interlaced=True), CROP, "bob")
    with pytest.raises(ValueError, match="one of"):
        DeinterlacingReader(open_y4m(path, interlaced=True), CROP, "blend")


@pytest.mark.parametrize("crop", [[(0, 0), (9, 7)], [(19, 13), (28, 20)], [(0, 5), (28, 12)], [(7, 0), (16, 20)], [(5, 3), (14, 10)],
                                  [(11, 7), (12, 8)]])
def test_cropped_equals_whole_frame_reference_cropped(tmp_path, crop):
    """crop regions touching each picture edge, at odd origins, and of one pixel; from a file (whole frames) and from a pipe (frames
    that hold the margin rectangle plus the footprint), 4:2:0 and 4:2:2 at 10 bits"""
    from swiftwatcher_amd.deinterlace import DeinterlacingReader
    from swiftwatcher_amd.io_roi_stream import margin_rect
    from swiftwatcher_amd.io_y4m import open_y4m
    N = 4
    for chroma, bits in (("420", 8), ("422", 10)):
        src = cases.Source("420" if chroma == "420" else "422", N, 20, 28, seed=len(crop[0]) + crop[0][0])
        if bits == 10:
            r = cases.rng("ten", crop)
            vals = tuple(r.integers(0, 1024, size=p.shape, dtype=np.int64) for p in src.values)
        else:
            vals = src.values
        dt = np.uint16 if bits > 8 else np.uint8
        path = _write(tmp_path / ("%s.y4m" % chroma), tuple(p.astype(dt) for p in vals), "t", chroma=chroma, bits=bits)
        whole = ref.call_bgr(*vals, subsampling=(1, 1) if chroma == "420" else (1, 0), bits=bits, tff=True)
        rect = margin_rect((20, 28), crop, (6, 6))
        for source in (path, io.BytesIO(open(path, "rb").read())):
            wrapped = open_y4m(source, interlaced=True)
            reader = DeinterlacingReader(wrapped, None, "bob", backend=RefBackend())
            reader.set_region(crop, (6, 6))
            frames, numbers, _ = reader.get_n_frames(2 * N)
            assert numbers == list(range(2 * N))
            for k, f in enumerate(frames):
                assert f.origin == (rect[0], rect[2]) and np.array_equal(_cut(f, rect), whole[k][rect[0]:rect[1], rect[2]:rect[3]]), (chroma, k)
            if hasattr(wrapped, "close"):
                wrapped.close()


# ------------------------------------------------------------------------------------------------ what it buys
SCENE_HW = (64, 128)


@pytest.fixture(scope="module")
def scene():
    """A noise-free scene rendered at field rate (synthetic.py): a static textured chimney, birds moving several pixels per field.
    21 stored frames = 42 field-rate pictures, as 4:2:0; the stored frames are the pictures woven plane by plane (top field first).
    Returns the field-rate pictures' planes and BGR, the stored planes, and per picture the mask of pixels a bird covers."""
    from swiftwatcher_amd import synthetic
    import yuv_ref
    Hc, Wc = SCENE_HW
    kw = dict(bird_len=(8, 12), bird_wid=(4, 6), noise=0.0)
    shown = synthetic.roi_window(11, 42, Hc, Wc, birds=5, **kw)[::-1]          # (oldest first)
    empty = synthetic.roi_window(11, 42, Hc, Wc, birds=0, **kw)[::-1]
    assert (empty == empty[0]).all()
    birds = (shown != empty).any(axis=-1)
    y, u, v = yuv_ref.bgr_to_yuv420(np.ascontiguousarray(shown))
    stored = tuple(ref.weave(p[0::2], p[1::2]) for p in (y, u, v))
    progressive = yuv_ref.bgr(y, u, v)
    return dict(planes=(y, u, v), progressive=progressive, stored=stored, birds=birds)


def _bob(scene, temporal):
    y, u, v = (p.astype(np.int64) for p in scene["stored"])
    return ref.call_bgr(y, u, v, subsampling=(1, 1), tff=True, temporal=temporal)


def _clean(scene):
    """per output picture k (of stored frame t = k // 2): the pixels whose footprint -- rows y - 1 .. y + 1 and columns x - 3 .. x + 3
    of the luma plane, and the same of the chroma planes, which is +-3 rows and +-7 columns of luma and one more for the cell -- no
    bird touches in the stored frames t - 1, t, t + 1, that is in the field-rate pictures 2t - 2 .. 2t + 3"""
    from scipy import ndimage
    birds = scene["birds"]
    out = np.zeros(birds.shape, bool)
    for k in range(len(birds)):
        t = k // 2
        near = birds[max(2 * t - 2, 0):2 * t + 4].any(axis=0)
        out[k] = ~ndimage.binary_dilation(near, structure=np.ones((9, 17), bool))
    return out


def test_adaptive_bob_is_exact_where_nothing_moves(scene):
    adaptive, spatial, prog = _bob(scene, True), _bob(scene, False), scene["progressive"]
    clean = _clean(scene)
    assert clean.mean() > 0.3 and (~clean).mean() > 0.05
    assert np.array_equal(adaptive[clean], prog[clean])
    # ... where spatial bob is not: in every picture the chimney's top edge, of which every other row is interpolated, differs
    Hc, Wc = SCENE_HW
    top = int(round(Hc * 0.8))
    differs = (spatial != prog).any(axis=-1) & clean
    assert differs[:, top - 1:top + 1, :].any(axis=(1, 2)).all()


def test_adaptive_bob_gives_the_segment_stage_less_to_chew(scene):
    """Through the oracle's segment stage over the first 21 pictures: flicker of still edges at field rate lands in the sparse term
    (DESIGN.md section 18 records the three counts)"""
    from oracle import reference_path as orc
    counts = {}
    for name, pics in (("progressive", scene["progressive"]), ("adaptive", _bob(scene, True)), ("spatial", _bob(scene, False))):
        res = orc.window(np.ascontiguousarray(pics[:21][::-1]))          # (queue order: newest first)
        counts[name] = sum(len(s) for s in res["segments"])
    print("segments over 21 pictures:", counts)
    assert counts["adaptive"] <= counts["spatial"] and counts["adaptive"] < counts["spatial"]
