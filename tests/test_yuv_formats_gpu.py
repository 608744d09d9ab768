"""swk_yuv_to_bgr (k_yuv_to_bgr, csrc/yuv.hip) and the ingest of the YUV formats beyond 8-bit 4:2:0 on the MI355X.  Every comparison
is bit for bit against the restatement tests/yuv_formats_ref.py; the batch path over a .y4m file is compared with the same calls
over the restated BGR frames."""
import ctypes

import numpy as np
import pytest

import yuv_formats_ref as ref

pytestmark = pytest.mark.gpu

CROP = [(30, 20), (30 + 96, 20 + 64)]
CROP_ODD = [(31, 21), (31 + 96, 21 + 64)]
ALL_SS = [(0, 0), (1, 0), (2, 0), (0, 1), (1, 1), (2, 1)]


@pytest.fixture(scope="module")
def ctx():
    from swiftwatcher_amd import _lib
    return _lib.default_context(0)


def _planes(seed, count, H, W, ss=(1, 1), bits=8, top=None):
    rng = np.random.default_rng(seed)
    dt = np.uint16 if bits > 8 else np.uint8
    hi = (1 << bits) if top is None else top
    cs = ref.chroma_shape(H, W, *ss)
    return (rng.integers(0, hi, (count, H, W)).astype(dt), rng.integers(0, hi, (count,) + cs).astype(dt),
            rng.integers(0, hi, (count,) + cs).astype(dt))


def _semi(u, v):
    return np.ascontiguousarray(np.stack([u, v], axis=-1))


# ------------------------------------------------------------------------------------------------------- values
@pytest.mark.parametrize("full_range", [False, True], ids=["limited", "full"])
def test_every_8_bit_triple(ctx, full_range):
    """2^24 pixels of 4:4:4 (64 frames of 512 x 512) hold every (Y, U, V) exactly once: pixel i has Y = i >> 16, U = (i >> 8) & 255,
    V = i & 255."""
    i = np.arange(1 << 24, dtype=np.uint32).reshape(64, 512, 512)
    y, u, v = (i >> 16).astype(np.uint8), ((i >> 8) & 255).astype(np.uint8), (i & 255).astype(np.uint8)
    want = ref.bgr(y, u, v, None, (0, 0), 8, full_range)
    assert np.array_equal(ctx.yuv_to_bgr(y, u, v, subsampling=(0, 0), full_range=full_range), want)
    assert np.array_equal(ctx.yuv_to_bgr(y, _semi(u, v), subsampling=(0, 0), full_range=full_range), want)


def _lattice_10():
    lat = np.arange(4, 1023, 8)
    lat[[0, 63, 64, 127]] = [0, 511, 512, 1023]
    assert len(lat) == 128 and len(set(lat.tolist())) == 128
    return lat.astype(np.uint16)


@pytest.fixture(scope="module")
def ten_bit():
    """Every Y of 0 .. 1023 (one frame each) against a 128 x 128 lattice of (U, V) that includes 0, 511, 512 and 1023, as 4:4:4
    planes; the restated BGR per range, computed once."""
    lat = _lattice_10()
    y = np.ascontiguousarray(np.broadcast_to(np.arange(1024, dtype=np.uint16)[:, None, None], (1024, 128, 128)))
    u = np.ascontiguousarray(np.broadcast_to(lat[None, :, None], (1024, 128, 128)))
    v = np.ascontiguousarray(np.broadcast_to(lat[None, None, :], (1024, 128, 128)))
    want = {full: ref.bgr(y, u, v, None, (0, 0), 10, full) for full in (False, True)}
    for w in want.values():
        w.setflags(write=False)
    return y, u, v, want


@pytest.mark.parametrize("full_range", [False, True], ids=["limited", "full"])
@pytest.mark.parametrize("msb", [False, True], ids=["lsb", "msb"])
def test_10_bit_values(ctx, ten_bit, msb, full_range):
    y, u, v, want = ten_bit
    if msb:
        y, u, v = y << 6, u << 6, v << 6
    kw = dict(subsampling=(0, 0), bits=10, msb_aligned=msb, full_range=full_range)
    assert np.array_equal(ctx.yuv_to_bgr(y, u, v, **kw), want[full_range])
    assert np.array_equal(ctx.yuv_to_bgr(y, _semi(u, v), **kw), want[full_range])


@pytest.mark.parametrize("bits,msb", [(16, False), (16, True), (12, True), (14, False), (9, True)])
def test_16_bit_values_and_the_depths_between(ctx, bits, msb):
    """64 values per component, 0, the two middle values and the largest among them: every combination, both ranges.  The values
    run over the whole 16-bit word at any depth (samples are taken as stored: LSB-aligned values above 2^bits - 1 are not masked)."""
    vals = np.round(np.linspace(0, 65535, 64)).astype(np.int64)
    vals[[31, 32]] = [32767, 32768]
    assert {0, 32767, 32768, 65535} <= set(vals.tolist()) and len(set(vals.tolist())) == 64
    if msb:
        vals = (vals >> (16 - bits)) << (16 - bits)
    vals = vals.astype(np.uint16)
    Y, U, V = np.meshgrid(vals, vals, vals, indexing="ij")          # (64, 64, 64): 64 frames of 64 x 64
    Y, U, V = (np.ascontiguousarray(a) for a in (Y, U, V))
    for full in (False, True):
        want = ref.bgr(Y, U, V, None, (0, 0), bits, full, msb)
        kw = dict(subsampling=(0, 0), bits=bits, msb_aligned=msb, full_range=full)
        assert np.array_equal(ctx.yuv_to_bgr(Y, U, V, **kw), want)
        assert np.array_equal(ctx.yuv_to_bgr(Y, _semi(U, V), **kw), want)
        mono = ctx.yuv_to_bgr(Y, bits=bits, msb_aligned=msb, full_range=full)
        assert np.array_equal(mono, ref.bgr(Y, None, None, None, (0, 0), bits, full, msb))


@pytest.mark.parametrize("bits", [9, 10, 12, 14, 16])
def test_samples_shifted_up_give_the_8_bit_bytes(ctx, bits):
    for ss in ((1, 1), (1, 0), (2, 0)):
        y, u, v = _planes(bits, 2, 37, 53, ss)
        k = bits - 8
        wide = [p.astype(np.uint16) << k for p in (y, u, v)]
        for full in (False, True):
            want = ctx.yuv_to_bgr(y, u, v, subsampling=ss, full_range=full)
            assert np.array_equal(want, ref.bgr(y, u, v, None, ss, 8, full))
            assert np.array_equal(ctx.yuv_to_bgr(*wide, subsampling=ss, bits=bits, full_range=full), want)


@pytest.mark.parametrize("H,W,rect", [(47, 94, None), (67, 131, (1, 1, 130, 65)), (110, 160, (9, 5, 100, 41)), (5, 9, (3, 0, 6, 5))])
def test_equals_the_420_entry_point(ctx, H, W, rect):
    import torch
    y, u, v = _planes(H + W, 3, H, W)
    uv = _semi(u, v)
    old = ctx.yuv420_to_bgr(y, u, v, rect=rect)
    assert np.array_equal(ctx.yuv_to_bgr(y, u, v, rect=rect), old)
    assert np.array_equal(ctx.yuv420_to_bgr(y, uv, rect=rect), old)
    assert np.array_equal(ctx.yuv_to_bgr(y, uv, rect=rect), old)
    assert np.array_equal(ctx.yuv_to_bgr(y, uv.reshape(3, u.shape[1], -1), rect=rect), old)
    t = lambda a: torch.from_numpy(a).to("cuda:0")          # noqa: E731
    assert np.array_equal(ctx.yuv_to_bgr(t(y), t(u), t(v), rect=rect, device_out=True).cpu().numpy(), old)
    assert np.array_equal(ctx.yuv_to_bgr(t(y), t(uv), rect=rect, device_out=True).cpu().numpy(), old)


# ------------------------------------------------------------------------------------------------------- geometry
def _rects(H, W):
    out = set()
    for x0 in range(4):
        for w in range(1, 10):                                       # every origin mod 4 with every width 1 .. 9
            y0 = (x0 + w) & 1
            out.add((x0, y0, w, min(3, H - y0)))
    for y0 in (0, 1):
        for x0 in range(4):
            out.add((x0, y0, W - x0, H - y0))                        # ends at the last row and column
            out.add((x0, y0, W - x0 - 1, H - y0 - 1))                # the other parity of Hr / Wr
            out.add((W - 1 - x0, H - 1 - y0, x0 + 1, y0 + 1))        # the last few columns and rows alone
    out |= {(0, 0, W, H), (0, 0, 1, 1), (W - 1, H - 1, 1, 1)}
    return sorted(r for r in out if r[0] >= 0 and r[1] >= 0 and r[2] >= 1 and r[3] >= 1 and r[0] + r[2] <= W and r[1] + r[3] <= H)


@pytest.mark.parametrize("H,W", [(1, 1), (2, 2), (3, 5), (5, 9), (47, 94), (67, 131)])
def test_geometry(ctx, H, W):
    rects = _rects(H, W)
    if H >= 47:
        assert {(r[0] & 3, r[1] & 1) for r in rects} == {(a, b) for a in range(4) for b in range(2)}
        assert {(x0 & 3, w) for x0, _, w, _ in rects if w <= 9} >= {(a, w) for a in range(4) for w in range(1, 10)}
        ends = [r for r in rects if r[0] + r[2] == W and r[1] + r[3] == H]
        assert {(r[2] & 1, r[3] & 1) for r in ends} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    for bits in (8, 10):
        for ss in ALL_SS:
            y, u, v = _planes(H * 1000 + W + bits, 2, H, W, ss, bits)
            uv = _semi(u, v)
            kw = dict(subsampling=ss, bits=bits, full_range=bits == 10)
            for rect in rects:
                want = ref.bgr(y, u, v, rect, ss, bits, bits == 10)
                got = ctx.yuv_to_bgr(y, u, v, rect=rect, **kw)
                assert got.shape == want.shape and np.array_equal(got, want), ("planar", bits, ss, rect)
                assert np.array_equal(ctx.yuv_to_bgr(y, uv, rect=rect, **kw), want), ("semiplanar", bits, ss, rect)
        y = _planes(H + W, 2, H, W, (0, 0), bits)[0]
        for rect in rects:
            assert np.array_equal(ctx.yuv_to_bgr(y, rect=rect, bits=bits), ref.bgr(y, None, None, rect, (0, 0), bits)), ("mono", bits, rect)
    one = ctx.yuv_to_bgr(y[1], bits=10)
    assert one.shape == (H, W, 3) and np.array_equal(one, ref.bgr(y[1], bits=10))


def test_geometry_on_device_planes(ctx):
    """The kernel addresses device planes at the rectangle's own origin (a host source is cut to the rectangle first)."""
    import torch
    H, W = 47, 94
    rects = _rects(H, W)
    t = lambda a: torch.from_numpy(a).to("cuda:0")          # noqa: E731
    for bits, ss in [(8, (0, 0)), (8, (1, 0)), (8, (2, 1)), (10, (1, 1)), (10, (2, 0)), (10, (0, 1))]:
        y, u, v = _planes(bits + ss[0], 2, H, W, ss, bits)
        ty, tu, tv, tuv = t(y), t(u), t(v), t(_semi(u, v))
        kw = dict(subsampling=ss, bits=bits)
        for rect in rects:
            want = ref.bgr(y, u, v, rect, ss, bits)
            assert np.array_equal(ctx.yuv_to_bgr(ty, tu, tv, rect=rect, **kw), want), ("planar", bits, ss, rect)
            assert np.array_equal(ctx.yuv_to_bgr(ty, tuv, rect=rect, **kw), want), ("semiplanar", bits, ss, rect)


# ------------------------------------------------------------------------------------------------------- memory
@pytest.mark.parametrize("H,W,rect,ss,bits,msb,full", [
    (47, 94, (3, 5, 80, 41), (1, 0), 8, False, True),
    (67, 131, (0, 1, 131, 66), (1, 1), 10, True, False),
    (67, 131, (65, 32, 66, 35), (0, 0), 12, False, False),
    (16, 64, (0, 0, 64, 16), (2, 0), 8, False, False),
    (33, 70, (5, 2, 61, 30), (0, 1), 16, True, True),
])
def test_layouts_memory_and_strides(ctx, H, W, rect, ss, bits, msb, full):
    import torch
    count = 4
    y, u, v = _planes(H * 7 + W, count, H, W, ss, bits)
    if msb:
        y, u, v = (p << (16 - bits) for p in (y, u, v))
    ch, cw = u.shape[1:]
    want = ref.bgr(y, u, v, rect, ss, bits, full, msb)
    want_mono = ref.bgr(y, None, None, rect, ss, bits, full, msb)
    dev = "cuda:0"

    def pitched(a, rows_extra, cols_extra, xp):
        """the same values in a buffer with a larger row pitch and frame stride"""
        big = np.full((a.shape[0], a.shape[1] + rows_extra, a.shape[2] + cols_extra), 0xA5, a.dtype)
        big[:, :a.shape[1], :a.shape[2]] = a
        if xp is not np:
            big = torch.from_numpy(big).to(dev)
        return big[:, :a.shape[1], :a.shape[2]]

    t = lambda a: torch.from_numpy(a).to(dev)          # noqa: E731
    uv = _semi(u, v)
    flat = uv.reshape(count, ch, 2 * cw)
    cases = {
        "host planar dense": (y, u, v),
        "host semiplanar dense": (y, uv, None),
        "host semiplanar flat": (y, flat, None),
        "host planar pitched, own chroma frame stride": (pitched(y, 0, 13, np), pitched(u, 3, 11, np), pitched(v, 3, 11, np)),
        "host semiplanar pitched": (pitched(y, 2, 13, np), pitched(flat, 1, 14, np), None),
        "host mono pitched": (pitched(y, 1, 7, np), None, None),
        "device planar dense": (t(y), t(u), t(v)),
        "device semiplanar dense": (t(y), t(uv), None),
        "device planar pitched, own chroma frame stride": (pitched(y, 0, 13, torch), pitched(u, 3, 11, torch), pitched(v, 3, 11, torch)),
        "device semiplanar pitched": (pitched(y, 2, 13, torch), pitched(flat, 1, 14, torch), None),
        "device mono pitched": (pitched(y, 1, 7, torch), None, None),
    }
    kw = dict(subsampling=ss, bits=bits, msb_aligned=msb, full_range=full, rect=rect)
    for name, (py, pu, pv) in cases.items():
        expect = want_mono if pu is None else want
        host = ctx.yuv_to_bgr(py, pu, pv, **kw)
        assert isinstance(host, np.ndarray) and np.array_equal(host, expect), name
        on_gpu = ctx.yuv_to_bgr(py, pu, pv, device_out=True, **kw)
        assert on_gpu.is_cuda and on_gpu.dtype == torch.uint8 and tuple(on_gpu.shape) == expect.shape, name
        assert np.array_equal(on_gpu.cpu().numpy(), expect), name
    # a window read backwards (negative frame stride), as the batch calls take them
    assert np.array_equal(ctx.yuv_to_bgr(y[::-1], u[::-1], v[::-1], **kw), want[::-1])


def test_product_host_conversion_equals_the_kernel(ctx):
    from swiftwatcher_amd.io_y4m import YuvFrame
    for (H, W), ss, bits, full in [((67, 131), (1, 0), 10, True), ((110, 160), (0, 0), 8, False), ((33, 47), (2, 0), 8, True),
                                   ((67, 131), (1, 1), 16, False)]:
        y, u, v = _planes(H + W, 1, H, W, ss, bits)
        frame = YuvFrame(y[0], u[0], v[0], ss, bits, full)
        got = ctx.yuv_to_bgr(y[0], u[0], v[0], subsampling=ss, bits=bits, full_range=full)
        assert np.array_equal(np.asarray(frame), got)
        assert np.array_equal(frame[5:30, 9:40], got[5:30, 9:40])
        mono = YuvFrame(y[0], bits=bits, full_range=full)
        assert np.array_equal(np.asarray(mono), ctx.yuv_to_bgr(y[0], bits=bits, full_range=full))


# ------------------------------------------------------------------------------------------------------- refusals
def test_refusals_launch_nothing_and_leave_the_context_usable(ctx):
    from swiftwatcher_amd import _lib
    y, u, v = _planes(11, 2, 10, 12, (1, 0), 10)          # 4:2:2, two-byte samples: u, v are (2, 10, 6)
    uv = _semi(u, v)
    good = dict(subsampling=(1, 0), bits=10)
    out = np.full((2, 10, 12, 3), 0x5A, np.uint8)

    def raw(count=2, rect=(0, 0, 12, 10), **over):
        f = dict(y=y.ctypes.data, u=u.ctypes.data, v=v.ctypes.data, mem=_lib.MEM_HOST, layout=_lib.YUV_PLANAR, H=10, W=12,
                 y_row_stride=24, y_frame_stride=240, c_row_stride=12, c_frame_stride=120, sx=1, sy=0, bits=10, msb_aligned=0, full_range=0)
        f.update(over)
        src = _lib.Yuv(**f)
        rc = ctx._lib.swk_yuv_to_bgr(ctx._h, ctypes.byref(src), count, rect[0], rect[1], rect[3], rect[2], out.ctypes.data, _lib.MEM_HOST)
        return rc, ctx._lib.swk_last_error(ctx._h).decode()

    ctx.prof_enable(True)
    try:
        ctx.prof_reset()
        refused = [
            (dict(bits=7), "bits"), (dict(bits=17), "bits"), (dict(bits=0), "bits"),
            (dict(sx=3), "subsampling"), (dict(sx=-1), "subsampling"), (dict(sy=2), "subsampling"), (dict(sy=-1), "subsampling"),
            (dict(layout=3), "layout"), (dict(layout=-1), "layout"),
            (dict(y=None), "plane"), (dict(u=None), "plane"), (dict(v=None), "plane"),
            (dict(layout=_lib.YUV_SEMIPLANAR, u=None, v=None, c_row_stride=24), "plane"),
            (dict(layout=_lib.YUV_MONO, y=None), "plane"),
            (dict(y_row_stride=22), "stride"), (dict(c_row_stride=10), "stride"),
            (dict(layout=_lib.YUV_SEMIPLANAR, u=uv.ctypes.data, v=None, c_row_stride=22), "stride"),          # a row of (U, V) pairs is 24 bytes
            (dict(y_row_stride=25), "odd"), (dict(c_row_stride=13), "odd"), (dict(y_frame_stride=241), "odd"), (dict(c_frame_stride=121), "odd"),
            (dict(y=y.ctypes.data + 1), "odd"), (dict(u=u.ctypes.data + 1), "odd"), (dict(v=v.ctypes.data + 1), "odd"),
            (dict(layout=_lib.YUV_SEMIPLANAR, u=uv.ctypes.data + 1, v=None, c_row_stride=24), "odd"),
        ]
        for over, word in refused:
            rc, msg = raw(**over)
            assert rc == -1 and word in msg, (over, msg)
        for count in (0, -3):
            rc, msg = raw(count=count)
            assert rc == -1 and "count" in msg
        for rect in [(-1, 0, 4, 4), (0, -1, 4, 4), (0, 0, 13, 10), (0, 0, 12, 11), (11, 9, 2, 1), (11, 9, 1, 2), (0, 0, 0, 4), (0, 0, 4, 0)]:
            rc, msg = raw(rect=rect)
            assert rc == -1 and "rectangle" in msg, rect
            with pytest.raises(_lib.SwkError) as err:
                ctx.yuv_to_bgr(y, u, v, rect=rect, **good)
            assert "rectangle" in str(err.value), rect
        for kw in (dict(bits=17), dict(subsampling=(3, 0)), dict(subsampling=(1, 2))):
            with pytest.raises(_lib.SwkError):
                ctx.yuv_to_bgr(y, u, v, **dict(good, **kw))
        assert ctx.prof()["gray"][1] == 0, "a refused call launched a kernel"
        assert (out == 0x5A).all()
        # what is not refused: 8-bit samples at odd addresses and strides, mono with no chroma planes, one frame with any frame stride
        assert raw()[0] == 0 and np.array_equal(out, ref.bgr(y, u, v, None, (1, 0), 10))
        assert raw(layout=_lib.YUV_MONO, u=None, v=None, c_row_stride=0, c_frame_stride=0)[0] == 0 and np.array_equal(out, ref.bgr(y, bits=10))
        assert raw(count=1, y_frame_stride=241, c_frame_stride=121)[0] == 0
        assert ctx.prof()["gray"][1] == 3
    finally:
        ctx.prof_enable(False)
    y8, u8, v8 = _planes(12, 2, 9, 11, (1, 1))
    odd = (y8[:, 1:, 1:], u8[:, 1:, 1:], v8[:, 1:, 1:])          # 8 x 10 pictures at odd addresses, 11 and 6 bytes between rows
    assert np.array_equal(ctx.yuv_to_bgr(*odd, rect=(1, 0, 9, 8)), ref.bgr(*odd, (1, 0, 9, 8)))
    with pytest.raises(ValueError):
        ctx.yuv_to_bgr(y, u[:, :, :4], v[:, :, :4], **good)
    with pytest.raises(ValueError):
        ctx.yuv_to_bgr(y, u, **good)                                       # no v: semiplanar is asked for, the plane is not interleaved
    with pytest.raises(ValueError):
        ctx.yuv_to_bgr(y, None, v, **good)
    # the context still works
    assert np.array_equal(ctx.yuv_to_bgr(y, u, v, rect=(1, 1, 9, 7), **good), ref.bgr(y, u, v, (1, 1, 9, 7), (1, 0), 10))
    res = ctx.batch_run(np.ascontiguousarray(ref.bgr(y, u, v, None, (1, 0), 10)[:, :8, :8]), 1, 2, stages=("gray",))
    assert res["gray"].shape == (2, 8, 8)


# ------------------------------------------------------------------------------------------------------- the batch path
FORMATS = {"C422p10-full": ("422", 10, True), "C444": ("444", 8, False), "Cmono": ("mono", 8, False), "C420p10": ("420", 10, False)}


@pytest.fixture(scope="module")
def source():
    """The seeded 52-frame 110 x 160 BGR clip every format's file is made from."""
    from swiftwatcher_amd import synthetic
    return synthetic.full_frames(500, 52, CROP, frame_hw=(110, 160), birds=4, bird_len=(8, 12), bird_wid=(3, 5))[::-1].copy()


@pytest.fixture(scope="module")
def clips(source, tmp_path_factory):
    """Per format: its .y4m file, its planes, and the BGR frames those planes restate to."""
    from swiftwatcher_amd.io_y4m import Y4MWriter
    out = {}
    folder = tmp_path_factory.mktemp("y4m_formats")
    for name, (chroma, bits, full) in FORMATS.items():
        mono = chroma == "mono"
        ss = (0, 0) if mono else ref.SUBSAMPLINGS[chroma]
        y, u, v = ref.bgr_to_planes(source, ss, bits, full, mono)
        path = str(folder / (name + ".y4m"))
        with Y4MWriter(path, 160, 110, 30, chroma=chroma, bits=bits, full_range=full) as w:
            for k in range(len(y)):
                w.append(y[k]) if mono else w.append(y[k], u[k], v[k])
        bgr = ref.bgr(y, u, v, None, ss, bits, full)
        bgr.setflags(write=False)
        out[name] = dict(path=path, y=y, u=u, v=v, ss=ss, bits=bits, full=full, bgr=bgr)
    return out


def _seg_records(frame):
    return [(s.label, tuple(s.bbox), tuple(s.centroid), s.area, s.parent_frame_number, str(s.parent_timestamp)) for s in frame.segments]


def _queue_run(reader, n, crop, windows, classifier=None):
    from swiftwatcher_amd.data_structures import FrameQueue, STAGE_KEYS
    q = FrameQueue(n)
    out = []
    for _ in range(windows):
        frames, numbers, stamps = reader.get_n_frames(n)
        q.push_list_of_frames(frames, numbers, stamps)
        q.preprocess_queue(crop, None)
        q.segment_queue((24, 24), crop)
        table = None
        if classifier is not None:
            assert q._last_batch is not None
            table = q._last_batch.predictions(classifier)
        win = dict(iters=q.last_iters, table=table, frames=[])
        while not q.is_empty():
            f = q.pop_frame()
            rec = dict(number=f.frame_number, segs=_seg_records(f), stages={name: np.array(f.processed_frames[name]) for name in STAGE_KEYS.values()},
                       crop=np.array(f.processed_frames["crop"]), images=[np.array(s.segment_image) for s in f.segments])
            if classifier is not None:
                rec["kept"] = [tuple(s.bbox) for s in classifier(f.segments)]
            win["frames"].append(rec)
        out.append(win)
    return out


def _same_windows(a, b):
    assert len(a) == len(b)
    for wa, wb in zip(a, b):
        assert wa["iters"] == wb["iters"]
        assert (wa["table"] is None) == (wb["table"] is None)
        if wa["table"] is not None:
            assert np.array_equal(wa["table"], wb["table"])
        assert len(wa["frames"]) == len(wb["frames"])
        for fa, fb in zip(wa["frames"], wb["frames"]):
            assert fa["number"] == fb["number"] and fa["segs"] == fb["segs"], fa["number"]
            assert fa.get("kept") == fb.get("kept")
            assert np.array_equal(fa["crop"], fb["crop"])
            for name in fa["stages"]:
                assert np.array_equal(fa["stages"][name], fb["stages"][name]), (fa["number"], name)
            assert len(fa["images"]) == len(fb["images"]) and all(np.array_equal(x, z) for x, z in zip(fa["images"], fb["images"]))


@pytest.mark.parametrize("n,windows", [(21, 3), (5, 4)])
@pytest.mark.parametrize("crop", [CROP, CROP_ODD], ids=["even", "odd"])
@pytest.mark.parametrize("fmt", sorted(FORMATS))
def test_frame_queue_over_a_file_of_each_format(clips, fmt, n, windows, crop):
    from swiftwatcher_amd.io_frames import ArrayReader
    from swiftwatcher_amd.io_y4m import YuvReader, open_y4m
    clip = clips[fmt]
    want = _queue_run(ArrayReader(list(clip["bgr"]), fps=30.0), n, crop, windows)
    assert any(f["segs"] for w in want for f in w["frames"]), "no frame of the BGR run has a region"
    reader = open_y4m(clip["path"])
    assert type(reader) is YuvReader
    _same_windows(_queue_run(reader, n, crop, windows), want)


def _triples(reader, n, windows):
    return [reader.get_n_frames(n) for _ in range(windows)]


def _popped_records(popped_lists):
    return [[(f.frame_number, _seg_records(f), [np.array(s.segment_image).tobytes() for s in f.segments]) for f in popped] for popped in popped_lists]


@pytest.fixture(scope="module")
def other_video():
    from swiftwatcher_amd import synthetic
    from swiftwatcher_amd.data_structures import segment_windows
    from swiftwatcher_amd.io_frames import ArrayReader
    crop2 = [(21, 11), (21 + 80, 11 + 48)]
    other = synthetic.full_frames(77, 42, crop2, frame_hw=(90, 140), birds=3, bird_len=(8, 12), bird_wid=(3, 5))[::-1].copy()
    lone = _popped_records(segment_windows(_triples(ArrayReader(list(other), fps=30.0), 21, 2), crop2))
    assert any(segs for popped in lone for _, segs, _ in popped)
    return other, crop2, lone


@pytest.mark.parametrize("fmt", sorted(FORMATS))
def test_groups_call_mixing_each_format_with_a_bgr_video(clips, other_video, fmt):
    from swiftwatcher_amd.data_structures import segment_window_groups, segment_windows
    from swiftwatcher_amd.io_frames import ArrayReader
    from swiftwatcher_amd.io_y4m import open_y4m
    clip = clips[fmt]
    other, crop2, lone_bgr = other_video
    n = 21
    lone_restated = _popped_records(segment_windows(_triples(ArrayReader(list(clip["bgr"]), fps=30.0), n, 2), CROP))
    assert any(segs for popped in lone_restated for _, segs, _ in popped), "no frame of the BGR run has a region"
    assert _popped_records(segment_windows(_triples(open_y4m(clip["path"]), n, 2), CROP)) == lone_restated
    for order in (0, 1):
        groups = [(_triples(open_y4m(clip["path"]), n, 2), CROP), (_triples(ArrayReader(list(other), fps=30.0), n, 2), crop2)]
        out = segment_window_groups(groups[::-1] if order else groups)
        got = [_popped_records(g) for g in (out[::-1] if order else out)]
        assert got[0] == lone_restated and got[1] == lone_bgr


def _event_records(events):
    return [[(s.parent_frame_number, str(s.parent_timestamp), tuple(s.centroid), tuple(s.bbox), np.array(s.segment_image).tobytes()) for s in ev]
            for ev in events]


@pytest.mark.parametrize("fmt", sorted(FORMATS))
def test_count_swifts_over_a_file_of_each_format(clips, fmt):
    """52 frames = two windows and a padded one, one and two windows per call; the reader, its path and the restated BGR list."""
    from swiftwatcher_amd import pipeline
    from swiftwatcher_amd.io_y4m import open_y4m
    clip = clips[fmt]
    roi_mask = np.zeros((64, 96), np.uint8)
    roi_mask[28:, :] = 255
    seen = []
    for wpc in (1, 2):
        want = pipeline.count_swifts(list(clip["bgr"]), CROP, roi_mask, fps=30.0, windows_per_call=wpc)
        assert any(len(ev) for ev in want[1]), "the BGR run found no region"
        for src in (open_y4m(clip["path"]), clip["path"]):
            got = pipeline.count_swifts(src, CROP, roi_mask, windows_per_call=wpc)
            assert got[0] == want[0] and _event_records(got[1]) == _event_records(want[1])
        seen.append((want[0], _event_records(want[1])))
    assert seen[0] == seen[1]
    print("%s: count %d, %d events" % (fmt, seen[0][0], len(seen[0][1])))


def test_full_range_420_file_by_path_is_converted_as_full_range(source, tmp_path):
    """A C420jpeg XCOLORRANGE=FULL file (what ffmpeg writes for yuvj420p) given by path: full range; Y4MReader itself: as before."""
    from swiftwatcher_amd import pipeline
    from swiftwatcher_amd.io_y4m import Y4MReader, Y4MWriter
    y, u, v = ref.bgr_to_planes(source, (1, 1), 8, True)
    path = str(tmp_path / "j.y4m")
    with Y4MWriter(path, 160, 110, 30, full_range=True) as w:
        for k in range(len(y)):
            w.append(y[k], u[k], v[k])
    roi_mask = np.zeros((64, 96), np.uint8)
    roi_mask[28:, :] = 255
    for full, src in ((True, path), (False, Y4MReader(path))):
        want = pipeline.count_swifts(list(ref.bgr(y, u, v, full_range=full)), CROP, roi_mask, fps=30.0)
        assert any(len(ev) for ev in want[1]), "the BGR run found no region"
        got = pipeline.count_swifts(src, CROP, roi_mask)
        assert got[0] == want[0] and _event_records(got[1]) == _event_records(want[1])


def test_presegmenting_reader_over_a_10_bit_file(clips):
    from swiftwatcher_amd.io_frames import ArrayReader, PresegmentingReader
    from swiftwatcher_amd.io_y4m import open_y4m
    clip = clips["C420p10"]
    runs = []
    for inner in (open_y4m(clip["path"]), ArrayReader(list(clip["bgr"]), fps=30.0)):
        reader = PresegmentingReader(inner, crop_region=CROP, queue_size=21, windows=2)
        runs.append(_queue_run(reader, 21, CROP, 3))
        reader.close()
    assert any(f["segs"] for w in runs[1] for f in w["frames"])
    _same_windows(runs[0], runs[1])


def test_a_window_that_mixes_formats_is_refused(clips):
    from swiftwatcher_amd.data_structures import stack_frames
    from swiftwatcher_amd.io_y4m import open_y4m
    from swiftwatcher_amd import _lib
    a = open_y4m(clips["C420p10"]["path"]).get_n_frames(3)[0]
    b = open_y4m(clips["C444"]["path"]).get_n_frames(3)[0]
    c = open_y4m(clips["C420p10"]["path"], full_range=True).get_n_frames(3)[0]
    ctx = _lib.default_context(0)
    for mixed in (a[:2] + b[:1], a[:2] + c[:1], a[:2] + [clips["C444"]["bgr"][0]]):
        with pytest.raises(ValueError) as err:
            stack_frames(mixed, CROP, (24, 24), ctx.staging, 0)
        assert "mixes" in str(err.value)
    stack = stack_frames(a, CROP, (24, 24), ctx.staging, 0)[0]
    assert stack.is_cuda and np.array_equal(stack.cpu().numpy(), clips["C420p10"]["bgr"][:3, 8:96, 18:138])


def test_classifier_scores_and_decisions_equal(clips):
    """The window's segments scored through the device hand-over and through the segments' images: the same table, scores and keep
    decisions from the C422p10 full-range file as from the restated BGR frames."""
    import torch
    from oracle import classifier_ref as cref
    from swiftwatcher_amd.io_frames import ArrayReader
    from swiftwatcher_amd.io_y4m import open_y4m
    from swiftwatcher_amd.segment_classification import SegmentClassifier
    clip = clips["C422p10-full"]
    plain = _queue_run(ArrayReader(list(clip["bgr"]), fps=30.0), 21, CROP, 3)
    crops = [im for w in plain for f in w["frames"] for im in f["images"]]
    assert len(crops) > 20
    sd = cref.calibrate_head(cref.random_state_dict(5), crops[::3])
    clf = SegmentClassifier.from_state_dict(sd)
    assert clf.device.type == "cuda"
    want = _queue_run(ArrayReader(list(clip["bgr"]), fps=30.0), 21, CROP, 3, classifier=clf)
    got = _queue_run(open_y4m(clip["path"]), 21, CROP, 3, classifier=clf)
    assert all(w["table"] is not None for w in got if any(f["segs"] for f in w["frames"])), "the device hand-over did not serve the YUV windows"
    _same_windows(got, want)
    mine = [im for w in got for f in w["frames"] for im in f["images"]]
    assert torch.equal(clf.scores(mine), clf.scores(crops))


def test_p010_device_surfaces_into_batch_run(ctx, clips):
    """A hardware decoder's 10-bit surfaces: semiplanar, MSB-aligned, pitched, in device memory -> swk_yuv_to_bgr with a device
    result -> batch_run reading it in place; against batch_run over the restated frames."""
    import torch
    from swiftwatcher_amd import _lib
    clip = clips["C420p10"]
    n = 21
    y = clip["y"][:n] << 6
    uv = _semi(clip["u"][:n], clip["v"][:n]).reshape(n, 55, 160) << 6
    pitch = np.zeros((n, 110 + 55, 192), np.uint16)          # one surface per frame: luma rows, then the chroma rows, 192 words apart
    pitch[:, :110, :160] = y
    pitch[:, 110:, :160] = uv
    surf = torch.from_numpy(pitch).to("cuda:0")
    bgr = ctx.yuv_to_bgr(surf[:, :110, :160], surf[:, 110:, :160], bits=10, msb_aligned=True, device_out=True)
    assert bgr.is_cuda and np.array_equal(bgr.cpu().numpy(), clip["bgr"][:n])
    crop = (CROP[0][0], CROP[0][1], 96, 64)
    want = ctx.batch_run(np.ascontiguousarray(clip["bgr"][:n]), 1, n, crop=crop)
    assert want["nseg"].sum() > 0, "the BGR run found no region"
    got = ctx.batch_run(bgr, 1, n, crop=crop)
    for name in _lib.STAGES + ("iters", "nseg", "segs"):
        assert np.array_equal(got[name], want[name]), name
    # the ROI plus margin alone, as stack_frames asks for it
    part = ctx.yuv_to_bgr(surf[:, :110, :160], surf[:, 110:, :160], bits=10, msb_aligned=True, rect=(18, 8, 120, 88), device_out=True)
    got = ctx.batch_run(part, 1, n, crop=(12, 12, 96, 64))
    for name in _lib.STAGES + ("iters", "nseg", "segs"):
        assert np.array_equal(got[name], want[name]), name
