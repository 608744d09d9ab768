"""swk_yuv420_to_bgr (csrc/yuv.hip) and the 4:2:0 ingest of the batch path on the MI355X.  Every comparison is bit for bit against
the scalar restatement tests/yuv_ref.py; the batch path over a .y4m file is compared with the same calls over the restated BGR
frames."""
import ctypes

import numpy as np
import pytest

import yuv_ref

pytestmark = pytest.mark.gpu

CROP = [(30, 20), (30 + 96, 20 + 64)]
CROP_ODD = [(31, 21), (31 + 96, 21 + 64)]


@pytest.fixture(scope="module")
def ctx():
    from swiftwatcher_amd import _lib
    return _lib.default_context(0)


def _planes(seed, count, H, W):
    rng = np.random.default_rng(seed)
    ch, cw = (H + 1) // 2, (W + 1) // 2
    return (rng.integers(0, 256, (count, H, W), dtype=np.uint8), rng.integers(0, 256, (count, ch, cw), dtype=np.uint8),
            rng.integers(0, 256, (count, ch, cw), dtype=np.uint8))


def _nv12(u, v):
    return np.ascontiguousarray(np.stack([u, v], axis=-1))


def test_every_triple(ctx):
    """64 frames of 512 x 512 whose planes hold every (Y, U, V) exactly once: frame f, chroma cell (i, j) carries U = i, V = j and
    the four luma values 4 f .. 4 f + 3."""
    i, j = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    u = np.ascontiguousarray(np.broadcast_to(i, (64, 256, 256)))
    v = np.ascontiguousarray(np.broadcast_to(j, (64, 256, 256)))
    y = np.empty((64, 512, 512), np.uint8)
    for dr in (0, 1):
        for dc in (0, 1):
            y[:, dr::2, dc::2] = (4 * np.arange(64) + 2 * dr + dc).astype(np.uint8)[:, None, None]
    key = (y.astype(np.int64) << 16) | (np.repeat(np.repeat(u, 2, 1), 2, 2).astype(np.int64) << 8) | np.repeat(np.repeat(v, 2, 1), 2, 2)
    assert np.array_equal(np.sort(key.ravel()), np.arange(1 << 24))
    want = yuv_ref.bgr(y, u, v)
    assert np.array_equal(ctx.yuv420_to_bgr(y, u, v), want)
    assert np.array_equal(ctx.yuv420_to_bgr(y, _nv12(u, v)), want)


def _rects(H, W):
    out = {(0, 0, W, H), (0, 0, 1, 1), (W - 1, H - 1, 1, 1), (W // 2 | 1 if W > 1 else 0, H // 2 | 1 if H > 1 else 0, 1, 1)}
    for px in (0, 1):
        for py in (0, 1):
            x0 = min(px + (2 if W > 4 else 0), W - 1)
            y0 = min(py + (2 if H > 4 else 0), H - 1)
            out.add((x0, y0, W - x0, H - y0))                                   # ends at the last row and column
            out.add((x0, y0, max(W - x0 - 1, 1), max(H - y0 - 1, 1)))          # the other parity of Hr / Wr
            out.add((x0, y0, min(5, W - x0), min(3, H - y0)))
    return sorted(r for r in out if r[0] + r[2] <= W and r[1] + r[3] <= H)


@pytest.mark.parametrize("H,W", [(2, 2), (3, 5), (16, 64), (47, 94), (67, 131)])
def test_geometry(ctx, H, W):
    y, u, v = _planes(H * 1000 + W, 3, H, W)
    uv = _nv12(u, v)
    rects = _rects(H, W)
    assert {(r[0] & 1, r[1] & 1) for r in rects} == {(0, 0), (0, 1), (1, 0), (1, 1)} or min(H, W) < 2
    assert any(r[2] & 1 and r[3] & 1 for r in rects) and any(r[0] + r[2] == W and r[1] + r[3] == H and r[0] & 1 and r[1] & 1 for r in rects)
    for rect in rects:
        want = yuv_ref.bgr(y, u, v, rect)
        got = ctx.yuv420_to_bgr(y, u, v, rect=rect)
        assert got.shape == want.shape and np.array_equal(got, want), ("I420", rect)
        assert np.array_equal(ctx.yuv420_to_bgr(y, uv, rect=rect), want), ("NV12", rect)
    one = ctx.yuv420_to_bgr(y[1], u[1], v[1])
    assert one.shape == (H, W, 3) and np.array_equal(one, yuv_ref.bgr(y[1], u[1], v[1]))


@pytest.mark.parametrize("H,W,rect", [(47, 94, (3, 5, 80, 41)), (67, 131, (0, 1, 131, 66)), (67, 131, (65, 32, 66, 35)), (16, 64, (0, 0, 64, 16))])
def test_layouts_memory_and_strides(ctx, H, W, rect):
    import torch
    count = 4
    y, u, v = _planes(H * 7 + W, count, H, W)
    ch, cw = u.shape[1:]
    want = yuv_ref.bgr(y, u, v, rect)
    dev = "cuda:0"

    def pitched(a, rows_extra, cols_extra, xp):
        """the same values in a buffer with a larger row pitch and frame stride"""
        shape = (a.shape[0], a.shape[1] + rows_extra, a.shape[2] + cols_extra)
        big = np.full(shape, 0xA5, np.uint8) if xp is np else torch.full(shape, 0xA5, dtype=torch.uint8, device=dev)
        view = big[:, :a.shape[1], :a.shape[2]]
        if xp is np:
            view[...] = a
        else:
            view.copy_(torch.from_numpy(a))
        return view

    t = lambda a: torch.from_numpy(a).to(dev)          # noqa: E731
    uv = _nv12(u, v)
    cases = {
        "host I420 dense": (y, u, v),
        "host NV12 dense": (y, uv, None),
        "host NV12 flat": (y, uv.reshape(count, ch, 2 * cw), None),
        "host I420 pitched, own chroma frame stride": (pitched(y, 0, 13, np), pitched(u, 3, 13, np), pitched(v, 3, 13, np)),
        "host NV12 pitched": (pitched(y, 2, 13, np), pitched(uv.reshape(count, ch, 2 * cw), 1, 13, np), None),
        "device I420 dense": (t(y), t(u), t(v)),
        "device NV12 dense": (t(y), t(uv), None),
        "device I420 pitched, own chroma frame stride": (pitched(y, 0, 13, torch), pitched(u, 3, 13, torch), pitched(v, 3, 13, torch)),
        "device NV12 pitched": (pitched(y, 2, 13, torch), pitched(uv.reshape(count, ch, 2 * cw), 1, 13, torch), None),
    }
    for name, (py, pu, pv) in cases.items():
        host = ctx.yuv420_to_bgr(py, pu, pv, rect=rect)
        assert isinstance(host, np.ndarray) and np.array_equal(host, want), name
        on_gpu = ctx.yuv420_to_bgr(py, pu, pv, rect=rect, device_out=True)
        assert on_gpu.is_cuda and on_gpu.dtype == torch.uint8 and tuple(on_gpu.shape) == want.shape, name
        assert np.array_equal(on_gpu.cpu().numpy(), want), name
    # a window read backwards (negative frame stride), as the batch calls take them
    assert np.array_equal(ctx.yuv420_to_bgr(y[::-1], u[::-1], v[::-1], rect=rect), want[::-1])


def test_product_host_conversion_equals_the_kernel(ctx):
    from swiftwatcher_amd.io_y4m import Yuv420Frame
    for H, W in [(67, 131), (110, 160)]:
        y, u, v = _planes(H + W, 1, H, W)
        y[0, :4, :8] = [[0, 15, 16, 17, 234, 235, 236, 255]] * 4
        frame = Yuv420Frame(y[0], u[0], v[0])
        got = ctx.yuv420_to_bgr(y[0], u[0], v[0])
        assert np.array_equal(np.asarray(frame), got)
        assert np.array_equal(frame[5:40, 9:100], got[5:40, 9:100])


def test_refusals_leave_the_context_usable(ctx):
    from swiftwatcher_amd import _lib
    y, u, v = _planes(11, 2, 10, 12)
    for rect in [(-1, 0, 4, 4), (0, -1, 4, 4), (0, 0, 13, 10), (0, 0, 12, 11), (11, 9, 2, 1), (11, 9, 1, 2), (0, 0, 0, 4), (0, 0, 4, 0)]:
        with pytest.raises(_lib.SwkError) as err:
            ctx.yuv420_to_bgr(y, u, v, rect=rect)
        assert "rectangle" in str(err.value), rect
    out = np.empty((2, 10, 12, 3), np.uint8)

    def raw(count=2, **over):
        f = dict(y=y.ctypes.data, u=u.ctypes.data, v=v.ctypes.data, mem=_lib.MEM_HOST, layout=_lib.YUV_I420, H=10, W=12,
                 y_row_stride=12, y_frame_stride=120, c_row_stride=6, c_frame_stride=30)
        f.update(over)
        src = _lib.Yuv420(**f)
        rc = ctx._lib.swk_yuv420_to_bgr(ctx._h, ctypes.byref(src), count, 0, 0, 10, 12, out.ctypes.data, _lib.MEM_HOST)
        return rc, ctx._lib.swk_last_error(ctx._h).decode()
    assert raw()[0] == 0 and np.array_equal(out, yuv_ref.bgr(y, u, v))
    for over, word in [(dict(y=None), "plane"), (dict(u=None), "plane"), (dict(v=None), "plane"), (dict(layout=2), "layout"),
                       (dict(layout=-1), "layout"), (dict(y_row_stride=11), "stride"), (dict(c_row_stride=5), "stride")]:
        rc, msg = raw(**over)
        assert rc == -1 and word in msg, (over, msg)
    for count in (0, -3):
        rc, msg = raw(count=count)
        assert rc == -1 and "count" in msg
    rc, msg = raw(layout=_lib.YUV_NV12, v=None, c_row_stride=11)          # an NV12 row needs 2 * ceil(W / 2) bytes
    assert rc == -1 and "stride" in msg
    with pytest.raises(ValueError):
        ctx.yuv420_to_bgr(y, u[:, :4], v[:, :4])
    with pytest.raises(ValueError):
        ctx.yuv420_to_bgr(y, u)                                            # no v: NV12 is asked for, the plane is not interleaved
    # the context still works
    assert np.array_equal(ctx.yuv420_to_bgr(y, u, v, rect=(1, 1, 9, 7)), yuv_ref.bgr(y, u, v, (1, 1, 9, 7)))
    res = ctx.batch_run(np.ascontiguousarray(yuv_ref.bgr(y, u, v)[:, :8, :8]), 1, 2, stages=("gray",))
    assert res["gray"].shape == (2, 8, 8)


# ---------------------------------------------------------------------------------------------------- the batch path
@pytest.fixture(scope="module")
def clip(tmp_path_factory):
    """A seeded 52-frame 110 x 160 clip as 4:2:0 planes, its .y4m file, and the BGR frames those planes restate to."""
    from swiftwatcher_amd import synthetic
    from swiftwatcher_amd.io_y4m import Y4MWriter
    bgr = synthetic.full_frames(500, 52, CROP, frame_hw=(110, 160), birds=4, bird_len=(8, 12), bird_wid=(3, 5))[::-1].copy()
    y, u, v = yuv_ref.bgr_to_yuv420(bgr)
    path = str(tmp_path_factory.mktemp("y4m") / "clip.y4m")
    with Y4MWriter(path, 160, 110, 30) as w:
        for k in range(len(y)):
            w.append(y[k], u[k], v[k])
    return dict(path=path, y=y, u=u, v=v, bgr=yuv_ref.bgr(y, u, v))


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
        for fa, fb in zip(wa["frames"], wb["frames"]):
            assert fa["number"] == fb["number"] and fa["segs"] == fb["segs"], fa["number"]
            assert fa.get("kept") == fb.get("kept")
            assert np.array_equal(fa["crop"], fb["crop"])
            for name in fa["stages"]:
                assert np.array_equal(fa["stages"][name], fb["stages"][name]), (fa["number"], name)
            assert len(fa["images"]) == len(fb["images"]) and all(np.array_equal(x, z) for x, z in zip(fa["images"], fb["images"]))


@pytest.mark.parametrize("n,windows", [(21, 3), (5, 4)])
@pytest.mark.parametrize("crop", [CROP, CROP_ODD], ids=["even", "odd"])
def test_frame_queue_over_a_y4m_reader(clip, n, windows, crop):
    from swiftwatcher_amd.io_frames import ArrayReader
    from swiftwatcher_amd.io_y4m import Y4MReader
    want = _queue_run(ArrayReader(list(clip["bgr"]), fps=30.0), n, crop, windows)
    assert any(f["segs"] for w in want for f in w["frames"]), "no frame of the BGR run has a region"
    got = _queue_run(Y4MReader(clip["path"]), n, crop, windows)
    _same_windows(got, want)


def _triples(reader, n, windows):
    return [reader.get_n_frames(n) for _ in range(windows)]


def _popped_records(popped_lists):
    return [[(f.frame_number, _seg_records(f), [np.array(s.segment_image).tobytes() for s in f.segments]) for f in popped] for popped in popped_lists]


def test_groups_call_mixing_a_yuv_and_a_bgr_video(clip):
    from swiftwatcher_amd import synthetic
    from swiftwatcher_amd.data_structures import segment_window_groups, segment_windows
    from swiftwatcher_amd.io_frames import ArrayReader
    from swiftwatcher_amd.io_y4m import Y4MReader
    crop2 = [(21, 11), (21 + 80, 11 + 48)]
    other = synthetic.full_frames(77, 42, crop2, frame_hw=(90, 140), birds=3, bird_len=(8, 12), bird_wid=(3, 5))[::-1].copy()
    n = 21
    lone_yuv = _popped_records(segment_windows(_triples(Y4MReader(clip["path"]), n, 2), CROP))
    lone_restated = _popped_records(segment_windows(_triples(ArrayReader(list(clip["bgr"]), fps=30.0), n, 2), CROP))
    lone_bgr = _popped_records(segment_windows(_triples(ArrayReader(list(other), fps=30.0), n, 2), crop2))
    assert lone_yuv == lone_restated
    for order in (0, 1):
        groups = [(_triples(Y4MReader(clip["path"]), n, 2), CROP), (_triples(ArrayReader(list(other), fps=30.0), n, 2), crop2)]
        out = segment_window_groups(groups[::-1] if order else groups)
        got = [_popped_records(g) for g in (out[::-1] if order else out)]
        assert got[0] == lone_yuv and got[1] == lone_bgr
    assert any(segs for popped in lone_yuv for _, segs, _ in popped) and any(segs for popped in lone_bgr for _, segs, _ in popped)


def _event_records(events):
    return [[(s.parent_frame_number, str(s.parent_timestamp), tuple(s.centroid), tuple(s.bbox), np.array(s.segment_image).tobytes()) for s in ev]
            for ev in events]


def test_count_swifts_over_a_y4m_file(clip):
    """52 frames = two windows and a padded one, one and two windows per call; the reader, its path and the restated BGR list."""
    from swiftwatcher_amd import pipeline
    from swiftwatcher_amd.io_y4m import Y4MReader
    roi_mask = np.zeros((64, 96), np.uint8)
    roi_mask[28:, :] = 255
    seen = []
    for wpc in (1, 2):
        want = pipeline.count_swifts(list(clip["bgr"]), CROP, roi_mask, fps=30.0, windows_per_call=wpc)
        for source in (Y4MReader(clip["path"]), clip["path"]):
            got = pipeline.count_swifts(source, CROP, roi_mask, windows_per_call=wpc)
            assert got[0] == want[0] and _event_records(got[1]) == _event_records(want[1])
        seen.append((want[0], _event_records(want[1])))
    assert seen[0] == seen[1]
    print("count %d, %d events" % (seen[0][0], len(seen[0][1])))


def test_presegmenting_reader_over_a_y4m_reader(clip):
    from swiftwatcher_amd.io_frames import ArrayReader, PresegmentingReader
    from swiftwatcher_amd.io_y4m import Y4MReader
    runs = []
    for inner in (Y4MReader(clip["path"]), ArrayReader(list(clip["bgr"]), fps=30.0)):
        reader = PresegmentingReader(inner, crop_region=CROP, queue_size=21, windows=2)
        runs.append(_queue_run(reader, 21, CROP, 3))
        reader.close()
    _same_windows(runs[0], runs[1])


def test_classifier_scores_and_decisions_equal(clip):
    """The window's segments scored through the device hand-over (swk_segment_inputs_last on the converted frames the batch holds) and
    through the segments' images: the same table, scores and keep decisions from the .y4m file as from the restated BGR frames."""
    import torch
    from oracle import classifier_ref as ref
    from swiftwatcher_amd.io_frames import ArrayReader
    from swiftwatcher_amd.io_y4m import Y4MReader
    from swiftwatcher_amd.segment_classification import SegmentClassifier
    plain = _queue_run(ArrayReader(list(clip["bgr"]), fps=30.0), 21, CROP, 3)
    crops = [im for w in plain for f in w["frames"] for im in f["images"]]
    assert len(crops) > 20
    sd = ref.calibrate_head(ref.random_state_dict(5), crops[::3])
    clf = SegmentClassifier.from_state_dict(sd)
    assert clf.device.type == "cuda"
    want = _queue_run(ArrayReader(list(clip["bgr"]), fps=30.0), 21, CROP, 3, classifier=clf)
    got = _queue_run(Y4MReader(clip["path"]), 21, CROP, 3, classifier=clf)
    assert all(w["table"] is not None for w in got if any(f["segs"] for f in w["frames"])), "the device hand-over did not serve the YUV windows"
    _same_windows(got, want)
    mine = [im for w in got for f in w["frames"] for im in f["images"]]
    assert torch.equal(clf.scores(mine), clf.scores(crops))
