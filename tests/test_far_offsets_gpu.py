"""The entry points that read device memory at the caller's strides, on frames that start beyond 2 GiB and 4 GiB of their buffer.

One device buffer per test of 4 * fs + (bytes of one frame), fs = 2^30 + 4099 (odd frame starts) or 2^30 + 4096 (16-byte aligned),
made with torch.empty and never initialised as a whole; five frames are written at f * fs, so frame 2 starts above 2^31 and frame 4
above 2^32.  Each call's result must equal, bit for bit, the same call on the same five frames packed densely -- which the other
tests of each entry point hold to its CPU restatement.  A 32-bit product of frame index and stride anywhere on the way shows as a
difference on frames 2..4 (or as a refusal).

Out of scope: dense OUTPUTS above 2 GiB, which would need multi-gigabyte host arrays to check."""
import numpy as np
import pytest

import torch

import frame_chunks as fc

pytestmark = pytest.mark.gpu

STRIDES = [(1 << 30) + 4099, (1 << 30) + 4096]
IDS = ["odd_starts", "aligned_starts"]
NEED = 6 << 30


@pytest.fixture(scope="module")
def ctx():
    from swiftwatcher_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


class Far:
    """five frames at f * fs in one uninitialised device buffer; view(...) places arrays in it"""

    def __init__(self, fs, frame_bytes):
        free, _total = torch.cuda.mem_get_info()
        if free < NEED:
            pytest.skip("the device has less than 6 GiB free (%.1f GiB)" % (free / 2.0 ** 30))
        self.fs = fs
        self.buf = torch.empty(4 * fs + frame_bytes, dtype=torch.uint8, device="cuda:0")

    def place(self, arr, offset=0, row_stride=None):
        """the (5, rows, ...) host array written at offset + f * fs (rows row_stride bytes apart) -> the strided device view of it"""
        a = np.ascontiguousarray(arr)
        b = a.view(np.uint8).reshape(a.shape[0], a.shape[1], -1)
        rs = row_stride or b.shape[2]
        view = torch.as_strided(self.buf, b.shape, (self.fs, rs, 1), storage_offset=offset)
        view.copy_(torch.from_numpy(b))
        assert view.data_ptr() + 4 * self.fs - self.buf.data_ptr() >= 1 << 32
        return view

    def free(self):
        self.buf = None
        torch.cuda.empty_cache()


def _shaped(view, shape):
    """place()'s (5, rows, bytes) uint8 view as (5, rows, ...) of that shape, rows at the view's stride"""
    st = view.stride()
    tail = tuple(shape[2:])
    inner = [int(np.prod(tail[i + 1:])) for i in range(len(tail))]
    return torch.as_strided(view, tuple(shape), (st[0], st[1]) + tuple(inner), storage_offset=view.storage_offset())


def _same(a, b, what):
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    b = b.cpu().numpy() if hasattr(b, "cpu") else np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), what


@pytest.mark.parametrize("fs", STRIDES, ids=IDS)
@pytest.mark.parametrize("wide_rows", [False, True], ids=["rows_dense", "rows_wide"])
def test_batch_run(ctx, fs, wide_rows):
    """one window of n = 5 with a crop, at a row stride of the frame width and a wider one"""
    from helpers import STAGES, scene
    roi = scene("bgr33x75n5")                                        # (5, 33, 75, 3)
    Hf, Wf, x0, y0 = 40, 84, 5, 4
    frames = np.random.default_rng(3).integers(0, 256, size=(5, Hf, Wf, 3), dtype=np.uint8)
    frames[:, y0:y0 + 33, x0:x0 + 75] = roi
    rs = Wf * 3 + (7 if wide_rows else 0)
    far = Far(fs, Hf * rs)
    try:
        view = _shaped(far.place(frames, row_stride=rs), frames.shape)
        got = ctx.batch_run(view, 1, 5, crop=(x0, y0, 75, 33))
        want = ctx.batch_run(torch.from_numpy(frames).cuda(), 1, 5, crop=(x0, y0, 75, 33))
        assert want["opened"].any() and want["nseg"].max() >= 1
        for key in STAGES + ("iters", "nseg", "segs"):
            _same(got[key], want[key], key)
    finally:
        far.free()


@pytest.mark.parametrize("fs", STRIDES, ids=IDS)
def test_segment_shapes_u8(ctx, fs):
    labels = fc.label_planes(9, 13)[[3, 9, 17, 25, 36]]
    far = Far(fs, labels[0].size)
    try:
        view = far.place(labels)
        got = ctx.segment_shapes_u8(view)
        want = ctx.segment_shapes_u8(labels)
        _same(got[0], want[0], "shapes")
        _same(got[1], want[1], "nseg")
        assert want[1].tolist() == [4, 10, 18, 26, 37]
    finally:
        far.free()


@pytest.mark.parametrize("fs", STRIDES, ids=IDS)
@pytest.mark.parametrize("subpel", [False, True], ids=["integer", "subpel"])
def test_stabilize(ctx, fs, subpel):
    frames, rect, anchor, _moved = fc.stabilize_case(seed=2)
    frames = frames[[0, 7, 13, 21, 30]]
    far = Far(fs, frames[0].size)
    try:
        view = _shaped(far.place(frames), frames.shape)
        fn = ctx.stabilize_subpel if subpel else ctx.stabilize
        got = fn(view, rect, fc.STAB_S, anchor, table=True)
        want = fn(frames, rect, fc.STAB_S, anchor, table=True)
        _same(got[0], want[0], "records")
        for g, w in zip(got[1] if subpel else (got[1],), want[1] if subpel else (want[1],)):
            _same(g, w, "table")
        _same(got[2], want[2], "pixels")
        assert len({(int(s["dy"]), int(s["dx"])) for s in want[0]}) == 5
    finally:
        far.free()


@pytest.mark.parametrize("fs", STRIDES, ids=IDS)
@pytest.mark.parametrize("layout", ["i420", "nv12"])
def test_yuv420_to_bgr(ctx, fs, layout):
    """luma and chroma strides both far: y at f * fs, u (or the interleaved plane) 2^29 further, v behind u"""
    H, W, rect = 10, 14, (3, 1, 11, 9)
    y, u, v = (p[:5] for p in fc.yuv420_planes(H, W))
    far = Far(fs, (1 << 29) + 4096)
    try:
        dy = far.place(y)
        if layout == "i420":
            du, dv = far.place(u, offset=1 << 29), far.place(v, offset=(1 << 29) + 1024)
            got = ctx.yuv420_to_bgr(dy, du, dv, rect=rect, device_out=True)
            want = ctx.yuv420_to_bgr(y, u, v, rect=rect)
        else:
            uv = np.ascontiguousarray(np.stack([u, v], axis=-1)).reshape(5, u.shape[1], -1)
            got = ctx.yuv420_to_bgr(dy, far.place(uv, offset=1 << 29), rect=rect, device_out=True)
            want = ctx.yuv420_to_bgr(y, uv, rect=rect)
        _same(got, want, layout)
    finally:
        far.free()


@pytest.mark.parametrize("fs", STRIDES, ids=IDS)
def test_yuv_to_bgr(ctx, fs):
    """8-bit 4:2:2 planar, and 10-bit 4:2:0 semiplanar in 16-bit words (the aligned stride only: words lie at even addresses)"""
    H, W, rect = 10, 14, (3, 1, 11, 9)
    rng = np.random.default_rng(8)
    far = Far(fs, (1 << 29) + 4096)
    try:
        y = rng.integers(0, 256, size=(5, H, W), dtype=np.uint8)
        u, v = (rng.integers(0, 256, size=(5, H, 7), dtype=np.uint8) for _ in range(2))
        got = ctx.yuv_to_bgr(far.place(y), far.place(u, offset=1 << 29), far.place(v, offset=(1 << 29) + 1024), subsampling=(1, 0), rect=rect,
                             device_out=True)
        _same(got, ctx.yuv_to_bgr(y, u, v, subsampling=(1, 0), rect=rect), "4:2:2")
        if fs % 2 == 0:
            from swiftwatcher_amd import _lib
            y16 = (rng.integers(0, 1024, size=(5, H, W)) << 6).astype(np.uint16)
            uv16 = (rng.integers(0, 1024, size=(5, 5, 14)) << 6).astype(np.uint16)
            dy, duv = far.place(y16), far.place(uv16, offset=1 << 29)
            src = _lib.Yuv(y=dy.data_ptr(), u=duv.data_ptr(), v=None, mem=_lib.MEM_DEVICE, layout=_lib.YUV_SEMIPLANAR, H=H, W=W,
                           y_row_stride=W * 2, y_frame_stride=fs, c_row_stride=28, c_frame_stride=fs, sx=1, sy=1, bits=10, msb_aligned=1,
                           full_range=0)
            out = torch.empty((5, rect[3], rect[2], 3), dtype=torch.uint8, device="cuda:0")
            import ctypes
            ctx._check(ctx._lib.swk_yuv_to_bgr(ctx._h, ctypes.byref(src), 5, rect[0], rect[1], rect[3], rect[2], ctypes.c_void_p(out.data_ptr()),
                                               _lib.MEM_DEVICE))
            _same(out, ctx.yuv_to_bgr(y16, uv16, subsampling=(1, 1), bits=10, msb_aligned=True, rect=rect), "P010")
    finally:
        far.free()


@pytest.mark.parametrize("fs", STRIDES, ids=IDS)
def test_render_review(ctx, fs):
    frames = fc.bgr_frames(11, 16, seed=3)[:5]
    rect = (2, 1, 13, 9)
    styles = [(0, 255, 0, 48, 256), (0, 0, 255, 128, 255)]
    kw = dict(boxes=[(f, f % 3, 1 + f, 6, 9 + f % 2, 1 + f % 2) for f in range(5)], marks=[(2, 4, 4, 2), (4, 5, 6, 1)], styles=styles, mark_arm=2,
              border=1, frame_style=np.array([0, 1, 2, 0, 1], np.int32), rect=rect)
    far = Far(fs, frames[0].size)
    try:
        view = _shaped(far.place(frames), frames.shape)
        got = ctx.render_review(view, labels=[(2, 1, 1, 1, 2, 1, "F2"), (4, 1, 1, 1, 2, 1, "F4")], **kw)
        want = ctx.render_review(frames, labels=[(2, 1, 1, 1, 2, 1, "F2"), (4, 1, 1, 1, 2, 1, "F4")], **kw)
        plain = ctx.bgr_to_yuv420(frames, rect=rect)
        for g, w, p in zip(got, want, plain):
            _same(g, w, "review")
        assert all(not np.array_equal(want[0][f], plain[0][f]) for f in (2, 4)), "the overlay shows on the far frames"
        for g, w in zip(ctx.bgr_to_yuv420(view, rect=rect), plain):
            _same(g, w, "conversion")
    finally:
        far.free()


@pytest.mark.parametrize("fs", STRIDES, ids=IDS)
def test_segment_inputs(ctx, fs):
    """boxes in frames 2 and 4 (and one in frame 0)"""
    from swiftwatcher_amd import _lib
    from swiftwatcher_amd.segment_classification import IMAGENET_MEAN, IMAGENET_STD
    fh, fw, cap, pad = 40, 56, 2, 8
    frames = np.random.default_rng(12).integers(0, 256, size=(5, fh, fw, 3), dtype=np.uint8)
    records = np.zeros((5, cap), _lib.SEGMENT_DTYPE)
    counts = np.array([1, 0, 2, 0, 1], np.int32)
    records[0, 0] = (1, 2, 3, 20, 30, 0, 18 * 27, 0, 0)
    records[2, 0] = (1, 5, 6, 12, 14, 0, 7 * 8, 0, 0)          # below 24 x 24: grown
    records[2, 1] = (2, 8, 20, 38, 55, 0, 30 * 35, 0, 0)
    records[4, 0] = (1, 10, 1, 37, 50, 0, 27 * 49, 0, 0)
    segs = torch.from_numpy(records.view(np.uint8).reshape(5, cap, 48)).cuda()
    nseg = torch.from_numpy(counts).cuda()
    side = 24 + 2 * pad

    def cut(ptr, frame_stride):
        x = torch.full((4, 3, side, side), -7.25, dtype=torch.float32, device="cuda:0")
        fidx = torch.full((4,), -99, dtype=torch.int32, device="cuda:0")
        inp = _lib.Input(frames=ptr, mem=_lib.MEM_DEVICE, channels=3, nwin=1, n=5, Hc=fh, Wc=fw, x0=0, y0=0, frame_stride=frame_stride,
                         row_stride=fw * 3)
        total, skipped = ctx.segment_inputs(inp, (fh, fw), segs.data_ptr(), nseg.data_ptr(), cap, IMAGENET_MEAN, IMAGENET_STD, x.data_ptr(), 4,
                                            pad=pad, seg_frame_ptr=fidx.data_ptr())
        return total, skipped, x.cpu().numpy(), fidx.cpu().numpy()
    far = Far(fs, frames[0].size)
    try:
        view = far.place(frames)
        dense = torch.from_numpy(frames).cuda()
        got = cut(view.data_ptr(), fs)
        want = cut(dense.data_ptr(), frames[0].size)
        assert want[0] == 4 and want[1] == 0 and want[3].tolist() == [0, 2, 2, 4]
        assert len({want[2][i].tobytes() for i in range(4)}) == 4
        assert got[0] == want[0] and got[1] == want[1]
        _same(got[2], want[2], "network inputs")
        _same(got[3], want[3], "frame of each input")
    finally:
        far.free()
