"""The CPU side of the end-to-end parity tests lives in oracle/pipeline_ref.py (bench.py's parity leg uses it too)."""
from oracle.pipeline_ref import oracle_frames, track, oracle_events, event_signature, classify_keep          # noqa: F401
import numpy as np

# ---- swk_batch_run_groups: every group against its lone swk_batch_run and the CPU oracle (tests/test_video_groups*_gpu.py) ----
ATOL_AE = 1e-5
STAGES = ("gray", "rpca", "bilateral", "thresh", "opened", "labels")


def gray_u8(bgr):
    b, g, r = (bgr[..., k].astype(np.int32) for k in range(3))
    return ((b * 1868 + g * 9617 + r * 4899 + (1 << 13)) >> 14).astype(np.uint8)


def roi_stack(seed, nwin, Hc, Wc, n=21, null_tail=()):
    """(nwin * n, Hc, Wc, 3) ROI frames, queue order per window; null_tail[w] = how many of window w's newest frames are null"""
    from swiftwatcher_amd import synthetic
    out = []
    for w in range(nwin):
        if Hc * Wc < 64:
            roi = np.random.default_rng(seed + w).integers(0, 256, size=(n, Hc, Wc, 3), dtype=np.uint8)
        else:
            roi = synthetic.roi_window(seed + w, n, Hc, Wc, birds=3, bird_len=(6, 10), bird_wid=(3, 5))
        k = null_tail[w] if w < len(null_tail) else 0
        roi[:k] = 0
        out.append(roi)
    return np.ascontiguousarray(np.concatenate(out))


def lone_run(ctx, spec, **kw):
    """swk_batch_run on one group spec of batch_run_groups"""
    frames = spec["frames"]
    if hasattr(frames, "cpu"):
        frames = frames.cpu().numpy()
    return ctx.batch_run(frames, spec["nwin"], spec["n"], crop=spec.get("crop"), reverse_frames=spec.get("reverse_frames", False),
                         seg_cap=spec.get("seg_cap", 255), **kw)


def seg_tuples(res, f):
    return [(int(s["label"]), int(s["r0"]), int(s["c0"]), int(s["r1"]), int(s["c1"]), int(s["area"]), int(s["sum_r"]), int(s["sum_c"]))
            for s in res["segs"][f, :res["nseg"][f]]]


def orc_seg_tuples(seglist):
    return [(s["label"],) + s["bbox"] + (s["area"], s["sum_r"], s["sum_c"]) for s in seglist]


def check_against_lone(g, res, lone, ae, exact_ae=False):
    """one group of a groups call against the same group run alone: u8 stages, iterations and region records bit for bit; A / E to
    float64 summation order (exact_ae: bit for bit)"""
    for key in STAGES:
        if key in res:
            assert np.array_equal(res[key], lone[key]), "group %d: stage %s differs from a lone run" % (g, key)
    assert np.array_equal(res["iters"], lone["iters"]), g
    assert np.array_equal(res["nseg"], lone["nseg"]), g
    assert np.array_equal(res["segs"], lone["segs"]), g
    if ae and exact_ae:
        assert np.array_equal(res["A"], lone["A"]) and np.array_equal(res["E"], lone["E"]), g
    elif ae:
        assert np.abs(res["A"] - lone["A"]).max() <= ATOL_AE, g
        assert np.abs(res["E"] - lone["E"]).max() <= ATOL_AE, g


def check_against_oracle(orc, g, spec, roi, res):
    """every window of one group against the CPU oracle run on its ROI frames (roi: the group's frames in queue order)"""
    n = spec["n"]
    for w in range(spec["nwin"]):
        ref = orc.window(np.ascontiguousarray(roi[w * n:(w + 1) * n]))
        for key in ("gray", "rpca", "opened", "labels"):
            assert np.array_equal(res[key][w * n:(w + 1) * n], ref[key]), "group %d window %d: %s vs oracle" % (g, w, key)
        for i in range(n):
            assert seg_tuples(res, w * n + i) == orc_seg_tuples(ref["segments"][i]), "group %d window %d frame %d" % (g, w, i)


def check_against_lone_and_oracle(ctx, orc, specs, rois, ae):
    kw = dict(want_A=True, want_E=True) if ae else {}
    got = ctx.batch_run_groups(specs, **kw)
    assert len(got) == len(specs)
    for g, (spec, roi, res) in enumerate(zip(specs, rois, got)):
        # one group: the lone run's kernels, so the same summation order
        check_against_lone(g, res, lone_run(ctx, spec, **kw), ae, exact_ae=len(specs) == 1)
        check_against_oracle(orc, g, spec, roi, res)
    return got


# ---- frame ingest and output placement of the batch calls (tests/test_ingest_*.py, tests/test_output_placement_gpu.py) ----
# One SCENE is a set of ROI frames; a VIEW embeds it in a larger buffer (margins, row padding, frame padding, frame order, base offset).
# Every view of a scene must give the results of the dense scene: only where the library reads from differs.
ROUTE_DENSE, ROUTE_WHOLE, ROUTE_ROWS, ROUTE_2D, ROUTE_DEVICE = 0, 1, 2, 3, -1
ROUTE_NAMES = {ROUTE_DENSE: "dense", ROUTE_WHOLE: "whole", ROUTE_ROWS: "rows", ROUTE_2D: "2d", ROUTE_DEVICE: "device"}
ANCHOR_ELEMS = 1.4e5          # below this the CPU oracle itself is LAPACK-dependent (tests/fuzz_parity.py)

# name: (seed, nwin, n, Hc, Wc, channels); Wc mod 4 = 0, 1, 2, 3 for the BGR scenes
SCENES = {
    "bgr60x120n21": (7100, 1, 21, 60, 120, 3),
    "bgr67x101n21": (7200, 1, 21, 67, 101, 3),
    "bgr47x94n21": (7300, 1, 21, 47, 94, 3),
    "bgr47x94n5": (7402, 1, 5, 47, 94, 3),
    "bgr33x75n21": (7500, 1, 21, 33, 75, 3),
    "bgr33x75n5": (7600, 1, 5, 33, 75, 3),
    "gray60x120n21": (7100, 1, 21, 60, 120, 1),
    "bgr36x52n21w2": (7700, 2, 21, 36, 52, 3),
}
# five frames leave little in the sparse term (every singular value of five is kept): birds chosen so that regions survive the threshold
SCENE_BIRDS = {"bgr47x94n5": dict(birds=8, bird_len=(10, 16), bird_wid=(5, 8), contrast=(120, 160)),
               "bgr33x75n5": dict(birds=1, bird_len=(3, 5), bird_wid=(5, 8), contrast=(200, 250), noise=0.5)}
ANCHORED = tuple(k for k, (_, nwin, n, H, W, _c) in SCENES.items() if nwin == 1 and _c == 3 and n * H * W >= ANCHOR_ELEMS)
_scene_cache = {}


def scene(name):
    """(nwin * n, Hc, Wc[, 3]) u8 frames of a scene, queue order per window; the single-channel scene is the gray of its BGR twin"""
    if name not in _scene_cache:
        seed, nwin, n, H, W, ch = SCENES[name]
        if name in SCENE_BIRDS:
            from swiftwatcher_amd import synthetic
            s = np.ascontiguousarray(synthetic.roi_window(seed, n, H, W, **SCENE_BIRDS[name]))
        else:
            s = roi_stack(seed, nwin, H, W, n=n)
        _scene_cache[name] = np.ascontiguousarray(gray_u8(s)) if ch == 1 else s
        _scene_cache[name].setflags(write=False)
    return _scene_cache[name]


def scene_gray(name, gray_mode=0):
    """the numpy statement of BGR2GRAY on a scene (Q14: gray_u8; Q15: the oracle's integer statement); one channel passes through"""
    s = scene(name)
    if s.ndim == 3:
        return s
    if gray_mode == 0:
        return gray_u8(s)
    from oracle import reference_path as orc
    return np.stack([orc.bgr2gray(np.ascontiguousarray(f), 1) for f in s])


def gray_kernel(name):
    """which gray kernel one lone call on this scene launches (filters.hip, launch_gray; the X plane it writes is dword aligned)"""
    _, _, _, _, W, ch = SCENES[name]
    return "k_gray" if ch == 1 else ("k_gray4" if W % 4 == 0 else "k_gray4g")


class View:
    """A scene embedded in a byte buffer.  Frame j of the batch lies at memory frame j (reverse: F - 1 - j); a memory frame has
    Hf = y0 + Hc + below rows of rs = (x0 + Wc + right) * channels + row_pad bytes, and fs = Hf * rs + frame_pad bytes; memory frame 0
    starts base bytes into the buffer.  Every byte that is not a ROI byte is seeded noise."""

    def __init__(self, scene_name, route, label, x0=0, y0=0, right=0, below=0, row_pad=0, frame_pad=0, reverse=False, base=0,
                 device=False, gray_mode=0):
        self.scene, self.route, self.label = scene_name, route, label
        _, self.nwin, self.n, self.Hc, self.Wc, self.ch = SCENES[scene_name]
        self.F = self.nwin * self.n
        self.x0, self.y0, self.reverse, self.base, self.device, self.gray_mode = x0, y0, reverse, base, device, gray_mode
        self.Wf, self.Hf = x0 + self.Wc + right, y0 + self.Hc + below
        self.rs = self.Wf * self.ch + row_pad
        self.fs = self.Hf * self.rs + frame_pad
        self.nbytes = base + self.F * self.fs + 8
        self.id = "%s-%s-%s%s" % (scene_name, ROUTE_NAMES[route], label, "-dev" if device else "")

    # geometry the calls take
    @property
    def crop(self):
        return (self.x0, self.y0, self.Wc, self.Hc)

    @property
    def shape(self):
        return (self.F, self.Hf, self.Wf) + ((3,) if self.ch == 3 else ())

    @property
    def strides(self):
        return (self.fs, self.rs, self.ch) + ((1,) if self.ch == 3 else ())

    @property
    def roi_bytes(self):
        return self.F * self.Hc * self.Wc * self.ch

    def rule_route(self):
        """host_stage_plan (swk_api.hip) restated: the route a host view takes"""
        fs = -self.fs if self.reverse else self.fs
        rowb = self.Wc * self.ch
        if self.x0 == 0 and self.rs == rowb and fs == self.Hc * self.rs:
            return ROUTE_DENSE
        if (self.rs >= (self.x0 + self.Wc) * self.ch and self.rs % self.ch == 0 and self.fs % self.rs == 0 and
                self.fs >= (self.y0 + self.Hc) * self.rs and self.F * self.fs <= 2 * self.roi_bytes):
            return ROUTE_WHOLE
        if self.x0 == 0 and self.rs == rowb:
            return ROUTE_ROWS
        return ROUTE_2D

    def kernel_geometry(self, base_residue=0):
        """(address of frame 0 mod 4 taken as an offset, frame stride, row stride, x0, y0) as the gray kernel sees them: the caller's for a
        device view and the whole-buffer route, the packed copy's for the other routes (staging buffers are 256-byte aligned)"""
        if self.device or self.route == ROUTE_WHOLE:
            first = (self.F - 1) * self.fs if self.reverse else 0
            return ((base_residue + self.base) if self.device else 0) + first, -self.fs if self.reverse else self.fs, self.rs, self.x0, self.y0
        return 0, self.Hc * self.Wc * self.ch, self.Wc * self.ch, 0, 0

    def first_roi_residue(self, base_residue=0):
        """address mod 4 of the first ROI byte of frame 0 at the kernel"""
        a, _fs, rs, x0, y0 = self.kernel_geometry(base_residue)
        return (a + y0 * rs + x0 * self.ch) % 4

    def row_residues(self, base_residue=0):
        """the set of address residues mod 4 of the ROI's row starts at the kernel, over all frames and rows"""
        a, fs, rs, x0, y0 = self.kernel_geometry(base_residue)
        return {(a + f * fs + (y0 + r) * rs + x0 * self.ch) % 4 for f in range(self.F) for r in range(self.Hc)}

    def _embed(self, buf, frames):
        arr = np.lib.stride_tricks.as_strided(buf[self.base:], shape=self.shape, strides=self.strides, writeable=True)
        arr[:, self.y0:self.y0 + self.Hc, self.x0:self.x0 + self.Wc] = frames[::-1] if self.reverse else frames
        return arr

    def buffer(self):
        """the byte buffer: noise everywhere, the scene at its place"""
        import zlib
        buf = np.random.default_rng(zlib.crc32(self.id.encode())).integers(0, 256, size=self.nbytes, dtype=np.uint8)
        self._embed(buf, scene(self.scene))
        return buf

    def roi_mask(self):
        """True at the buffer's ROI bytes"""
        mask = np.zeros(self.nbytes, np.uint8)
        self._embed(mask, np.ones_like(scene(self.scene)))
        return mask.astype(bool)

    def host_array(self, buf):
        return np.lib.stride_tricks.as_strided(buf[self.base:], shape=self.shape, strides=self.strides, writeable=False)

    def device_array(self, buf):
        """(torch view read in place, the allocation it lives in)"""
        import torch
        t = torch.from_numpy(buf).cuda()
        return torch.as_strided(t, self.shape, self.strides, storage_offset=self.base), t

    def group_spec(self, keep):
        """batch_run_groups' spec of this view; keep: a list that holds the buffers alive"""
        buf = self.buffer()
        if self.device:
            arr, t = self.device_array(buf)
            keep.append(t)
        else:
            arr = self.host_array(buf)
        keep.append(buf)
        return dict(frames=arr, nwin=self.nwin, n=self.n, crop=self.crop, reverse_frames=self.reverse)


def _route_rows(name):
    """the staging table of one scene: (route, label, geometry)"""
    _, _, _, H, W, ch = SCENES[name]
    rows = [
        (ROUTE_DENSE, "scene", {}),
        (ROUTE_WHOLE, "margin_all_sides", dict(x0=5, y0=4, right=5, below=4)),
        (ROUTE_WHOLE, "margin_right_below", dict(right=5, below=4)),
        (ROUTE_WHOLE, "rows_padded", dict(row_pad=3 * ch)),
        (ROUTE_WHOLE, "frames_padded_rows", dict(below=3)),
        (ROUTE_WHOLE, "reversed", dict(x0=5, y0=4, right=5, below=4, reverse=True)),
        (ROUTE_WHOLE, "factor2_exact", dict(x0=13, right=W - 13)),                      # Hf * rs = Hc * 2 Wc ch
        (ROUTE_2D, "factor2_one_more_row", dict(x0=13, right=W - 13, below=1)),
        (ROUTE_WHOLE, "factor2_exact_full_rows", dict(y0=7, below=H - 7)),              # 2 Hc rows of Wc ch bytes
        (ROUTE_ROWS, "factor2_one_more_full_row", dict(y0=7, below=H - 6)),
        (ROUTE_2D, "small_roi_large_frame", dict(x0=40, y0=30, right=100, below=80)),
        (ROUTE_2D, "frame_stride_off_rows", dict(x0=2, y0=1, right=3, below=1, frame_pad=7)),
        (ROUTE_2D, "reversed", dict(x0=40, y0=30, right=100, below=80, reverse=True)),
        (ROUTE_ROWS, "tall_frames", dict(y0=H, below=H + 2)),
        (ROUTE_ROWS, "tall_frames_reversed", dict(y0=H, below=H + 2, reverse=True)),
    ]
    if ch == 3:
        rows += [(ROUTE_2D, "row_stride_off_pixels_1", dict(x0=2, y0=1, right=3, below=1, row_pad=1)),
                 (ROUTE_2D, "row_stride_off_pixels_2", dict(x0=2, y0=1, right=3, below=1, row_pad=2))]
    return rows


def route_views():
    """every scene through every staging route"""
    return [View(name, route, label, **geo) for name in SCENES for route, label, geo in _route_rows(name)]


ALIGN_SCENES = ("bgr60x120n21", "bgr33x75n5", "gray60x120n21")          # k_gray4, k_gray4g, k_gray
ALIGN_X0 = (0, 1, 2, 3, 13)


def alignment_views():
    """Every residue of the first ROI byte mod 4 with a row stride of every residue mod 4, for each gray kernel: host views on the
    whole-buffer route (the only host route on which the kernels see the caller's geometry; its row stride is a multiple of the
    channel count, so the residue comes from the frame width), device views read in place (row padding and a base 0..3 bytes into the
    allocation), and dense device views at a base of 1, 2 and 3.  Q15 gray on the x0 = 13 views."""
    views = []
    for name in ALIGN_SCENES:
        _, _, _, H, W, ch = SCENES[name]
        i = 0
        for x0 in ALIGN_X0:
            for res in range(4):
                mode = 1 if x0 == 13 else 0
                right = next(r for r in range(1, 9) if ((x0 + W + r) * ch) % 4 == res)
                views.append(View(name, ROUTE_WHOLE, "x%d_rs%d%s" % (x0, res, "_q15" if mode else ""), x0=x0, y0=1, right=right, below=1,
                                  gray_mode=mode))
                pad = next(p for p in range(4) if ((x0 + W + 2) * ch + p) % 4 == res)
                views.append(View(name, ROUTE_DEVICE, "x%d_rs%d_base%d%s" % (x0, res, i % 4, "_q15" if mode else ""), x0=x0, y0=1, right=2,
                                  below=1, row_pad=pad, base=i % 4, device=True, gray_mode=mode))
                i += 1
        for base in (1, 2, 3):
            views.append(View(name, ROUTE_DEVICE, "dense_base%d" % base, base=base, device=True, gray_mode=1 if base == 3 else 0))
    return views


def residue_table(views):
    """{kernel: set of first-ROI-byte residues}, {kernel: set of row stride residues}, {kernel: residues of misaligned Q15 views}"""
    first, stride, q15 = {}, {}, {}
    for v in views:
        k = gray_kernel(v.scene)
        first.setdefault(k, set()).add(v.first_roi_residue())
        stride.setdefault(k, set()).add(v.kernel_geometry()[2] % 4)
        if v.gray_mode == 1 and v.first_roi_residue() != 0:
            q15.setdefault(k, set()).add(v.first_roi_residue())
    return first, stride, q15


def group_views():
    """one swk_batch_run_groups call: a host group per staging route, a device group at a misaligned base, a reversed group and a
    single-channel group, every geometry different"""
    return [View("bgr47x94n21", ROUTE_DENSE, "group_scene"),
            View("bgr60x120n21", ROUTE_WHOLE, "group_margin", x0=13, y0=4, right=6, below=4),
            View("bgr33x75n21", ROUTE_ROWS, "group_tall_frames", y0=33, below=35),
            View("bgr67x101n21", ROUTE_2D, "group_small_roi_large_frame", x0=41, y0=30, right=100, below=80, row_pad=1),
            View("bgr47x94n21", ROUTE_DEVICE, "group_misaligned", x0=1, y0=2, right=2, below=1, row_pad=2, base=1, device=True),
            View("bgr36x52n21w2", ROUTE_WHOLE, "group_reversed", x0=3, y0=2, right=4, below=3, reverse=True),
            View("gray60x120n21", ROUTE_2D, "group_one_channel", x0=7, y0=30, right=100, below=80)]


class Guarded:
    """nbytes of output in the middle of a larger buffer filled with a sentinel: at least `guard` bytes before and after, the
    payload `shift` bytes past a 256-byte boundary.  On the device (a torch uint8 tensor) or on the host (numpy)."""
    SENTINEL = 0xA5

    def __init__(self, nbytes, device, shift=0, guard=256):
        self.nbytes, self.device, self.lead = int(nbytes), device, guard + shift
        total = self.lead + self.nbytes + guard + 8
        if device:
            import torch
            self.buf = torch.full((total,), self.SENTINEL, dtype=torch.uint8, device="cuda")
            assert self.buf.data_ptr() % 256 == 0
            self.ptr = self.buf.data_ptr() + self.lead
        else:
            raw = np.full(total + 256, self.SENTINEL, np.uint8)
            off = (-raw.ctypes.data) % 256
            self.buf = raw[off:off + total]
            self.ptr = self.buf.ctypes.data + self.lead

    def _bytes(self):
        return self.buf.cpu().numpy() if self.device else self.buf

    def read(self, dtype=np.uint8, shape=None):
        """the payload; asserts that every guard byte still holds the sentinel"""
        b = self._bytes()
        before, after = b[:self.lead], b[self.lead + self.nbytes:]
        assert (before == self.SENTINEL).all(), "%d guard bytes written before the buffer" % int((before != self.SENTINEL).sum())
        assert (after == self.SENTINEL).all(), "%d guard bytes written after the buffer" % int((after != self.SENTINEL).sum())
        out = b[self.lead:self.lead + self.nbytes].copy().view(dtype)
        return out.reshape(shape) if shape is not None else out
