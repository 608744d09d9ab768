"""The numpy restatement of swk_stabilize_subpel_u8 (include/swk.h) and the sub-pixel shaken scene its tests share.

Restatement: stage 1 is stabilize_ref's (swk_stabilize_u8's search); stage 2 scores the 25 total shifts (4 dy + qy, 4 dx + qx) in
quarter pixels around stage 1's winner on the grey resampled with the 4-tap Catmull-Rom filter T in units of 1/128 -- separable,
one rounding, int64 throughout --, excludes those whose footprint leaves the frame, chooses by (score, Qy^2 + Qx^2, Qy, Qx) and
resamples B, G and R at the choice.  RefSubpelBackend offers it with the methods of _lib.Context that StabilizingReader calls.

Scene: subpel_clip() renders stabilize_ref.scene_frames' ingredients -- sky gradient, smooth brickwork, a dark textured chimney with
hard edges, a cable, a pole, birds, sensor noise -- at 4 x supersampling, blurs them optically (Gaussian, SIGMA pixels), cuts every
frame at a seeded jitter in quarter pixels (one supersample = a quarter pixel) and integrates 4 x 4 boxes to pixels.  Frame 0 has
jitter 0; the "still" twin is every frame cut at jitter 0.  The first BIRD_FREE frames show no bird."""
import numpy as np

import stabilize_ref as ref1

SUBSHIFT_DTYPE = np.dtype([("dy", "<i4"), ("dx", "<i4"), ("qy_total", "<i4"), ("qx_total", "<i4"), ("sad", "<u8"), ("sad_int", "<u8"),
                           ("sad_unshifted", "<u8")])
EXCLUDED = ref1.EXCLUDED
T = np.array([[0, 128, 0, 0], [-9, 111, 29, -3], [-8, 72, 72, -8], [-3, 29, 111, -9]], np.int64)
V_BOUND = (144 * 144 + 16 * 16) * 255          # positive taps sum to at most 144, negative ones to -16, pixels are 0..255


def axis_inside(o, size, lim, Q):
    """one axis of a candidate: phase 0 needs the rectangle [o + i, o + i + size), another phase the footprint [o + i - 1, o + i + size + 2)"""
    i, p = Q >> 2, Q & 3                            # floor and 0..3, also for negative Q
    return (0 <= o + i - 1 and o + i + size + 2 <= lim) if p else (0 <= o + i and o + i + size <= lim)


def admissible(frame_hw, rect, Qy, Qx):
    y0, x0, Ho, Wo = rect
    return axis_inside(y0, Ho, frame_hw[0], Qy) and axis_inside(x0, Wo, frame_hw[1], Qx)


def resample_unclamped(plane, rect, Qy, Qx):
    """v of the definition, int64 (Ho, Wo[, channels]), for an admissible (Qy, Qx); plane (Hs, Ws[, channels]).  Taps of weight zero
    are not read (at phase 0 they may lie outside the plane)."""
    y0, x0, Ho, Wo = rect
    g = np.asarray(plane).astype(np.int64)
    iy, py, ix, px = Qy >> 2, Qy & 3, Qx >> 2, Qx & 3
    h = 0
    for k in range(4):
        if T[px, k]:
            a = x0 + ix - 1 + k
            assert 0 <= a and a + Wo <= g.shape[1]
            h = h + T[px, k] * g[:, a:a + Wo]
    v = 0
    for k in range(4):
        if T[py, k]:
            a = y0 + iy - 1 + k
            assert 0 <= a and a + Ho <= g.shape[0]
            v = v + T[py, k] * h[a:a + Ho]
    return v


def resample(plane, rect, Qy, Qx):
    """R of the definition, uint8"""
    return np.clip((resample_unclamped(plane, rect, Qy, Qx) + 8192) >> 14, 0, 255).astype(np.uint8)


def sub_table(grey, rect, dy, dx, anchor):
    """(5, 5) uint64 of one frame: the scores of (4 dy + qy, 4 dx + qx), EXCLUDED where not admissible"""
    a = np.asarray(anchor).astype(np.int64)
    out = np.full((5, 5), EXCLUDED, np.uint64)
    for qy in range(-2, 3):
        for qx in range(-2, 3):
            Qy, Qx = 4 * dy + qy, 4 * dx + qx
            if admissible(grey.shape, rect, Qy, Qx):
                out[qy + 2, qx + 2] = np.abs(a - resample(grey, rect, Qy, Qx).astype(np.int64)).sum()
    return out


def choose(table, dy, dx):
    """(Qy, Qx) of one frame's (5, 5) table: smallest score, then Qy^2 + Qx^2, then Qy, then Qx"""
    best = None
    for qy in range(-2, 3):
        for qx in range(-2, 3):
            s = int(table[qy + 2, qx + 2])
            if s == int(EXCLUDED):
                continue
            Qy, Qx = 4 * dy + qy, 4 * dx + qx
            key = (s, Qy * Qy + Qx * Qx, Qy, Qx)
            if best is None or key < best:
                best = key
    return best[2], best[3]


def stabilize_subpel(frames, rect, search, anchor, gray_mode=0):
    """(records SUBSHIFT_DTYPE (count,), (stage 1's table, the quarter-pixel table (count, 5, 5)), pixels (count, Ho, Wo, 3))"""
    frames = np.asarray(frames)
    rect = tuple(int(v) for v in rect)
    first, table, _ = ref1.stabilize(frames, rect, search, anchor, gray_mode)
    y0, x0, Ho, Wo = rect
    recs = np.zeros(len(frames), SUBSHIFT_DTYPE)
    sub = np.empty((len(frames), 5, 5), np.uint64)
    pixels = np.empty((len(frames), Ho, Wo, 3), np.uint8)
    for f, frame in enumerate(frames):
        dy, dx = int(first[f]["dy"]), int(first[f]["dx"])
        sub[f] = sub_table(ref1.gray(frame, gray_mode), rect, dy, dx, anchor)
        Qy, Qx = choose(sub[f], dy, dx) if frame.any() else (0, 0)           # a null frame is not matched (its dy = dx = 0)
        recs[f] = (dy, dx, Qy, Qx, sub[f, Qy - 4 * dy + 2, Qx - 4 * dx + 2], first[f]["sad"], first[f]["sad_unshifted"])
        pixels[f] = resample(frame, rect, Qy, Qx)
    return recs, (table, sub), pixels


class RefSubpelBackend:
    """_lib.Context's stabilize, stabilize_subpel and bgr2gray by the restatements; calls / subpel_calls = how often each ran"""

    def __init__(self):
        self.calls = 0
        self.subpel_calls = 0
        self.rects = []

    def stabilize(self, frames, rect, search, anchor, gray_mode=0, device_out=False, table=False):
        self.calls += 1
        self.rects.append((tuple(np.asarray(frames).shape[1:3]), tuple(int(v) for v in rect)))
        shifts, tab, pixels = ref1.stabilize(np.asarray(frames), tuple(int(v) for v in rect), int(search), np.asarray(anchor), gray_mode)
        return shifts, (tab if table else None), pixels

    def stabilize_subpel(self, frames, rect, search, anchor, gray_mode=0, device_out=False, table=False):
        self.subpel_calls += 1
        self.rects.append((tuple(np.asarray(frames).shape[1:3]), tuple(int(v) for v in rect)))
        recs, tabs, pixels = stabilize_subpel(np.asarray(frames), rect, int(search), np.asarray(anchor), gray_mode)
        return recs, (tabs if table else None), pixels

    def bgr2gray(self, bgr, gray_mode=0):
        return ref1.gray(np.asarray(bgr), gray_mode)


def step_plane(H, W, period=3):
    """(H, W, 3) of 0 / 255 blocks `period` pixels wide and high, all channels equal: the filter's negative lobes drive the unclamped
    value below 0 beside a 255 block and above 255 inside one"""
    yy, xx = np.mgrid[0:H, 0:W]
    p = (((yy // period) + (xx // period)) % 2 * 255).astype(np.uint8)
    return np.repeat(p[:, :, None], 3, 2)


# ---- the scene --------------------------------------------------------------------------------------------------------------
SS = 4                          # supersampling: one supersample = a quarter pixel
MARGIN = 6                      # scene pixels around the picture
JITTER_Q = 16                   # largest |jitter| per axis in quarter pixels (4 px)
BIRD_FREE = 21                  # frames 0 .. BIRD_FREE - 1 show no bird
SIGMA = 0.45                    # optical blur, pixels
NOISE = 1.0                     # sensor noise, grey levels (at scene_frames' 2.0 the segment counts of two noise realisations of the
                                # still clip differ by as much as the integer stage's surplus of segments, 1-4 in about 105)
CHIMNEY = (8, 1)                # the chimney's texture: +- grey levels, in cells of so many pixels (scene_frames: +-8 per pixel)
CLIP = dict(seed=4242, total=52, frame_hw=(110, 160), crop_region=[(30, 20), (30 + 96, 20 + 64)])
_clip_cache = {}


def _gauss_rows(a, sigma):
    """Gaussian blur along axis 0 and 1, sigma in samples (edges: the kernel is cut)"""
    n = int(np.ceil(4 * sigma))
    ker = np.exp(-0.5 * (np.arange(-n, n + 1) / sigma) ** 2)
    ker /= ker.sum()
    for axis in (0, 1):
        a = np.apply_along_axis(lambda v: np.convolve(v, ker, mode="same"), axis, a)
    return a


def _static_scene(rng, frame_hw, crop_region, chimney=CHIMNEY):
    """the unmoving grey scene at SS x, float64 (SS Hs, SS Ws), blurred"""
    H, W = frame_hw
    Hs, Ws = H + 2 * MARGIN, W + 2 * MARGIN
    (cx0, cy0), (cx1, cy1) = crop_region
    Hc, Wc = cy1 - cy0, cx1 - cx0
    yy = np.arange(SS * Hs, dtype=np.float64)[:, None] / SS
    base = 150.0 + 50.0 * yy / (Hs - 1) + np.zeros((SS * Hs, SS * Ws))
    brick = ref1._smooth(rng.uniform(-1.0, 1.0, size=(SS * Hs, SS * Ws)), 5 * SS)
    base = base + 14.0 * brick / np.abs(brick).max()
    top = MARGIN + cy0 + int(round(Hc * 0.8))
    left, right = MARGIN + cx0 + int(round(Wc * 0.1)), MARGIN + cx0 + int(round(Wc * 0.9))
    amp, block = chimney
    cells = rng.uniform(-amp, amp, size=(-(-(Hs - top) // block), -(-(right - left) // block)))
    texture = np.kron(cells, np.ones((SS * block, SS * block)))[:SS * (Hs - top), :SS * (right - left)]
    base[SS * top:, SS * left:SS * right] = 60.0 + texture
    base[SS * (MARGIN + cy0 - 6):SS * (MARGIN + cy0 - 2), SS * (MARGIN + cx0 + 10):SS * (MARGIN + cx0 + 70)] -= 45.0      # a cable
    base[SS * (MARGIN + cy0 + 5):SS * (MARGIN + cy1 + 4), SS * (MARGIN + cx1 + 3):SS * (MARGIN + cx1 + 6)] += 30.0        # a pole
    return _gauss_rows(base, SIGMA * SS)


def subpel_scene(seed, total, frame_hw, crop_region, birds=4, bird_len=(8, 12), bird_wid=(3, 5), noise=2.0, contrast=(60, 100),
                 bird_free=BIRD_FREE, chimney=None):
    """(static (SS Hs, SS Ws) float64, [per frame: list of (y, x, blurred bird patch to subtract)], rng for the noise)"""
    rng = np.random.default_rng(seed)
    H, W = frame_hw
    (cx0, cy0), (cx1, cy1) = crop_region
    Hc, Wc = cy1 - cy0, cx1 - cx0
    static = _static_scene(rng, frame_hw, crop_region, chimney or CHIMNEY)
    pos = np.stack([rng.uniform(0, Hc * 0.7, birds), rng.uniform(0, Wc, birds)], 1)
    speed = rng.uniform(2, 6, birds)
    heading = rng.uniform(0, 2 * np.pi, birds)
    vel = np.stack([np.sin(heading), np.cos(heading)], 1) * speed[:, None]
    length, width = rng.uniform(*bird_len, birds), rng.uniform(*bird_wid, birds)
    dark = rng.uniform(contrast[0], contrast[1], birds)
    half = int(np.ceil(bird_len[1] / 2)) + 3                                     # patch half-size in pixels
    uu = (np.arange(-half * SS, half * SS + 1, dtype=np.float64)) / SS
    py, px = np.meshgrid(uu, uu, indexing="ij")
    patches = []
    for t in range(total):
        here = []
        for b in range(birds if t >= bird_free else 0):
            by = MARGIN + cy0 + (pos[b, 0] + vel[b, 0] * t) % (Hc * 0.75)
            bx = MARGIN + cx0 + (pos[b, 1] + vel[b, 1] * t) % Wc
            iy, ix = int(round(by * SS)), int(round(bx * SS))                    # the bird's centre on the supersample grid
            ca, sa = np.cos(heading[b]), np.sin(heading[b])
            u = px * ca + py * sa
            v = -px * sa + py * ca
            mask = ((u / (length[b] / 2)) ** 2 + (v / (width[b] / 2)) ** 2 <= 1.0).astype(np.float64)
            here.append((iy - half * SS, ix - half * SS, dark[b] * _gauss_rows(mask, SIGMA * SS)))
        patches.append(here)
    return static, patches, rng, noise


def _render(static, patches, jitter_q, frame_hw, noise_fields):
    H, W = frame_hw
    out = np.empty((len(patches), H, W, 3), np.uint8)
    for t, (here, (jy, jx)) in enumerate(zip(patches, jitter_q)):
        hi = static
        if here:
            hi = static.copy()
            for y, x, patch in here:
                hi[y:y + patch.shape[0], x:x + patch.shape[1]] -= patch
        a, b = SS * MARGIN + int(jy), SS * MARGIN + int(jx)
        grey = hi[a:a + SS * H, b:b + SS * W].reshape(H, SS, W, SS).mean(axis=(1, 3))            # the sensor's box pixels
        bgr = np.stack([grey + 10.0, grey, grey - 10.0], axis=-1) + noise_fields[t]
        out[t] = np.clip(np.rint(bgr), 0, 255).astype(np.uint8)
    return out


def subpel_clip(seed=CLIP["seed"], total=CLIP["total"], frame_hw=CLIP["frame_hw"], crop_region=CLIP["crop_region"], noise=NOISE,
                integer_jitter=False, **scene_kw):
    """(shaken (total, H, W, 3), still (total, H, W, 3), jitter_q (total, 2) int: (jy, jx) of every frame in QUARTER pixels, frame 0
    at (0, 0)).  A point that the still picture shows at (r, c) lies at (r - jy / 4, c - jx / 4) in the shaken one: the total shift
    that brings a shaken frame back onto the first is (Qy, Qx) = (-jy, -jx).  Both clips carry the same noise per frame.
    integer_jitter: the jitter is a multiple of 4.  Read-only, cached."""
    key = (seed, total, tuple(frame_hw), tuple(map(tuple, crop_region)), noise, integer_jitter, tuple(sorted(scene_kw.items())))
    if key not in _clip_cache:
        static, patches, rng, noise = subpel_scene(seed, total, frame_hw, crop_region, noise=noise, **scene_kw)
        H, W = frame_hw
        fields = rng.normal(0.0, noise, size=(total, H, W, 3)) if noise else np.zeros((total, 1, 1, 3))
        jrng = np.random.default_rng(seed + 1)
        jitter = jrng.integers(-JITTER_Q // 4, JITTER_Q // 4 + 1, size=(total, 2)) * 4 if integer_jitter \
            else jrng.integers(-JITTER_Q, JITTER_Q + 1, size=(total, 2))
        jitter[0] = 0
        shaken = _render(static, patches, jitter, frame_hw, fields)
        still = _render(static, patches, np.zeros_like(jitter), frame_hw, fields)
        for a in (shaken, still, jitter):
            a.setflags(write=False)
        _clip_cache[key] = (shaken, still, jitter)
    return _clip_cache[key]


def designed_case(Ho, Wo, search, count, seed, x_res=0, null_tail=0, edge=None, gap=1, pad=(22, 24), steps=False, extreme=False):
    """Frames for the kernel tests: a smooth textured scene at SS x moved by a seeded shift in quarter pixels per frame (within the
    search range; +-1 px at search 0), box-integrated, noise added; the anchor is the grey of another noisy picture of the unmoved
    scene.  Returns (frames (count, Hs, Ws, 3), rect (y0, x0, Ho, Wo), anchor (Ho, Wo)).  x_res: x0 mod 4.  edge: None or "top" /
    "bottom" / "left" / "right": the nominal rectangle lies `gap` px from that edge of the picture.  null_tail: the newest frames are
    all zero.  steps: the scene is step_plane (0 / 255 blocks, no noise) moved by whole pixels, and the anchor is the unmoved picture
    resampled at (Qy, Qx) = (1, -2): the winning candidates then lie at non-zero phases where the filter overshoots.  extreme: frame 0 is moved by (-search, +search) px and frame 1, where there
    is one, by (+search, -search) px exactly, so stage 1's winners reach +-S."""
    rng = np.random.default_rng(seed)
    py, px = pad
    y0, x0 = py, px + (x_res - px) % 4
    Hs, Ws = y0 + Ho + py, x0 + Wo + px
    if edge == "top":
        y0 = gap
    elif edge == "bottom":
        y0 = Hs - Ho - gap
    elif edge == "left":
        x0 = gap
    elif edge == "right":
        x0 = Ws - Wo - gap
    M = 18
    lim = max(search, 1)
    moves = rng.integers(-4 * lim, 4 * lim + 1, size=(count, 2))
    if extreme:
        moves[0] = (-4 * search, 4 * search)
        if count > 1:
            moves[1] = (4 * search, -4 * search)
    frames = np.empty((count, Hs, Ws, 3), np.uint8)
    if steps:
        scene = step_plane(Hs + 2 * M, Ws + 2 * M).astype(np.float64)
        moves = (moves // 4) * 4
        cut = lambda sy, sx: scene[M + sy // 4:M + sy // 4 + Hs, M + sx // 4:M + sx // 4 + Ws]
        sigma = 0.0
    else:
        hi = rng.integers(0, 256, size=(SS * (Hs + 2 * M) // 2, SS * (Ws + 2 * M) // 2, 3)).astype(np.float64)
        hi = np.stack([np.kron(ref1._smooth(hi[..., k], 5), np.ones((2, 2))) for k in range(3)], -1)          # smooth at the 4 x scale
        hi = (hi - hi.min()) / (hi.max() - hi.min()) * 255.0
        cut = lambda sy, sx: hi[SS * M + sy:SS * M + sy + SS * Hs, SS * M + sx:SS * M + sx + SS * Ws].reshape(Hs, SS, Ws, SS, 3).mean(axis=(1, 3))
        sigma = 1.5
    for f in range(count):
        pic = cut(int(moves[f, 0]), int(moves[f, 1]))
        frames[f] = np.clip(np.rint(pic + (rng.normal(0.0, sigma, size=(Hs, Ws, 3)) if sigma else 0.0)), 0, 255)
    if null_tail:
        frames[count - null_tail:] = 0
    still = np.clip(np.rint(cut(0, 0) + (rng.normal(0.0, sigma, size=(Hs, Ws, 3)) if sigma else 0.0)), 0, 255).astype(np.uint8)
    if steps:                    # the anchor is the unmoved picture a quarter pixel down and half a pixel to the left, by the defined filter
        anchor = resample(still[..., 0], (y0, x0, Ho, Wo), 1, -2)
    else:
        anchor = ref1.gray(still[y0:y0 + Ho, x0:x0 + Wo], 0)
    return frames, (y0, x0, Ho, Wo), anchor
