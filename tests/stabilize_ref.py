"""The numpy restatement of swk_stabilize_u8 (include/swk.h) and the shaken scenes the stabilization tests share.

Restatement: grey by the oracle's Q14 / Q15 integer formula (oracle/swk_oracle.c, orc_bgr2gray), the table of summed absolute
differences in int64 for every candidate shift, UINT64_MAX where the candidate's rectangle leaves the frame, the choice by
(score, dy^2 + dx^2, dy, dx), null frames (all bytes zero) unmatched and copied through.  RefBackend offers it with the two methods
of _lib.Context that swiftwatcher_amd.stabilize.StabilizingReader calls, so the reader can be tested without a GPU.

Scenes: shaken_clip() cuts pictures out of a scene that is larger than the picture -- smooth random brickwork, a dark textured
chimney with hard edges, birds and per-frame sensor noise, all in SCENE coordinates -- at a seeded integer jitter; the "still" twin
is the same scene frames cut at jitter 0.  Frame 0 has jitter 0: it defines where the scene lies."""
import numpy as np

SHIFT_DTYPE = np.dtype([("dy", "<i4"), ("dx", "<i4"), ("sad", "<u8"), ("sad_unshifted", "<u8")])
EXCLUDED = np.uint64(0xFFFFFFFFFFFFFFFF)


def gray(bgr, mode=0):
    b, g, r = (bgr[..., k].astype(np.int64) for k in range(3))
    if mode == 0:
        y = (b * 1868 + g * 9617 + r * 4899 + (1 << 13)) >> 14
    else:
        y = (b * 3735 + g * 19235 + r * 9798 + (1 << 14)) >> 15
    return y.astype(np.uint8)


def candidates(frame_hw, rect, search):
    """[(dy, dx, inside)] in table order"""
    Hs, Ws = frame_hw
    y0, x0, Ho, Wo = rect
    return [(dy, dx, 0 <= y0 + dy and y0 + dy + Ho <= Hs and 0 <= x0 + dx and x0 + dx + Wo <= Ws)
            for dy in range(-search, search + 1) for dx in range(-search, search + 1)]


def sad_table(frames, rect, search, anchor, gray_mode=0):
    """(count, 2 S + 1, 2 S + 1) uint64"""
    frames = np.asarray(frames)
    y0, x0, Ho, Wo = rect
    side = 2 * search + 1
    a = np.asarray(anchor).astype(np.int64)
    assert a.shape == (Ho, Wo)
    out = np.full((len(frames), side, side), EXCLUDED, np.uint64)
    cands = candidates(frames.shape[1:3], rect, search)
    for f, frame in enumerate(frames):
        g = gray(frame, gray_mode).astype(np.int64)
        for dy, dx, inside in cands:
            if inside:
                out[f, dy + search, dx + search] = np.abs(a - g[y0 + dy:y0 + dy + Ho, x0 + dx:x0 + dx + Wo]).sum()
    return out


def choose(table, search):
    """(dy, dx) of one frame's table by the rule: smallest score, then dy^2 + dx^2, then dy, then dx"""
    best = None
    for dy in range(-search, search + 1):
        for dx in range(-search, search + 1):
            s = int(table[dy + search, dx + search])
            if s == int(EXCLUDED):
                continue
            key = (s, dy * dy + dx * dx, dy, dx)
            if best is None or key < best:
                best = key
    return best[2], best[3]


def stabilize(frames, rect, search, anchor, gray_mode=0):
    """(shifts SHIFT_DTYPE (count,), table, pixels (count, Ho, Wo, 3))"""
    frames = np.asarray(frames)
    y0, x0, Ho, Wo = rect
    Hs, Ws = frames.shape[1:3]
    if not (0 <= search <= 16) or y0 < 0 or x0 < 0 or y0 + Ho > Hs or x0 + Wo > Ws or np.asarray(anchor).shape != (Ho, Wo):
        raise ValueError("refused")
    table = sad_table(frames, rect, search, anchor, gray_mode)
    shifts = np.zeros(len(frames), SHIFT_DTYPE)
    pixels = np.empty((len(frames), Ho, Wo, 3), np.uint8)
    for f, frame in enumerate(frames):
        dy, dx = choose(table[f], search) if frame.any() else (0, 0)          # a null frame is not matched
        shifts[f] = (dy, dx, table[f, dy + search, dx + search], table[f, search, search])
        pixels[f] = frame[y0 + dy:y0 + dy + Ho, x0 + dx:x0 + dx + Wo]
    return shifts, table, pixels


class RefBackend:
    """_lib.Context's stabilize and bgr2gray by the restatement; calls = how often stabilize ran"""

    def __init__(self):
        self.calls = 0

    def stabilize(self, frames, rect, search, anchor, gray_mode=0, device_out=False, table=False):
        self.calls += 1
        shifts, tab, pixels = stabilize(np.asarray(frames), tuple(int(v) for v in rect), int(search), np.asarray(anchor), gray_mode)
        return shifts, (tab if table else None), pixels

    def bgr2gray(self, bgr, gray_mode=0):
        return gray(np.asarray(bgr), gray_mode)


# ---- scenes ---------------------------------------------------------------------------------------------------------------
JITTER = 5                      # largest |jitter| per axis
CLIP = dict(seed=9107, total=52, frame_hw=(110, 160), crop_region=[(30, 20), (30 + 96, 20 + 64)])
_clip_cache = {}


def _smooth(a, k):
    """separable box blur, twice (edges: the box is cut)"""
    ker = np.ones(k) / k
    for _ in range(2):
        a = np.apply_along_axis(lambda v: np.convolve(v, ker, mode="same"), 0, a)
        a = np.apply_along_axis(lambda v: np.convolve(v, ker, mode="same"), 1, a)
    return a


def scene_frames(seed, total, frame_hw, crop_region, birds=4, bird_len=(8, 12), bird_wid=(3, 5), noise=2.0, contrast=(60, 100)):
    """(total, H + 2 JITTER, W + 2 JITTER, 3) uint8 scene frames, oldest first: the picture at jitter (jy, jx) is
    scene[JITTER + jy: ... + H, JITTER + jx: ... + W].  Sky gradient with smooth brickwork of +-14 grey levels, a dark chimney with
    per-pixel texture and hard edges below the crop region's 80 % line, birds flying through the crop region, noise per frame."""
    rng = np.random.default_rng(seed)
    H, W = frame_hw
    Hs, Ws = H + 2 * JITTER, W + 2 * JITTER
    (cx0, cy0), (cx1, cy1) = crop_region
    Hc, Wc = cy1 - cy0, cx1 - cx0
    yy, xx = np.mgrid[0:Hs, 0:Ws].astype(np.float64)
    base = 150.0 + 50.0 * yy / (Hs - 1)
    brick = _smooth(rng.uniform(-1.0, 1.0, size=(Hs, Ws)), 5)
    base = base + 14.0 * brick / np.abs(brick).max()
    top = JITTER + cy0 + int(round(Hc * 0.8))
    left, right = JITTER + cx0 + int(round(Wc * 0.1)), JITTER + cx0 + int(round(Wc * 0.9))
    base[top:, left:right] = 60.0 + rng.uniform(-8, 8, size=(Hs - top, right - left))
    base[JITTER + cy0 - 6:JITTER + cy0 - 2, JITTER + cx0 + 10:JITTER + cx0 + 70] -= 45.0          # a cable above the crop region
    base[JITTER + cy0 + 5:JITTER + cy1 + 4, JITTER + cx1 + 3:JITTER + cx1 + 6] += 30.0            # a pole beside it
    bgr = np.stack([base + 10.0, base, base - 10.0], axis=-1)
    pos = np.stack([rng.uniform(0, Hc * 0.7, birds), rng.uniform(0, Wc, birds)], 1)
    speed = rng.uniform(2, 6, birds)
    heading = rng.uniform(0, 2 * np.pi, birds)
    vel = np.stack([np.sin(heading), np.cos(heading)], 1) * speed[:, None]
    length, width = rng.uniform(*bird_len, birds), rng.uniform(*bird_wid, birds)
    dark = rng.uniform(contrast[0], contrast[1], birds)
    out = np.empty((total, Hs, Ws, 3), np.uint8)
    for t in range(total):
        f = bgr.copy()
        for b in range(birds):
            by = JITTER + cy0 + (pos[b, 0] + vel[b, 0] * t) % (Hc * 0.75)
            bx = JITTER + cx0 + (pos[b, 1] + vel[b, 1] * t) % Wc
            ca, sa = np.cos(heading[b]), np.sin(heading[b])
            u = (xx - bx) * ca + (yy - by) * sa
            v = -(xx - bx) * sa + (yy - by) * ca
            f[(u / (length[b] / 2)) ** 2 + (v / (width[b] / 2)) ** 2 <= 1.0] -= dark[b]
        f += rng.normal(0.0, noise, size=f.shape)
        out[t] = np.clip(np.rint(f), 0, 255).astype(np.uint8)
    return out


def cut(scene, jitter, frame_hw):
    H, W = frame_hw
    return np.ascontiguousarray(np.stack([s[JITTER + jy:JITTER + jy + H, JITTER + jx:JITTER + jx + W] for s, (jy, jx) in zip(scene, jitter)]))


def shaken_clip(seed=CLIP["seed"], total=CLIP["total"], frame_hw=CLIP["frame_hw"], crop_region=CLIP["crop_region"]):
    """(shaken (total, H, W, 3), still (total, H, W, 3), jitter (total, 2) int: (jy, jx) of every frame, frame 0 at (0, 0)).  A
    point of the scene that the still picture shows at (r, c) lies at (r - jy, c - jx) in the shaken one: the shift that brings a
    shaken frame back onto the first is (-jy, -jx).  Read-only, cached."""
    key = (seed, total, tuple(frame_hw), tuple(map(tuple, crop_region)))
    if key not in _clip_cache:
        scene = scene_frames(seed, total, frame_hw, crop_region)
        jitter = np.random.default_rng(seed + 1).integers(-JITTER, JITTER + 1, size=(total, 2))
        jitter[0] = 0
        shaken, still = cut(scene, jitter, frame_hw), cut(scene, np.zeros_like(jitter), frame_hw)
        for a in (shaken, still, jitter):
            a.setflags(write=False)
        _clip_cache[key] = (shaken, still, jitter)
    return _clip_cache[key]


def yuv_planes(frame, chroma):
    """Per-pixel YUV planes of a BGR picture, so that cutting a picture and converting it commute: Y = the grey, limited to 16..235;
    chroma "444": U and V from B and R per pixel; "420": constant 128 (subsampling then loses nothing)."""
    y = (16 + gray(frame).astype(np.int32) * 219 // 255).astype(np.uint8)
    if chroma == "444":
        return y, (frame[..., 0] // 4 + 96).astype(np.uint8), (frame[..., 2] // 4 + 96).astype(np.uint8)
    H, W = y.shape
    c = np.full(((H + 1) // 2, (W + 1) // 2), 128, np.uint8)
    return y, c, c


CORNERS = ((40, 71), (116, 71))          # the top edge of the shaken clip's chimney, as the CLI's --corners take it


def yuv420_round_trip(frames):
    """the BGR frames a reader of the 8-bit 4:2:0 file of yuv_planes(frame, "420") hands out (the host conversion of io_y4m)"""
    from swiftwatcher_amd.io_y4m import yuv420_rect_to_bgr
    H, W = frames.shape[1:3]
    return np.stack([yuv420_rect_to_bgr(*yuv_planes(f, "420"), 0, H, 0, W) for f in frames])


def designed_case(Ho, Wo, search, count, seed, x_res=0, null_tail=0, edge=None, pad=(20, 24)):
    """Frames for the kernel tests: a textured scene moved by a seeded shift per frame (within the search range, or +-1 at search 0),
    noise added; the anchor is the grey of another noisy picture of the unmoved scene.  Returns (frames (count, Hs, Ws, 3), rect (y0, x0, Ho, Wo), anchor (Ho, Wo)).  x_res: x0 mod 4.
    edge: None, or "top" / "bottom" / "left" / "right": the nominal rectangle lies 1 px from that edge of the picture (candidates
    beyond it are excluded).  null_tail: the newest (last) frames are all zero."""
    rng = np.random.default_rng(seed)
    py, px = pad
    y0, x0 = py, px + (x_res - px) % 4
    Hs, Ws = y0 + Ho + py, x0 + Wo + px
    if edge == "top":
        y0 = 1
    elif edge == "bottom":
        y0 = Hs - Ho - 1
    elif edge == "left":
        x0 = 1
    elif edge == "right":
        x0 = Ws - Wo - 1
    M = 17
    scene = rng.integers(0, 256, size=(Hs + 2 * M, Ws + 2 * M, 3)).astype(np.float64)
    scene = np.stack([_smooth(scene[..., k], 3) for k in range(3)], -1)
    scene = (scene - scene.min()) / (scene.max() - scene.min()) * 255.0
    frames = np.empty((count, Hs, Ws, 3), np.uint8)
    for f in range(count):
        sy, sx = rng.integers(-max(search, 1), max(search, 1) + 1, size=2)
        pic = scene[M + sy:M + sy + Hs, M + sx:M + sx + Ws] + rng.normal(0.0, 1.5, size=(Hs, Ws, 3))
        frames[f] = np.clip(np.rint(pic), 0, 255)
    if null_tail:
        frames[count - null_tail:] = 0
    still = np.clip(np.rint(scene[M:M + Hs, M:M + Ws] + rng.normal(0.0, 1.5, size=(Hs, Ws, 3))), 0, 255).astype(np.uint8)
    anchor = gray(still[y0:y0 + Ho, x0:x0 + Wo], 0)
    return frames, (y0, x0, Ho, Wo), anchor
