"""Test-side restatement of the deinterlacer defined in include/swk.h (swk_yuv_deinterlace), written from that text: sample() is the
definition read aloud for one sample, picture() the same thing over whole rows with numpy, pictures() / call() the bookkeeping of
the C call (which frames give output, in which order, which rectangle of which plane).

A plane stack is an integer array (count, H, W) of d-bit sample VALUES (an MSB-aligned source is shifted down before it gets here)."""
import numpy as np


def kept_parity(tff, second):
    """parity (0 = top field) of the rows the picture of a frame's first (second = 0) or second field in time keeps"""
    first = 0 if tff else 1
    return first if not second else 1 - first


def sample(P, t, y, x, keep, second, parity0=0, temporal=True):
    """out[y][x] of the picture for (frame t, kept parity `keep`); second: it is the frame's second field in time"""
    count, H, W = P.shape
    cur = P[t]
    if (y + parity0) % 2 == keep:
        return int(cur[y][x])
    has_up, has_dn = y - 1 >= 0, y + 1 <= H - 1
    if not has_up and not has_dn:
        return int(cur[y][x])
    up = y - 1 if has_up else y + 1
    dn = y + 1 if has_dn else y - 1
    U = [int(v) for v in cur[up]]
    D = [int(v) for v in cur[dn]]
    c, e = U[x], D[x]
    xl, xr = max(x - 1, 0), min(x + 1, W - 1)
    score = abs(U[xl] - D[xl]) + abs(c - e) + abs(U[xr] - D[xr]) - 1
    pred = (c + e) >> 1

    def admissible(j):
        return x - 1 - abs(j) >= 0 and x + 1 + abs(j) <= W - 1

    def try_(j, score, pred):
        if not admissible(j):
            return False, score, pred
        sj = sum(abs(U[x + k + j] - D[x + k - j]) for k in (-1, 0, 1))
        if sj < score:
            return True, sj, (U[x + j] + D[x - j]) >> 1
        return False, score, pred

    taken, score, pred = try_(-1, score, pred)
    if taken:
        _, score, pred = try_(-2, score, pred)
    taken, score, pred = try_(1, score, pred)
    if taken:
        _, score, pred = try_(2, score, pred)
    if not temporal:
        return pred
    Pv = P[t - 1] if t - 1 >= 0 else cur
    Nx = P[t + 1] if t + 1 <= count - 1 else cur
    Bf, Af = (cur, Nx) if second else (Pv, cur)
    b, a = int(Bf[y][x]), int(Af[y][x])
    dm = (b + a) >> 1
    td0 = abs(b - a)
    td1 = (abs(int(Pv[up][x]) - c) + abs(int(Pv[dn][x]) - e)) >> 1
    td2 = (abs(int(Nx[up][x]) - c) + abs(int(Nx[dn][x]) - e)) >> 1
    diff = max(td0 >> 1, td1, td2)
    return min(max(pred, dm - diff), dm + diff)


def picture_scalar(P, t, keep, second, parity0=0, temporal=True):
    _, H, W = P.shape
    return np.array([[sample(P, t, y, x, keep, second, parity0, temporal) for x in range(W)] for y in range(H)], np.int64)


def directions(U, D):
    """(pred, chosen direction) per column of one missing row, from the rows above and below it (1-D int64 arrays)"""
    W = U.shape[0]
    x = np.arange(W)

    def at(A, idx):
        return A[np.clip(idx, 0, W - 1)]          # (inadmissible directions are masked out below: what a clipped index reads is unused)
    xl, xr = np.maximum(x - 1, 0), np.minimum(x + 1, W - 1)
    score = np.abs(U[xl] - D[xl]) + np.abs(U - D) + np.abs(U[xr] - D[xr]) - 1
    pred = (U + D) >> 1
    chosen = np.zeros(W, np.int64)

    def try_(j, allowed, score, pred, chosen):
        adm = (x - 1 - abs(j) >= 0) & (x + 1 + abs(j) <= W - 1) & allowed
        sj = sum(np.abs(at(U, x + k + j) - at(D, x + k - j)) for k in (-1, 0, 1))
        take = adm & (sj < score)
        pj = (at(U, x + j) + at(D, x - j)) >> 1
        return take, np.where(take, sj, score), np.where(take, pj, pred), np.where(take, j, chosen)
    always = np.ones(W, bool)
    t1, score, pred, chosen = try_(-1, always, score, pred, chosen)
    _, score, pred, chosen = try_(-2, t1, score, pred, chosen)
    t1, score, pred, chosen = try_(1, always, score, pred, chosen)
    _, score, pred, chosen = try_(2, t1, score, pred, chosen)
    return pred, chosen


def picture(P, t, keep, second, parity0=0, temporal=True):
    """The whole output picture for (frame t, kept parity `keep`), int64 (H, W)"""
    P = np.asarray(P).astype(np.int64)
    count, H, W = P.shape
    cur = P[t]
    out = cur.copy()
    if H == 1:
        return out
    Pv = P[t - 1] if t - 1 >= 0 else cur
    Nx = P[t + 1] if t + 1 <= count - 1 else cur
    Bf, Af = (cur, Nx) if second else (Pv, cur)
    for y in range(H):
        if (y + parity0) % 2 == keep:
            continue
        up = y - 1 if y - 1 >= 0 else y + 1
        dn = y + 1 if y + 1 <= H - 1 else y - 1
        pred, _ = directions(cur[up], cur[dn])
        if temporal:
            b, a = Bf[y], Af[y]
            dm = (b + a) >> 1
            td1 = (np.abs(Pv[up] - cur[up]) + np.abs(Pv[dn] - cur[dn])) >> 1
            td2 = (np.abs(Nx[up] - cur[up]) + np.abs(Nx[dn] - cur[dn])) >> 1
            diff = np.maximum(np.maximum(np.abs(b - a) >> 1, td1), td2)
            pred = np.minimum(np.maximum(pred, dm - diff), dm + diff)
        out[y] = pred
    return out


def pictures(P, tff, rate=2, temporal=True, has_prev=False, has_next=False, parity0=0, fn=picture):
    """The nout = rate * (count - has_prev - has_next) output pictures of one plane stack in temporal order, int64 (nout, H, W)"""
    P = np.asarray(P)
    count = P.shape[0]
    out = []
    for t in range(int(bool(has_prev)), count - int(bool(has_next))):
        for second in range(rate):
            out.append(fn(P, t, kept_parity(tff, second), second, parity0, temporal))
    return np.stack(out)


def call(y, u=None, v=None, *, subsampling=(1, 1), rect=None, tff=True, rate=2, temporal=True, has_prev=False, has_next=False,
         parity0=(0, 0)):
    """What swk_yuv_deinterlace's `planes` holds: (Y (nout, Hr, Wr), U, V (nout, ch, cw) or None) of sample-value stacks y (count, H, W),
    u, v (count, CH, CW): the whole planes are deinterlaced and then cropped.  rect = (x0, y0, Wr, Hr)."""
    sx, sy = subsampling if u is not None else (0, 0)
    H, W = y.shape[1:]
    x0, y0, Wr, Hr = rect if rect is not None else (0, 0, W, H)
    kw = dict(tff=tff, rate=rate, temporal=temporal, has_prev=has_prev, has_next=has_next)
    Y = pictures(y, parity0=parity0[0], **kw)[:, y0:y0 + Hr, x0:x0 + Wr]
    if u is None:
        return Y, None, None
    rows = slice(y0 >> sy, ((y0 + Hr - 1) >> sy) + 1)
    cols = slice(x0 >> sx, ((x0 + Wr - 1) >> sx) + 1)
    return Y, pictures(u, parity0=parity0[1], **kw)[:, rows, cols], pictures(v, parity0=parity0[1], **kw)[:, rows, cols]


def call_bgr(y, u=None, v=None, *, subsampling=(1, 1), bits=8, full_range=False, rect=None, **kw):
    """What swk_yuv_deinterlace's `bgr` holds: the conversion of swk_yuv_to_bgr (io_y4m.yuv_rect_to_bgr restates it on the host)
    applied to the whole deinterlaced pictures, cropped to rect."""
    from swiftwatcher_amd.io_y4m import yuv_rect_to_bgr
    H, W = y.shape[1:]
    x0, y0, Wr, Hr = rect if rect is not None else (0, 0, W, H)
    Y, U, V = call(y, u, v, subsampling=subsampling, rect=None, **kw)
    dt = np.uint16 if bits > 8 else np.uint8
    sx, sy = subsampling if u is not None else (0, 0)
    out = [yuv_rect_to_bgr(Y[k].astype(dt), None if U is None else U[k].astype(dt), None if V is None else V[k].astype(dt),
                           y0, y0 + Hr, x0, x0 + Wr, sx, sy, bits, full_range) for k in range(len(Y))]
    return np.stack(out)


def weave(fields_top, fields_bottom):
    """Stored frames (N, H, W) from the rows of two field-rate picture stacks: even rows from fields_top, odd rows from fields_bottom"""
    out = np.array(fields_top, copy=True)
    out[:, 1::2] = np.asarray(fields_bottom)[:, 1::2]
    return out
