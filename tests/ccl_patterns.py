"""Structured frames for the connected-component labeller (csrc/ccl.hip, k_ccl_frame and the multi-kernel path), shared by
tests/test_ccl_patterns_cpu.py and tests/test_ccl_patterns_gpu.py.

Every generator is deterministic and returns Case tuples: a uint8 image whose foreground carries many different nonzero values (the
labeller must treat any nonzero as foreground), and the counts the pattern has BY CONSTRUCTION -- runs (maximal row segments of
foreground), 4-way components, 8-way components -- or None where the construction does not give one.  The numpy restatements at the
bottom (run starts on the flattened bitmap, region records per label value, the one-workgroup kernel's LDS budget) are yardsticks
of their own: plain, slow, and independent of both the C oracle and the kernels."""
from collections import namedtuple

import numpy as np

Case = namedtuple("Case", "name img runs comps4 comps8")

RUN_CAP = 1024          # kRunCap of csrc/ccl.hip: a frame with more runs takes the per-pixel union-find


def paint(mask):
    """uint8 image, nonzero exactly where mask is set, values 1..255 changing along rows and columns"""
    mask = np.asarray(mask, bool)
    r, c = np.indices(mask.shape)
    return np.where(mask, (r * 7 + c * 13) % 255 + 1, 0).astype(np.uint8)


def _case(name, mask, runs=None, comps4=None, comps8=None):
    return Case(name, paint(mask), runs, comps4, comps8)


# ------------------------------------------------------------------ long runs across word boundaries
LONG_RUN_WIDTHS = (31, 32, 33, 63, 64, 65, 95, 97)
_EDGE = (0, 1, 30, 31)


def _run_rows(W):
    """(a, b) of every row: single runs a..b for every a mod 32 and b mod 32 in {0, 1, 30, 31}, full-width rows, last-pixel-only rows"""
    ends = [x for x in range(W) if x % 32 in _EDGE]
    rows = [(a, b) for a in ends for b in ends if a <= b]
    return rows + [(0, W - 1), (W - 1, W - 1), (0, W - 1), (W - 1, W - 1), (W - 1, W - 1)]


def long_runs(W, stacked):
    """One run per row.  stacked = False: a blank row between any two, every run its own component.  stacked = True: consecutive
    rows, so a component is a chain of consecutive rows whose runs overlap (4-way) or overlap once widened by a pixel (8-way)."""
    rows = _run_rows(W)
    step = 1 if stacked else 2
    m = np.zeros((len(rows) * step, W), bool)
    for i, (a, b) in enumerate(rows):
        m[i * step, a:b + 1] = True
    if not stacked:
        return _case("long_runs_%d" % W, m, len(rows), len(rows), len(rows))
    c4 = 1 + sum(1 for (a, b), (c, d) in zip(rows, rows[1:]) if not (c <= b and a <= d))
    c8 = 1 + sum(1 for (a, b), (c, d) in zip(rows, rows[1:]) if not (c <= b + 1 and a <= d + 1))
    return _case("long_runs_stacked_%d" % W, m, len(rows), c4, c8)


# ------------------------------------------------------------------ row-wrap adjacency
ROW_WRAP_WIDTHS = (5, 16, 31, 32, 33, 48, 64)


def row_wrap(W, H=14):
    """pixels (r, W - 1) and (r + 1, 0) on rows 1, 4, 7, ...: neighbours in the flattened bitmap, not in the image.  Two runs and two
    components per pair, at both connectivities."""
    m = np.zeros((H, W), bool)
    pairs = 0
    for r in range(1, H - 1, 3):
        m[r, W - 1] = m[r + 1, 0] = True
        pairs += 1
    return _case("row_wrap_%d" % W, m, 2 * pairs, 2 * pairs, 2 * pairs)


def row_wrap_straddles(W, H=14):
    """per pair of row_wrap(W, H): does the pair lie in two different 32-bit words of the flattened bitmap?"""
    return [((r + 1) * W) % 32 == 0 for r in range(1, H - 1, 3)]


# ------------------------------------------------------------------ diagonal contacts
def staircase(H, W, anti):
    """one pixel per row on the (anti-)diagonal: one component 8-way, one per pixel 4-way"""
    n = min(H, W)
    m = np.zeros((H, W), bool)
    for i in range(n):
        m[i, W - 1 - i if anti else i] = True
    return _case("staircase_%s_%dx%d" % ("anti" if anti else "main", H, W), m, n, n, 1)


def diagonal_contacts(W):
    """Small scenes stacked with two blank rows between them; each lists (rows, runs, comps4, comps8).  W >= 12."""
    scenes = []

    def scene(rows, runs, c4, c8):
        scenes.append((rows, runs, c4, c8))

    def row(*spans):
        r = np.zeros(W, bool)
        for a, b in spans:
            r[a:b + 1] = True
        return r

    # the row above touches only at cs - 1 / only at ce + 1: at column 0, at column W - 1, and away from the borders
    scene([row((0, 0)), row((1, 3))], 2, 2, 1)
    scene([row((W - 1, W - 1)), row((W - 4, W - 2))], 2, 2, 1)
    scene([row((4, 4)), row((5, 8))], 2, 2, 1)
    scene([row((9, 9)), row((5, 8))], 2, 2, 1)
    # the clamps: a run at column 0 must not see the last pixel of the row two above (its "column -1"), a run that ends at column
    # W - 1 must not see column 0 of its own row (its "column W" of the row above)
    scene([row((W - 1, W - 1)), row(), row((0, 2))], 2, 2, 2)
    scene([row(), row((0, 0), (W - 3, W - 1))], 2, 2, 2)
    scene([row((W - 2, W - 1)), row((0, 1))], 2, 2, 2)
    scene([row((0, 0), (W - 1, W - 1)), row((0, 0), (W - 1, W - 1)), row((1, W - 2))], 5, 3, 1)
    # one run under several separate runs of the row above: single pixels on even columns, then runs of two
    k = (W - 2) // 2
    scene([row(*[(2 * i + 1, 2 * i + 1) for i in range(k)]), row((0, W - 1))], k + 1, 1, 1)
    k3 = (W - 1) // 3
    scene([row(*[(3 * i, 3 * i + 1) for i in range(k3)]), row((1, W - 2))], k3 + 1, 1, 1)
    # ... of which the first and the last touch diagonally only
    scene([row((0, 0), (4, 4), (W - 1, W - 1)), row((1, W - 2))], 4, 3, 1)
    out, runs, c4, c8 = [], 0, 0, 0
    for rows, a, b, c in scenes:
        out += rows + [np.zeros(W, bool)] * 2
        runs, c4, c8 = runs + a, c4 + b, c8 + c
    return _case("diagonal_contacts_%d" % W, np.stack(out), runs, c4, c8)


# ------------------------------------------------------------------ long union chains
def spiral(H, W, gap=1):
    """a rectangular spiral, wall one pixel wide, `gap` background pixels between turns: one component.  A walker goes straight
    while the next gap + 1 pixels ahead are free, else turns right; it stops when it can do neither."""
    m = np.zeros((H, W), bool)
    r = c = d = turns = 0
    m[0, 0] = True
    while turns < 2:
        dr, dc = ((0, 1), (1, 0), (0, -1), (-1, 0))[d]
        ahead = [(r + dr * k, c + dc * k) for k in range(1, gap + 2)]
        inside = 0 <= ahead[0][0] < H and 0 <= ahead[0][1] < W
        if inside and not any(0 <= a < H and 0 <= b < W and m[a, b] for a, b in ahead):
            r, c, turns = r + dr, c + dc, 0
            m[r, c] = True
        else:
            d, turns = (d + 1) % 4, turns + 1
    return _case("spiral_%dx%d_gap%d" % (H, W, gap), m, None, 1, 1)


def serpentine(H, W):
    """full rows on even rows, joined alternately at the right and the left end: one component, H runs"""
    m = np.zeros((H, W), bool)
    m[::2] = True
    for k, r in enumerate(range(1, H, 2)):
        if r + 1 < H:
            m[r, W - 1 if k % 2 == 0 else 0] = True
    runs = (H + 1) // 2 + sum(1 for r in range(1, H, 2) if r + 1 < H)
    return _case("serpentine_%dx%d" % (H, W), m, runs, 1, 1)


def comb(H=64, W=128):
    """tests/test_gpu_parity.py::test_ccl's comb: full even rows joined by column 0"""
    m = np.zeros((H, W), bool)
    m[::2] = True
    m[:, 0] = True
    return _case("comb_%dx%d" % (H, W), m, H, 1, 1)


def rings(H, W, gap):
    """nested one-pixel rings, `gap` (1 or 2) background pixels between them: separate at both connectivities"""
    m = np.zeros((H, W), bool)
    k = n = 0
    while H - 2 * k >= 1 and W - 2 * k >= 1:
        m[k, k:W - k] = m[H - 1 - k, k:W - k] = True
        m[k:H - k, k] = m[k:H - k, W - 1 - k] = True
        n += 1
        k += gap + 1
    return _case("rings_%dx%d_gap%d" % (H, W, gap), m, None, n, n)


def u_shape(H=12, W=16):
    """A "U" whose left arm starts on row 1, in the first 2x2 block, and whose right arm starts on row 0: its first pixel in raster
    order is the top of the right arm, its first 2x2 block is the left arm's -- the union-find root differs between the two
    numbering rules.  A lone pixel at (0, 4) lies before the right arm in raster order and after block (0, 0) in block order: it
    is label 1 in raster order and label 2 in block order."""
    m = np.zeros((H, W), bool)
    m[1:H, 0] = True
    m[0:H, W - 3] = True
    m[H - 1, 0:W - 2] = True
    m[0, 4] = True
    # row 0: the pixel and the arm; rows 1 .. H - 2: two arms; row H - 1: the base
    return _case("u_shape_%dx%d" % (H, W), m, 2 + 2 * (H - 2) + 1, 2, 2)


# ------------------------------------------------------------------ checkerboards
def checkerboard(H, W, cell):
    r, c = np.indices((H, W))
    m = ((r // cell) + (c // cell)) % 2 == 0
    nr, nc = -(-H // cell), -(-W // cell)
    cells = (nr * nc + 1) // 2
    runs = sum(len(range((i // cell) % 2 * cell, W, 2 * cell)) for i in range(H))          # a run per cell and row
    return _case("checkerboard%d_%dx%d" % (cell, H, W), m, runs, cells, 1 if min(nr, nc) > 1 else cells)


# ------------------------------------------------------------------ exactly k runs
K_RUN_SHAPES = ((64, 96), (63, 94), (67, 95))          # P = 0 mod 4, 2 mod 4, odd: the kernel's 4-, 2- and 1-byte loads
K_RUNS = (1023, 1024, 1025)


def k_runs_isolated(H, W, k):
    """k single pixels on even rows and even columns, filled in raster order: k runs, k components"""
    per = (W + 1) // 2
    assert k <= ((H + 1) // 2) * per
    m = np.zeros((H, W), bool)
    i = np.arange(k)
    m[2 * (i // per), 2 * (i % per)] = True
    return _case("k%d_isolated_%dx%d" % (k, H, W), m, k, k, k)


def k_runs_trunk(H, W, k):
    """a full top row and k - 1 single-pixel runs hanging from it as teeth on the even columns: k runs, one component"""
    per = (W + 1) // 2
    depth, rem = divmod(k - 1, per)
    assert 1 + depth + 1 <= H
    m = np.zeros((H, W), bool)
    m[0] = True
    m[1:1 + depth, ::2] = True
    m[1 + depth, 0:2 * rem:2] = True
    return _case("k%d_trunk_%dx%d" % (k, H, W), m, k, 1, 1)


# ------------------------------------------------------------------ extreme aspect
EXTREME_SHAPES = ((1, 60000), (3, 40000), (20000, 2))
_LENS = (1, 2, 31, 32, 33, 64, 100, 1000, 3, 65)
_GAPS = (1, 2, 3, 40, 1, 700)


def _segments(W, start, lens=_LENS, gaps=_GAPS):
    row, c, i, n = np.zeros(W, bool), start, 0, 0
    while c < W:
        e = min(W, c + lens[i % len(lens)])
        row[c:e] = True
        n += 1
        c = e + gaps[i % len(gaps)]
        i += 1
    return row, n


def extreme_aspect(H, W, dense):
    """dense = False: at most RUN_CAP runs, long and short, reaching the last column and the last row (the packed run coordinates).
    dense = True: more than RUN_CAP runs, so the frame takes the per-pixel path."""
    m = np.zeros((H, W), bool)
    runs = 0
    if W > 2:
        for r in range(H):
            if dense:
                m[r], n = _segments(W, r, lens=(1, 2, 31, 3, 33), gaps=(1, 2, 1, 3))
                runs += n
            else:
                m[r] = _segments(W, 5 * r)[0]
                m[r, W - 1 - r] = True          # one of the last columns, alone or joined to the last segment: no count by construction
                runs = None
    else:
        rows = range(H) if dense else list(range(0, 300)) + list(range(H - 500, H))
        for r in rows:                           # a zigzag: 8-way one chain per stretch, 4-way a component per pixel ...
            m[r, r % 2] = True
        for r in list(rows)[40::50]:             # ... with some full rows
            m[r, :] = True
        runs = len(list(rows))
    return _case("extreme_%dx%d_%s" % (H, W, "dense" if dense else "runs"), m, runs)


# ------------------------------------------------------------------ the families, gathered
def small_families():
    """every family at frame sizes the one-workgroup kernel takes"""
    out = []
    for W in LONG_RUN_WIDTHS:
        out += [long_runs(W, False), long_runs(W, True)]
    out += [row_wrap(W) for W in ROW_WRAP_WIDTHS]
    for H, W in ((9, 9), (40, 33), (33, 70), (2, 2)):
        out += [staircase(H, W, False), staircase(H, W, True)]
    out += [diagonal_contacts(W) for W in (12, 32, 33, 65, 100)]
    out += [spiral(64, 96), spiral(63, 94, 2), spiral(67, 95), spiral(212, 424, 3), serpentine(64, 96), serpentine(67, 95),
            serpentine(212, 424), comb(), rings(64, 96, 1), rings(63, 94, 2), rings(67, 95, 1), rings(212, 424, 2), u_shape()]
    out += [checkerboard(64, 96, 1), checkerboard(63, 94, 1), checkerboard(67, 95, 1), checkerboard(212, 424, 1),
            checkerboard(64, 96, 2), checkerboard(67, 95, 2), checkerboard(212, 424, 2)]
    for H, W in K_RUN_SHAPES:
        for k in K_RUNS:
            out += [k_runs_isolated(H, W, k), k_runs_trunk(H, W, k)]
    for H, W in EXTREME_SHAPES:
        out += [extreme_aspect(H, W, False), extreme_aspect(H, W, True)]
    return out


def batch_mix(H, W):
    """same-shape frames for one batched call, run-path and per-pixel-path frames side by side: a 1025-run frame between two
    sparse ones, then the other side of the cap, an empty frame, a full one and the chains"""
    sparse = np.zeros((H, W), bool)
    sparse[3:6, 4:9] = sparse[H - 4:H - 1, W - 7:W - 2] = sparse[H // 2, :] = True
    other = np.zeros((H, W), bool)
    other[::5, 1::7] = True
    frames = [_case("sparse", sparse), k_runs_isolated(H, W, 1025), _case("sparse2", other), k_runs_trunk(H, W, 1024),
              checkerboard(H, W, 1), k_runs_isolated(H, W, 1023), _case("empty", np.zeros((H, W), bool)), k_runs_trunk(H, W, 1025),
              _case("full", np.ones((H, W), bool)), spiral(H, W), k_runs_isolated(H, W, 1024), serpentine(H, W), checkerboard(H, W, 2)]
    return frames


def tiled(case, H, W):
    """the pattern repeated (one blank row and column between copies) and cut to H x W"""
    t = np.pad(case.img, ((0, 1), (0, 1)))
    reps = (-(-H // t.shape[0]), -(-W // t.shape[1]))
    return Case(case.name + "_tiled_%dx%d" % (H, W), np.ascontiguousarray(np.tile(t, reps)[:H, :W]), None, None, None)


def large_families(H, W):
    """frames too large for the one-workgroup kernel: spiral, serpentine and long runs tiled, and the 1-pixel checkerboard"""
    return [tiled(spiral(50, 70), H, W), tiled(serpentine(41, 95), H, W), tiled(long_runs(97, True), H, W),
            tiled(long_runs(65, False), H, W), checkerboard(H, W, 1)]


# ------------------------------------------------------------------ numpy yardsticks
def run_starts_flat(img, col0=True):
    """Run starts the way k_ccl_frame finds them, restated in numpy: on the FLATTENED foreground bitmap a set bit starts a run when
    the bit before it is clear -- or when it sits in column 0 (col0), because the bit before column 0 is the last pixel of the row
    above.  col0 = False is the wrong rule, kept so that a test can show the row-wrap family tells the two apart."""
    fg = (np.asarray(img) != 0)
    H, W = fg.shape
    flat = fg.ravel()
    prev = np.concatenate([[False], flat[:-1]])
    st = flat & ~prev
    if col0:
        st |= flat & (np.arange(H * W) % W == 0)
    return st.reshape(H, W)


def count_runs(img, col0=True):
    return int(run_starts_flat(img, col0).sum())


def numpy_regionprops(lab8, alias=None):
    """region records of a u8 label plane by a plain recount per label value, ascending: (label, r0, c0, r1, c1, area, sum_r, sum_c)
    with r1 / c1 exclusive.  alias = {a: b} counts value a as value b (a wrong yardstick, for the tests that show a check can fail)."""
    lab = np.asarray(lab8).astype(np.int64)
    for a, b in (alias or {}).items():
        lab = np.where(lab == a, b, lab)
    out = []
    for v in range(1, int(lab.max()) + 1 if lab.size else 1):
        rr, cc = np.nonzero(lab == v)
        if rr.size:
            out.append((v, int(rr.min()), int(cc.min()), int(rr.max()) + 1, int(cc.max()) + 1, int(rr.size), int(rr.sum()), int(cc.sum())))
    return out


def merged_records(lab32):
    """What the records of labels_to_u8(lab32) must be, from the int32 labels: label k and every label k + 256 j united -- bounding
    box of the union, areas and coordinate sums added -- and labels that are multiples of 256 gone."""
    lab = np.asarray(lab32).astype(np.int64)
    out = []
    for v in range(1, min(255, int(lab.max())) + 1):
        rr, cc = np.nonzero((lab > 0) & (lab % 256 == v))
        if rr.size:
            out.append((v, int(rr.min()), int(cc.min()), int(rr.max()) + 1, int(cc.max()) + 1, int(rr.size), int(rr.sum()), int(cc.sum())))
    return out


# k_ccl_frame's LDS budget, restated from csrc/ccl.hip (FrameLds, kPfx, kRunCap, ccl_padded, ccl_words, ccl_frame_lds_bytes,
# ccl_frame_supported): a frame takes the one-workgroup kernel when this is at most 150 KiB and H < 32768, W < 65536.
FRAME_LDS_STRUCT = 5 * 256 * 4 + 2 * 256 * 8 + (1024 // 64) * 4 + 4 * 4
FRAME_LDS_LIMIT = 150 * 1024


def frame_lds_bytes(H, W):
    P = H * W
    words = (((H + 1) // 2) * ((W + 1) // 2) * 4 + 31) // 32
    return FRAME_LDS_STRUCT + ((P + 31) // 32) * 4 + words * 4 + ((words + 3) // 4) * 4 + RUN_CAP * 16 + (RUN_CAP // 32) * 8


def frame_kernel_takes(H, W):
    return frame_lds_bytes(H, W) <= FRAME_LDS_LIMIT and H < 32768 and W < 65536


# ------------------------------------------------------------------ the oracle against scipy
def assert_oracle_matches_scipy(orc, img):
    """oracle.reference_path.ccl_u8 in raster order == scipy.ndimage.label, 4- and 8-way; its 2x2-block order is the same
    partition, numbered by first 2x2 block in block-raster order.  Returns {connectivity: component count}."""
    from scipy import ndimage
    img = np.asarray(img)
    counts = {}
    for conn, st in [(4, ndimage.generate_binary_structure(2, 1)), (8, np.ones((3, 3), int))]:
        ref, nref = ndimage.label(img, structure=st)
        n, lab = orc.ccl_u8(img, conn, 0)
        assert n == nref
        np.testing.assert_array_equal(lab, ref)
        nb, labb = orc.ccl_u8(img, conn, 1)
        assert nb == n
        counts[conn] = n
        if conn == 4:       # block order is an 8-way (BBDT) rule; 4-way ignores it
            np.testing.assert_array_equal(labb, lab)
            continue
        # same partition, numbered by first 2x2 block in block-raster order
        pairs = np.unique(np.stack([lab.ravel(), labb.ravel()]), axis=1)
        assert pairs.shape[1] == n + (1 if (img == 0).any() else 0)
        Wb = (img.shape[1] + 1) // 2
        rr, cc = np.nonzero(labb)
        key = (rr >> 1) * Wb + (cc >> 1)
        first = np.full(nb + 1, np.iinfo(np.int64).max)
        np.minimum.at(first, labb[rr, cc], key)
        assert np.all(np.diff(first[1:]) > 0)
    return counts


# ------------------------------------------------------------------ windows whose OPENED frames have a wanted structure
def block_scene(H, W, n=21, pitch=(12, 12), counts=None, talls=None, seed=0, every=4):
    """(n, H, W, 3) frames for the whole pipeline: a flat sky of 200 with per-frame grey noise (sigma 1); every `every`-th frame
    holds dark (-100) blocks 3 wide on a regular pitch (rows, columns), at an offset that changes from frame to frame.  The j-th
    patterned frame holds its first counts[j] grid places only (None: all), of which the first talls[j] are 4 rows tall and the
    others 3.  Through the RPCA, the filter, the threshold and the opening a block comes out as a block of the same height, so
    the opened frame has (3 * blocks + tall blocks) runs and one component per block."""
    rng = np.random.default_rng(seed)
    f = np.repeat(200.0 + rng.normal(0.0, 1.0, size=(n, H, W, 1)), 3, axis=3)
    pr, pc = pitch
    for j, t in enumerate(range(0, n, every)):
        oy, ox = 1 + j % (pr - 4), 1 + (2 * j) % (pc - 4)
        places = [(r, c) for r in range(oy, H - 4, pr) for c in range(ox, W - 3, pc)]
        count = len(places) if counts is None else counts[j % len(counts)]
        tall = 0 if talls is None else talls[j % len(talls)]
        for k, (r, c) in enumerate(places[:count]):
            f[t, r:r + (4 if k < tall else 3), c:c + 3] -= 100.0
    return np.clip(np.rint(f), 0, 255).astype(np.uint8)


# name -> block_scene arguments.  The regimes in the comments are what the CPU oracle gives at the default parameters; the tests
# assert them on the oracle's output before they look at the GPU's.
SCENES = {
    # more than RUN_CAP runs (1785-1890) and more than 511 components (595-630) on every patterned frame
    "dense_212x424": dict(H=212, W=424, pitch=(12, 12)),
    "dense_211x422": dict(H=211, W=422, pitch=(12, 12)),          # P = 2 mod 4
    "dense_211x423": dict(H=211, W=423, pitch=(12, 12)),          # P odd
    # at most RUN_CAP runs (858-897) with 286-299 components: the u8 wrap happens on the run path
    "wrap_212x424": dict(H=212, W=424, pitch=(16, 19)),
    # either side of the cap: 341 blocks of which 0, 1, 2 are tall -> 1023, 1024, 1025 runs; then 300, 342, 400 blocks
    "cap_212x424": dict(H=212, W=424, pitch=(12, 12), counts=(341, 341, 341, 300, 342, 400), talls=(0, 1, 2, 0, 0, 0)),
    # small ROIs: about a hundred blocks, the run path (a small ROI cannot hold 342 blocks that survive the RPCA)
    "sparse_64x96": dict(H=64, W=96, pitch=(7, 7)),
    "sparse_63x94": dict(H=63, W=94, pitch=(7, 7)),
    "sparse_67x95": dict(H=67, W=95, pitch=(7, 7)),
}


def frame_regime(orc, opened, connectivity=8, label_order=1):
    """(runs, components) of one opened frame, from the numpy run count and the oracle's labeller"""
    return count_runs(opened), int(orc.ccl_u8(opened, connectivity, label_order)[0])
