"""The designed planes of tests/filter_planes.py on the CPU alone: the oracle deserves to be the expected value of
tests/test_filter_planes_gpu.py, and the planes can tell a wrong kernel from a right one.

Oracle against float64.  oracle.reference_path.bilateral_u8 (float32, the kernel's operation order; PARITY UNPINNED) equals
rint(sum / wsum) of the float64 statement at every pixel whose float64 quotient lies farther than 1e-3 from a half-integer; nearer
than that the two may differ by one level.  The pixels left out may be at most 0.5 % of all compared (a cap): with the seeds of
filter_planes.py the test leaves out 0.011 % (6,214 of 54,078,526 pixel comparisons; it prints the count) and finds no mismatch
outside them.  The oracle's threshold and opening equal numpy's and scipy's exactly.

Mutants.  Wrong kernels restated in numpy (filter_planes.mutant_*) differ from the oracle on the family meant to catch them, and only
where the mistake can show.

Outermost taps.  A lone pixel shows at distance exactly R along its row and column at the wide sets of radius 2 and 3.  At radius 4
it cannot, whatever its value: one tap at distance 4 contributes at most 0.31 of a grey level at (9, 40, 3) and 0.15 at (-1, 25, 2.5)
(filter_planes.outer_tap_quotient, float64), so the rounded output stays 0, and the same holds for a 3 x 3 block, of which a cell at
distance 4 also sees one pixel only.  The "tips" frames close that gap: four pixels at distance exactly 4 left, right, above and
below an empty cell give 1.24 and 0.61, a rounded 1 that a live mask one row AND one column too narrow loses.  A mask too narrow in
rows only (columns only) can lose nothing but the two taps above and below (left and right): the "vpair" / "hpair" frames hold just
those, 0.62 at (9, 40, 3), which shows, and 0.30 at (-1, 25, 2.5), which no plane can make show; the test asserts that arithmetic
instead."""
import numpy as np
import pytest

import filter_planes as fp

NEAR_TIE = 1e-3
LEFT_OUT_CAP = 0.005


def _bil(p):
    return (p.d, p.sc, p.ss)


@pytest.fixture(scope="module")
def lone():
    return fp.lone_families()[0]


_QUOTIENTS = {}


def _quotient(fam, bil):
    key = (fam.name, bil)
    if key not in _QUOTIENTS:
        _QUOTIENTS[key] = fp.bilateral_quotient(fam.planes, *bil)
    return _QUOTIENTS[key]


def _reference_bilateral(fam, p):
    return fp.round_u8(_quotient(fam, _bil(p)))


# ------------------------------------------------------------------ the oracle against the float64 reference
def test_oracle_equals_the_float64_reference():
    from scipy import ndimage
    compared = left_out = 0
    for fam in fp.all_families():
        for p in fam.params:
            q = _quotient(fam, _bil(p))
            near = np.abs(q - np.floor(q) - 0.5) <= NEAR_TIE
            bil, thr, opened = fp.oracle_stages(fam.name, fam.planes, p)
            want = fp.round_u8(q)
            bad = (bil != want) & ~near
            assert not bad.any(), "%s %s: %d pixels differ from float64 away from a tie, first at %s" % (
                fam.name, p, int(bad.sum()), tuple(np.argwhere(bad)[0]))
            assert np.abs(bil.astype(int) - want.astype(int)).max() <= 1, (fam.name, p)
            compared += q.size
            left_out += int(near.sum())
            assert np.array_equal(thr, np.where(bil > p.thresh, bil, 0)), (fam.name, p)
            assert np.array_equal(opened, ndimage.grey_opening(thr, size=(1, 3, 3))), (fam.name, p)
    print("near-tie pixels left out: %d of %d (%.3f %%)" % (left_out, compared, 100.0 * left_out / compared))
    assert compared > 2e7
    assert left_out <= LEFT_OUT_CAP * compared


def test_geom_planes_are_what_the_families_are():
    """the planes of the geometry buffers lie where the table says, at every residue mod 4, apart and inside the buffer"""
    for case in fp.geom_cases():
        spans = sorted((o, o + H * W) for H, W, o in case.geom)
        assert all(a[1] < b[0] and 1 <= b[0] - a[1] <= 7 for a, b in zip(spans, spans[1:])) and spans[-1][1] < case.buf.size
        assert {o % 4 for _, _, o in case.geom} == {0, 1, 2, 3}
        assert sorted((H, W) for H, W, _ in case.geom) == sorted(fp.GEOM_SHAPES)
        member = np.zeros(case.buf.size, bool)
        for (H, W, o), plane in zip(case.geom, case.planes):
            assert np.array_equal(case.buf[o:o + H * W].reshape(H, W), plane)
            member[o:o + H * W] = True
        assert (case.buf[~member] == 0xEE).all() and (~member).sum() >= 6
        assert any(not pl.any() for pl in case.planes)


def test_lone_places_cover_the_seams():
    placed = [f for f in fp.lone_layout() if f.kind in ("pixel", "block")]
    assert {f.r for f in placed} == set(fp.LONE_ROWS) and {f.c for f in placed} == set(fp.LONE_COLS)
    pixel_cols = {f.c for f in placed if f.kind == "pixel"}
    assert {62, 63, 64, 65, 126, 127, 128, 129} <= pixel_cols
    assert {f.value for f in placed if f.kind == "pixel"} == {f.value for f in placed if f.kind == "block"} == set(fp.LONE_VALUES)
    assert {f.kind for f in fp.lone_layout()} == {"pixel", "block"} | {k + str(R) for k in ("tips", "hpair", "vpair") for R in (2, 3, 4)}


# ------------------------------------------------------------------ mutant: live neighbourhood one too small
def test_outermost_taps_arithmetic():
    one = {b: fp.outer_tap_quotient(b, 1) for b in fp.WIDE + [fp.DEFAULT]}
    assert one[fp.DEFAULT] < 0.05                       # the reference's sigma_space = 1: nothing at distance R
    assert [fp.radius(b[0], b[2]) for b in fp.WIDE] == [4, 4, 3, 2]
    assert one[fp.WIDE[2]] > 0.5 and one[fp.WIDE[3]] > 0.5 and one[fp.WIDE[0]] < 0.5 and one[fp.WIDE[1]] < 0.5
    assert all(fp.outer_tap_quotient(b, 4) > 0.5 for b in fp.WIDE)
    assert fp.outer_tap_quotient(fp.WIDE[0], 2) > 0.5 and fp.outer_tap_quotient(fp.WIDE[1], 2) < 0.5


@pytest.mark.parametrize("bil", fp.WIDE, ids=lambda b: "d%d_sc%g_ss%g" % b)
def test_oracle_is_nonzero_at_distance_exactly_R(lone, bil):
    """along a row and along a column: from a lone pixel where the arithmetic allows it (radius 2 and 3), at the centre of the tips
    frames at every wide set"""
    R = fp.radius(bil[0], bil[2])
    orc_bil = fp.oracle_stages(lone.name, lone.planes, fp.P(*bil, 0, 15))[0]
    H, W = fp.LONE_SHAPE
    tips = [k for k, f in enumerate(fp.lone_layout()) if f.kind == "tips%d" % R]
    assert len(tips) >= 4
    for k in tips:
        f = fp.lone_layout()[k]
        assert lone.planes[k, f.r, f.c] == 0 and orc_bil[k, f.r, f.c] != 0, f
        box = lone.planes[k, f.r - R + 1:f.r + R, f.c - R + 1:f.c + R]
        assert not box.any() and lone.planes[k, f.r, f.c + R] and lone.planes[k, f.r + R, f.c]
    shows = []
    for k, f in enumerate(fp.lone_layout()):
        if f.kind != "pixel":
            continue
        along_row = orc_bil[k, f.r, f.c + R if f.c + R < W else f.c - R]
        along_col = orc_bil[k, f.r + R if f.r + R < H else f.r - R, f.c]
        if along_row and along_col:
            shows.append(f.value)
    if fp.outer_tap_quotient(bil, 1) > 0.5:
        assert shows, "no lone pixel shows at distance R"
    else:
        assert not shows


@pytest.mark.parametrize("bil", fp.WIDE, ids=lambda b: "d%d_sc%g_ss%g" % b)
def test_mutant_narrow_live_neighbourhood_differs_on_lone(lone, bil):
    p = fp.P(*bil, 0, 15)
    R = fp.radius(p.d, p.ss)
    orc_bil, _, orc_open = fp.oracle_stages(lone.name, lone.planes, p)
    ref = _reference_bilateral(lone, p)
    # the kernel's premise: a cell with an all-zero (2R + 1)^2 neighbourhood filters to 0
    full = fp.live_mask(lone.planes, R, R, R)
    assert not orc_bil[~full].any() and not ref[~full].any()
    ring = full & ~fp.live_mask(lone.planes, R, R - 1, R - 1)
    got = fp.mutant_narrow_live(lone.planes, p, ref)
    diff = got[0] != orc_bil
    assert diff.any(), "the lone family cannot tell a live mask one too small at %s" % (bil,)
    assert not (diff & ~ring).any()
    for rows, cols in ((True, False), (False, True)):
        one = fp.mutant_narrow_live(lone.planes, p, ref, rows=rows, cols=cols)[0] != orc_bil
        edge = full & ~fp.live_mask(lone.planes, R, R - 1 if rows else R, R - 1 if cols else R)
        assert not (one & ~edge).any()
        assert one.any() == (fp.outer_tap_quotient(bil, 2) > 0.5), (bil, rows, cols)
    # (what the outermost taps add stays below the threshold: the mistake shows in the bilateral image alone)
    assert np.array_equal(got[2], orc_open) and int(orc_bil[diff].max()) <= p.thresh


# ------------------------------------------------------------------ mutant: ring columns 64..67 dropped
@pytest.mark.parametrize("bil", [fp.DEFAULT, fp.WIDE[0]], ids=["default", "d9_sc40_ss3"])
def test_mutant_ring_columns_dropped_differs_on_lone_at_the_column_seams(lone, bil):
    p = fp.P(*bil, 0, 15)
    orc = fp.oracle_stages(lone.name, lone.planes, p)
    ref = _reference_bilateral(lone, p)
    assert np.array_equal(ref, orc[0])                  # (no tie on these frames)
    got = fp.mutant_ring_dropped(p, ref)
    W = fp.LONE_SHAPE[1]
    seam = [k for k, f in enumerate(fp.lone_layout()) if f.kind == "pixel" and f.c % 64 in (62, 63) and f.c + 2 < W]
    assert len(seam) >= 8
    for k in seam:
        assert not np.array_equal(got[0][k], orc[0][k]), fp.lone_layout()[k]
    # (a thresholded cell lost at column 62 changes the erosion from column 61 on and the dilation from column 60 on)
    for stage, cols in ((0, {62, 63}), (1, {62, 63}), (2, {60, 61, 62, 63})):
        where = np.argwhere(got[stage] != orc[stage])
        assert len(where), stage
        assert {int(c) % 64 for c in where[:, 2]} <= cols, stage
    far = [k for k, f in enumerate(fp.lone_layout()) if f.kind == "pixel" and f.c in (0, 1, 133, 134)]
    for k in far:
        assert all(np.array_equal(got[s][k], orc[s][k]) for s in range(3))


# ------------------------------------------------------------------ mutant: the wrong borders
@pytest.mark.parametrize("fam", fp.border_families(), ids=lambda f: f.name)
def test_mutant_borders_differ_on_border(fam):
    H, W = fam.planes.shape[1:]
    r, c = np.indices((H, W))
    for p in fam.params:
        if p.fma:
            continue
        R = fp.radius(p.d, p.ss)
        orc = fp.oracle_stages(fam.name, fam.planes, p)
        q = _quotient(fam, _bil(p))
        sure = np.abs(q - np.floor(q) - 0.5) > NEAR_TIE
        ref = fp.round_u8(q)
        # replicated instead of reflected border of the bilateral filter: differs, within R of an edge only
        rep = fp.mutant_borders(fam.planes, p, ref, bilateral=True, opening=False)
        diff = (rep[0] != orc[0]) & sure
        assert diff.any(), (fam.name, p)
        assert not (diff & ((r >= R) & (r < H - R) & (c >= R) & (c < W - R))[None]).any(), (fam.name, p)
        # zero border of the opening: differs, within 2 of an edge only (the oracle's own bilateral image, so nothing else differs)
        zb = fp.mutant_borders(fam.planes, p, np.asarray(orc[0]), bilateral=False, opening=True)
        assert np.array_equal(zb[1], orc[1])
        diff = zb[2] != orc[2]
        assert diff.any(), (fam.name, p)
        assert not (diff & ((r >= 2) & (r < H - 2) & (c >= 2) & (c < W - 2))[None]).any(), (fam.name, p)
        both = fp.mutant_borders(fam.planes, p, ref)
        assert not np.array_equal(both[2], orc[2]) or not np.array_equal(both[0], orc[0])


# ------------------------------------------------------------------ mutant: >= instead of >
@pytest.mark.parametrize("fam", fp.threshold_families() + [f for f in fp.dense_families() if f.name in ("dense_4x4", "dense_36x68", "dense_65x129")],
                         ids=lambda f: f.name)
def test_mutant_thresh_ge_differs_on_the_threshold_planes(fam):
    i15, i16, i255 = (fp.DENSE_FRAMES.index(n) for n in ("all15", "all16", "all255"))
    seen = set()
    for p in fam.params:
        if p.fma:
            continue
        bil, thr, _ = fp.oracle_stages(fam.name, fam.planes, p)
        got = fp.mutant_thresh_ge(p, np.asarray(bil))
        diff = got[1] != thr
        assert np.array_equal(diff, (bil == p.thresh) & (p.thresh > 0)), (fam.name, p)
        if p.thresh == 0:
            assert not diff.any()
        frame = {15: i15, 16: i16, 255: i255}.get(p.thresh)
        if frame is not None:
            assert (fam.planes[frame] == p.thresh).all() and (bil[frame] == p.thresh).all() and diff[frame].all(), (fam.name, p)
            assert not thr[frame].any() and (got[1][frame] == p.thresh).all()
            assert not np.array_equal(got[2], fp.oracle_stages(fam.name, fam.planes, p)[2])
        seen.add(p.thresh)
    assert seen >= ({15} if fam.name.startswith("dense") else set(fp.THRESHOLDS))
