"""The fused filter kernel of the batch calls (csrc/filters.hip, k_filter_fused<GEOM, R>) on the designed planes of
tests/filter_planes.py, handed to it by swk_debug_filter_fused (include/swk_debug.h) through the launchers swk_batch_run and
swk_batch_run_groups take.  Every comparison is byte for byte: the kernel and the CPU oracle perform the same float32 operations in
the same order.  tests/test_filter_planes_cpu.py holds the oracle to a float64 statement on the same planes and shows, with numpy
mutants, which mistakes each family catches.

Per family and parameter set: the three stage images equal the oracle's and the GPU stage functions'; the call with the bilateral
and thresholded outputs null gives the same opened planes; the bytes behind the device outputs are untouched.  The per-plane form
(plane sizes and byte offsets in one buffer) equals the uniform form plane by plane, whatever the order of the planes, and returns 0
between the planes.  Tables of one radius do not leak into a call at another; the batch calls' refusals hold here too."""
import ctypes

import numpy as np
import pytest

import filter_planes as fp

pytestmark = pytest.mark.gpu

STAGE_NAMES = ("bilateral", "thresh", "opened")


@pytest.fixture(scope="module")
def ctx():
    from swiftwatcher_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def _params(p, **more):
    from swiftwatcher_amd import _lib
    return _lib.default_params(bil_d=p.d, bil_sigma_color=p.sc, bil_sigma_space=p.ss, bil_fma=int(p.fma), thresh=int(p.thresh), **more)


def _same(got, want, what):
    """byte for byte, with the first differing pixel placed relative to the 32 x 64 tiles"""
    if np.array_equal(got, want):
        return
    f, r, c = (int(v) for v in np.argwhere(got != want)[0])
    raise AssertionError("%s: %d pixels differ, first in frame %d at (%d, %d) = tile (%d, %d) + (%d, %d): got %d, want %d" % (
        what, int((got != want).sum()), f, r, c, r // fp.TILE_H, c // fp.TILE_W, r % fp.TILE_H, c % fp.TILE_W, got[f, r, c], want[f, r, c]))


def _guard_intact(res, what):
    from swiftwatcher_amd import _lib
    assert res["guard"].shape == (3, _lib.DEBUG_GUARD_BYTES) and (res["guard"] == _lib.DEBUG_FILL).all(), "%s: guard bytes written" % what


def _check_uniform(ctx, fam, p):
    what = "%s %s" % (fam.name, p)
    want = fp.oracle_stages(fam.name, fam.planes, p)
    res = ctx.debug_filter_fused(fam.planes, params=_params(p))
    for key, w in zip(STAGE_NAMES, want):
        _same(res[key], w, "%s: %s against the oracle" % (what, key))
    _guard_intact(res, what)
    alone = ctx.debug_filter_fused(fam.planes, params=_params(p), bilateral=False, thresh=False)
    assert set(alone) == {"opened", "guard"}
    _same(alone["opened"], want[2], "%s: opened, the other outputs null" % what)
    _guard_intact(alone, what + " (outputs null)")
    blur = ctx.bilateral_u8(fam.planes, d=p.d, sigma_color=p.sc, sigma_space=p.ss, use_fma=bool(p.fma))
    _same(res["bilateral"], blur, "%s: bilateral against swk_bilateral_u8" % what)
    thr = ctx.thresh_tozero_u8(blur, p.thresh)
    _same(res["thresh"], thr, "%s: thresh against swk_thresh_tozero_u8" % what)
    _same(res["opened"], ctx.grey_open3x3_u8(thr), "%s: opened against swk_grey_open3x3_u8" % what)


# ------------------------------------------------------------------ the uniform form on every family
@pytest.mark.parametrize("fam", fp.dense_families() + fp.threshold_families() + fp.border_families(), ids=lambda f: f.name)
def test_family_equals_the_oracle_and_the_stage_functions(ctx, fam):
    for p in fam.params:
        _check_uniform(ctx, fam, p)


LONE = fp.lone_families()[0]


@pytest.mark.parametrize("p", LONE.params, ids=lambda p: "d%d_sc%g_ss%g_fma%d" % (p.d, p.sc, p.ss, p.fma))
def test_lone_pixels_at_the_tile_seams(ctx, p):
    assert LONE.planes.shape[1:] == fp.LONE_SHAPE and LONE.planes.shape[0] > 150
    _check_uniform(ctx, LONE, p)


# ------------------------------------------------------------------ the per-plane form
def _plane_of(flat, H, W, off):
    return flat[off:off + H * W].reshape(1, H, W)


@pytest.mark.parametrize("case", fp.geom_cases(), ids=lambda c: c.name)
def test_planes_of_several_sizes_in_one_buffer(ctx, case):
    member = np.zeros(case.buf.size, bool)
    for H, W, off in case.geom:
        member[off:off + H * W] = True
    for p in case.params:
        what = "%s %s" % (case.name, p)
        res = ctx.debug_filter_fused(case.buf, params=_params(p), geom=case.geom)
        _guard_intact(res, what)
        alone = ctx.debug_filter_fused(case.buf, params=_params(p), geom=case.geom, bilateral=False, thresh=False)
        _guard_intact(alone, what + " (outputs null)")
        assert np.array_equal(alone["opened"], res["opened"]), what
        for key in STAGE_NAMES:
            assert not res[key][~member].any(), "%s: %s is not 0 between the planes" % (what, key)
        for k, ((H, W, off), plane) in enumerate(zip(case.geom, case.planes)):
            name = "%s_plane_%dx%d" % (case.name.split("_")[0], H, W)
            want = fp.oracle_stages(name, plane[None], p)
            uni = ctx.debug_filter_fused(plane[None], params=_params(p))
            for key, w in zip(STAGE_NAMES, want):
                got = _plane_of(res[key], H, W, off)
                _same(got, w, "%s plane %d (%d x %d at %d): %s against the oracle" % (what, k, H, W, off, key))
                _same(got, uni[key], "%s plane %d (%d x %d at %d): %s against the uniform form" % (what, k, H, W, off, key))


def test_plane_order_does_not_matter(ctx):
    listed, shuffled = fp.geom_cases()
    assert [g[:2] for g in listed.geom] != [g[:2] for g in shuffled.geom]
    p = listed.params[0]
    a = ctx.debug_filter_fused(listed.buf, params=_params(p), geom=listed.geom)
    b = ctx.debug_filter_fused(shuffled.buf, params=_params(p), geom=shuffled.geom)
    by_shape = {g[:2]: g for g in shuffled.geom}
    for H, W, off in listed.geom:
        for key in STAGE_NAMES:
            assert np.array_equal(_plane_of(a[key], H, W, off), _plane_of(b[key], *by_shape[(H, W)])), (H, W, key)
    assert a["opened"].any()


# ------------------------------------------------------------------ tables do not leak between calls
def test_radius_4_then_radius_1_on_one_context(ctx):
    fam = next(f for f in fp.dense_families() if f.name == "dense_67x95")
    wide, narrow = fp.P(9, 40.0, 3.0, 0, 15), fp.P(3, 15.0, 1.0, 0, 15)
    assert fp.radius(wide.d, wide.ss) == 4 and fp.radius(narrow.d, narrow.ss) == 1
    assert not np.array_equal(fp.oracle_stages(fam.name, fam.planes, wide)[0], fp.oracle_stages(fam.name, fam.planes, narrow)[0])
    for p in (wide, narrow, wide, narrow):
        res = ctx.debug_filter_fused(fam.planes, params=_params(p))
        for key, w in zip(STAGE_NAMES, fp.oracle_stages(fam.name, fam.planes, p)):
            _same(res[key], w, "%s after another radius: %s" % (p, key))


# ------------------------------------------------------------------ refusals
def _raw_call(c, planes, params, geom=None, total=None):
    """swk_debug_filter_fused with outputs the test owns: (status, outputs and guard still as they were filled)"""
    from swiftwatcher_amd import _lib
    s = np.ascontiguousarray(planes, np.uint8)
    outs = [np.full(s.size if total is None else total, 0x3C, np.uint8) for _ in range(3)]
    guard = np.full((3, _lib.DEBUG_GUARD_BYTES), 0x3C, np.uint8)
    tab = None if geom is None else np.array(geom, _lib.DEBUG_PLANE_DTYPE)
    count, H, W = (s.shape[0], s.shape[1], s.shape[2]) if geom is None else (len(tab), 0, 0)
    rc = c._lib.swk_debug_filter_fused(c._h, _lib._ptr(s), count, H, W, _lib._ptr(tab), s.size if total is None else total,
                                       ctypes.byref(params), _lib._ptr(outs[0]), _lib._ptr(outs[1]), _lib._ptr(outs[2]), _lib._ptr(guard))
    untouched = all((o == 0x3C).all() for o in outs) and (guard == 0x3C).all()
    return rc, untouched


def test_refusals():
    """3 x 3 planes, a radius of 5, a 5-row opening window, planes that overlap, a plane past the buffer: SWK_ERR_ARG with no buffer
    made (the context's device bytes stay) and nothing written; the next valid call is right"""
    from swiftwatcher_amd import _lib
    c = _lib.Context(0)
    try:
        fam = next(f for f in fp.dense_families() if f.name == "dense_33x65")
        p = fp.P(*fp.DEFAULT, 0, 15)
        good = _lib.default_params()
        rng = np.random.default_rng(7)
        buf = rng.integers(0, 256, size=400, dtype=np.uint8)
        before = c.device_bytes
        refused = [
            ("3x3 planes", lambda: _raw_call(c, rng.integers(0, 256, size=(4, 3, 3), dtype=np.uint8), good)),
            ("4x3 planes", lambda: _raw_call(c, rng.integers(0, 256, size=(4, 4, 3), dtype=np.uint8), good)),
            ("bil_d 11", lambda: _raw_call(c, fam.planes, _lib.default_params(bil_d=11))),
            ("radius 6 from sigma_space", lambda: _raw_call(c, fam.planes, _lib.default_params(bil_d=0, bil_sigma_space=4.0))),
            ("open_kh 5", lambda: _raw_call(c, fam.planes, _lib.default_params(open_kh=5))),
            ("open_kw 1", lambda: _raw_call(c, fam.planes, _lib.default_params(open_kw=1))),
            ("planes overlap", lambda: _raw_call(c, buf, good, geom=[(10, 10, 0), (10, 10, 99)], total=400)),
            ("planes overlap, listed backwards", lambda: _raw_call(c, buf, good, geom=[(10, 10, 150), (10, 10, 51)], total=400)),
            ("plane past the buffer", lambda: _raw_call(c, buf, good, geom=[(10, 10, 0), (10, 10, 301)], total=400)),
            ("negative offset", lambda: _raw_call(c, buf, good, geom=[(10, 10, -1)], total=400)),
            ("3x3 plane in the table", lambda: _raw_call(c, buf, good, geom=[(10, 10, 0), (3, 3, 200)], total=400)),
        ]
        for name, call in refused:
            rc, untouched = call()
            assert rc == -1, name                     # SWK_ERR_ARG
            assert untouched, "%s: something was written" % name
            assert c.device_bytes == before, "%s: a buffer was made" % name
        with pytest.raises(_lib.SwkError):
            c.debug_filter_fused(fam.planes, params=_lib.default_params(bil_d=11))
        # planes that touch without overlapping and end with the buffer are served
        rc, untouched = _raw_call(c, buf, good, geom=[(10, 10, 0), (10, 10, 100), (10, 10, 300)], total=400)
        assert rc == 0 and not untouched
        res = c.debug_filter_fused(fam.planes, params=_params(p))
        for key, w in zip(STAGE_NAMES, fp.oracle_stages(fam.name, fam.planes, p)):
            _same(res[key], w, "after the refusals: %s" % key)
    finally:
        c.close()
