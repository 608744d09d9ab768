"""Where swk_batch_run puts its results (swk_api.hip, run_batch: in_place, rec_in_place, copy_out).  The reference is the plain
Context.batch_run of the same scene with host outputs (held to the CPU oracle by tests/test_ingest_routes_gpu.py).  Every output
buffer -- device or host -- lies in the middle of a larger one filled with a sentinel (helpers.Guarded): all outputs in device
memory, every plane pointer 1, 2 and 3 bytes off a dword, planes_on_device with host records, subsets of the outputs, and record caps
below the region count.  Results must be those of the reference and every guard byte must survive."""
import numpy as np
import pytest

from helpers import ATOL_AE, SCENES, STAGES, Guarded, scene

pytestmark = pytest.mark.gpu

OUT_SCENES = ("bgr67x101n21", "bgr60x120n21", "bgr33x75n5", "bgr36x52n21w2")          # F P odd (padded gray buffer), whole dwords, small, two windows


@pytest.fixture(scope="module")
def ctx():
    from swiftwatcher_amd import _lib
    c = _lib.Context(0)
    c._refs = {}
    yield c
    c.close()


def reference(ctx, name, ae=False):
    """plain batch_run with host outputs (A / E select the A/Y-state pass: a reference of its own), once per context"""
    if (name, ae) not in ctx._refs:
        _, nwin, n, _, _, _ = SCENES[name]
        ctx._refs[(name, ae)] = ctx.batch_run(scene(name), nwin, n, want_A=ae, want_E=ae)
    return ctx._refs[(name, ae)]


def run_placed(ctx, name, device, stages=STAGES, ae=False, iters=True, nseg=True, segs=True, seg_cap=255, shift=0, shifted=STAGES):
    """raw swk_batch_run of a scene with every requested output in a guarded buffer of its own (device: mem = SWK_MEM_DEVICE, one
    group, so the library works in place); the planes named in `shifted` start `shift` bytes off a 256-byte boundary.  Returns
    {output: array}; reading asserts the guards."""
    from swiftwatcher_amd import _lib
    _, nwin, n, H, W, _ = SCENES[name]
    F, P = nwin * n, H * W
    inp, _out, _res = ctx._group_io(scene(name), nwin, n, None, False, seg_cap, (), False, False)
    out = _lib.Output(mem=_lib.MEM_DEVICE if device else _lib.MEM_HOST, seg_cap=seg_cap)
    bufs = {}
    for st in stages:
        bufs[st] = (Guarded(F * P, device, shift=shift if st in shifted else 0), np.uint8, (F, H, W))
    if ae:
        for k in ("A", "E"):
            bufs[k] = (Guarded(nwin * P * n * 8, device), np.float64, (nwin, P, n))
    if iters:
        bufs["iters"] = (Guarded(nwin * 4, device), np.int32, (nwin,))
    if nseg:
        bufs["nseg"] = (Guarded(F * 4, device), np.int32, (F,))
    if segs:
        bufs["segs"] = (Guarded(F * seg_cap * 48, device), _lib.SEGMENT_DTYPE, (F, seg_cap))
    for k, (g, _dt, _sh) in bufs.items():
        setattr(out, k, g.ptr)
    ctx.batch_run_raw(inp, _lib.default_params(), out)
    return {k: g.read(dt, sh) for k, (g, dt, sh) in bufs.items()}


def check_equal(got, ref, keys=None, cap=None, where=""):
    for k in (keys if keys is not None else got):
        want = ref[k][:, :cap] if (k == "segs" and cap is not None) else ref[k]
        assert np.array_equal(got[k], want), "%s: %s differs from the host-output run" % (where, k)


# ------------------------------------------------------------------ 1. everything in device memory, one group: written in place
@pytest.mark.parametrize("name", OUT_SCENES)
def test_all_outputs_in_device_memory(ctx, name):
    got = run_placed(ctx, name, device=True, ae=True)
    assert set(got) == set(STAGES) | {"A", "E", "iters", "nseg", "segs"}
    check_equal(got, reference(ctx, name, ae=True), where=name)


@pytest.mark.parametrize("name", OUT_SCENES)
def test_all_outputs_in_guarded_host_memory(ctx, name):
    got = run_placed(ctx, name, device=False, ae=True)
    check_equal(got, reference(ctx, name, ae=True), where=name)


# ------------------------------------------------------------------ 2. plane pointers off a dword
@pytest.mark.parametrize("shifted", [STAGES, ("gray",)], ids=["all_planes", "gray_alone"])
@pytest.mark.parametrize("shift", [1, 2, 3])
@pytest.mark.parametrize("name", OUT_SCENES)
def test_plane_pointers_off_a_dword(ctx, name, shift, shifted):
    """swk.h promises plain pointers for the planes.  A misaligned X switches the integer start off (gram_u8_supported): A / E to
    ATOL_AE like test_integer_start_matches_f64_start, everything else bit for bit."""
    ref = reference(ctx, name, ae=True)
    got = run_placed(ctx, name, device=True, ae=True, shift=shift, shifted=shifted)
    check_equal(got, ref, keys=STAGES + ("iters", "nseg", "segs"), where="%s shift %d" % (name, shift))
    for k in ("A", "E"):
        err = float(np.abs(got[k] - ref[k]).max())
        assert err <= ATOL_AE, "%s shift %d: %s off by %.3g" % (name, shift, k, err)
    # ... and without A / E: the M-state pass reads X and writes the sparse image at the caller's pointers
    got = run_placed(ctx, name, device=True, shift=shift, shifted=shifted)
    check_equal(got, reference(ctx, name), where="%s shift %d (M-state)" % (name, shift))


# ------------------------------------------------------------------ 3. planes_on_device with host records
@pytest.mark.parametrize("name", ["bgr67x101n21", "bgr60x120n21"])
def test_planes_on_device_with_host_records(ctx, name):
    _, nwin, n, H, W, _ = SCENES[name]
    assert (nwin * n * H * W) % 4 == (3 if name == "bgr67x101n21" else 0)
    ref = reference(ctx, name)
    res = ctx.batch_run(scene(name), nwin, n, device_stages=True)
    planes = res["planes"]
    for st in STAGES:
        for f in range(nwin * n):
            assert np.array_equal(planes.read(st, f), ref[st][f]), (name, st, f)
        assert np.array_equal(planes.read_stack(st), ref[st]), (name, st)
    check_equal(res, ref, keys=("iters", "nseg", "segs"), where=name)
    # raw, with guards around each plane and host records
    from swiftwatcher_amd import _lib
    inp, out, host = ctx._group_io(scene(name), nwin, n, None, False, 255, (), False, False)
    out.planes_on_device = 1
    guards = {st: Guarded(nwin * n * H * W, True) for st in STAGES}
    for st, g in guards.items():
        setattr(out, st, g.ptr)
    ctx.batch_run_raw(inp, _lib.default_params(), out)
    for st, g in guards.items():
        assert np.array_equal(g.read(np.uint8, (nwin * n, H, W)), ref[st]), (name, st)
    check_equal(host, ref, keys=("iters", "nseg", "segs"), where=name + " raw")


# ------------------------------------------------------------------ 4. subsets of the outputs
SUBSETS = [dict(stages=(st,)) for st in STAGES] + [
    dict(stages=(st,), iters=False, nseg=False, segs=False) for st in ("bilateral", "thresh")] + [
    dict(stages=()), dict(stages=(), segs=False), dict(stages=(), nseg=False), dict(stages=(), nseg=False, segs=False)]
SUBSET_IDS = ["only_" + st for st in STAGES] + ["bilateral_no_records", "thresh_no_records", "records_only", "nseg_without_segs",
                                                "segs_without_nseg", "iters_only"]


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("name", ["bgr67x101n21", "bgr60x120n21"])
def test_subsets_of_outputs(ctx, name, device):
    ref = reference(ctx, name)
    _, nwin, n, _, _, _ = SCENES[name]
    for sub, label in zip(SUBSETS, SUBSET_IDS):
        got = run_placed(ctx, name, device, **sub)
        want = set(sub["stages"]) | {k for k in ("iters", "nseg", "segs") if sub.get(k, True)}
        assert set(got) == want
        check_equal(got, ref, where="%s %s" % (name, label))
        if label in ("only_gray", "iters_only", "thresh_no_records"):
            # nothing leaks from the smaller buffers into a later full run
            full = ctx.batch_run(scene(name), nwin, n)
            check_equal(full, ref, keys=STAGES + ("iters", "nseg", "segs"), where="%s full run after %s" % (name, label))
    got = run_placed(ctx, name, device)
    check_equal(got, ref, where=name + " full run after the subsets")


# ------------------------------------------------------------------ 5. record caps below the region count
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("name", ["bgr67x101n21", "bgr36x52n21w2"])
def test_record_cap_below_the_region_count(ctx, name, device):
    ref = reference(ctx, name)
    most = int(ref["nseg"].max())
    assert most >= 2, "scene %s has no frame with two regions" % name
    for cap in sorted({1, max(most - 1, 1)}):
        got = run_placed(ctx, name, device, stages=("labels",), seg_cap=cap)
        assert np.array_equal(got["nseg"], ref["nseg"]), "nseg must report the true count (cap %d)" % cap
        # [F][cap] records, densely: what follows frame f's cap records is frame f + 1's first record (or the guard, which read() checks)
        assert got["segs"].shape == (ref["segs"].shape[0], cap)
        check_equal(got, ref, cap=cap, where="%s cap %d" % (name, cap))
        assert any(int(c) > cap for c in ref["nseg"])
