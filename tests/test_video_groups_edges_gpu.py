"""swk_batch_run_groups at the edges of its plan (swk_api.hip, run_batch): reference-made IALM fixtures padded beside a large ROI, the
sub-batches of windows with fewer pixels than frames, the labeller's vector widths and its multi-kernel path inside a groups call, a
record cap per group, group order, 7 / 64 / 65 / 128 frames per window, device outputs, classifier inputs cut at frame corners.  Every
group must equal its lone swk_batch_run (u8 stages, iterations, records bit for bit; A / E to float64 summation order), the oracle
where it is cheap, and the reference's own numbers for the fixtures."""
import ctypes
import functools
import os

import numpy as np
import pytest

from helpers import (ATOL_AE, STAGES, check_against_lone, check_against_lone_and_oracle, check_against_oracle, lone_run, orc_seg_tuples,
                     roi_stack, seg_tuples)

pytestmark = pytest.mark.gpu

N = 21
FIXTURES = {21: ["ialm_64x96x21", "ialm_107x214x21", "ialm_47x94x21", "ialm_47x94x21_s301", "ialm_47x94x21_s302", "ialm_47x94x21_s303",
                 "ialm_47x94x21_s304", "ialm_47x94x21_s305", "ialm_107x214x21_s311", "ialm_107x214x21_s312", "ialm_212x424x21_seeded",
                 "ialm_425x850x21_seeded", "ialm_64x96x21_null5"],
            64: ["ialm_64x96x64", "ialm_40x48x64", "ialm_47x94x64", "ialm_47x94x64_quiet", "ialm_30x40x64", "ialm_212x424x64_seeded"]}
# held to 1e-6 by the accurate first iteration (test_gpu_parity.py::test_accurate_first_iteration_of_ill_conditioned_windows)
ILL_CONDITIONED = ("ialm_40x48x64", "ialm_47x94x64", "ialm_47x94x64_quiet", "ialm_30x40x64")
# rank deficient (null frames): defined, not reproduced -- against its lone run only
NOT_REPRODUCED = ("ialm_64x96x21_null5",)
SETTINGS = [(0, 0), (2, 0), (1, 1), (2, 1)]
SETTING_IDS = ["auto_pass+newton_schulz", "mfma_pass+newton_schulz", "lds_pass+jacobi", "mfma_pass+jacobi"]


@pytest.fixture(scope="module")
def orc():
    from oracle import reference_path
    return reference_path


@pytest.fixture(scope="module")
def ctx():
    from swiftwatcher_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def _fixture(golden_dir, name):
    from test_oracle_golden import seeded_frames
    g = np.load(os.path.join(golden_dir, name + ".npz"))
    return g, (seeded_frames(g) if "seed" in g.files else g["frames"])


@functools.lru_cache(maxsize=None)
def _companion(n):
    """600 x 900 BGR window (540,000 pixels): frames too large for the one-workgroup labeller, and a padded P that puts the
    accurate first iteration's pixel budget (ialm_refine.hip) far out of reach of the fixtures' windows if it were charged"""
    from swiftwatcher_amd import synthetic
    return synthetic.roi_window(4500 + n, n, 600, 900, birds=5, bird_len=(30, 50), bird_wid=(12, 20))


def _check_fixture(name, g, res, ae, tight):
    n, H, W = g["frames"].shape if "frames" in g.files else tuple(int(v) for v in g["shape"])
    assert int(res["iters"][0]) == int(g["iters"]), name
    if "sparse" in g.files and g["sparse"].size:
        np.testing.assert_array_equal(res["rpca"], g["sparse"], err_msg=name)
    else:
        from oracle.scenes import sha256
        np.testing.assert_array_equal(res["rpca"].reshape(n, -1).astype(np.int64).sum(axis=1), g["sparse_frame_sums"], err_msg=name)
        assert sha256(res["rpca"]) == str(g["sparse_sha256"]), name
    if ae:
        rows = g["rows"]
        A, E = res["A"][0], res["E"][0]
        bound = 1e-6 if tight and name in ILL_CONDITIONED else ATOL_AE
        err = max(np.abs(A[rows] - g["A_rows"]).max(), np.abs(E[rows] - g["E_rows"]).max())
        assert err <= bound, "%s: A / E off the reference by %.3g (bound %g)" % (name, err, bound)
        np.testing.assert_allclose(A.sum(axis=0), g["A_colsum"], rtol=1e-8, err_msg=name)


def _fixture_call(c, golden_dir, n, ae, companion, tight):
    """One batch_run_groups call over every fixture of n frames (one gray window each), the companion in the middle of the list when
    asked for; every group against the reference's numbers (or its lone run), the refinement counters against the lone runs'."""
    names = list(FIXTURES[n])
    loaded = [_fixture(golden_dir, nm) for nm in names]
    specs = [dict(frames=f, nwin=1, n=n) for _, f in loaded]
    fixtures = [g for g, _ in loaded]
    if companion:
        mid = len(specs) // 2
        specs.insert(mid, dict(frames=_companion(n), nwin=1, n=n))
        names.insert(mid, "companion")
        fixtures.insert(mid, None)
    kw = dict(want_A=True, want_E=True) if ae else {}
    before = c.refined_windows
    got = c.batch_run_groups(specs, **kw)
    after = c.refined_windows
    lone_delta = [0, 0]
    for gi, (name, g, spec, res) in enumerate(zip(names, fixtures, specs, got)):
        b0 = c.refined_windows
        lone = lone_run(c, spec, **kw)
        b1 = c.refined_windows
        lone_delta = [lone_delta[0] + b1[0] - b0[0], lone_delta[1] + b1[1] - b0[1]]
        if g is None or name in NOT_REPRODUCED:
            check_against_lone(gi, res, lone, ae)
        else:
            _check_fixture(name, g, res, ae, tight)
            assert np.array_equal(res["rpca"], lone["rpca"]) and np.array_equal(res["labels"], lone["labels"]), name
    # the same windows are refined as when they run alone -- none is left wanting it because of a neighbour's pixel count
    assert (after[0] - before[0], after[1] - before[1]) == tuple(lone_delta), (after, before, lone_delta)


# ------------------------------------------------------------------ 1. reference fixtures inside mixed calls
@pytest.mark.parametrize("ae", [False, True], ids=["mstate", "with_A_E"])
@pytest.mark.parametrize("n", [21, 64])
def test_reference_fixtures_beside_a_large_companion(ctx, golden_dir, n, ae):
    """Pmax = 540,000: every fixture is padded by far more than its own size.  The ill-conditioned windows of 64 frames (30x40x64's
    first shrinkage clips: its accurate first iteration is summed from the pixels) must still be refined and stay within 1e-6."""
    _fixture_call(ctx, golden_dir, n, ae, companion=True, tight=True)


@pytest.mark.parametrize("setting", SETTINGS, ids=SETTING_IDS)
def test_reference_fixtures_padded_to_the_largest_fixture(golden_dir, setting):
    """The 64-frame fixtures without the companion (Pmax = 212 x 424): a failure here points at padding, not at a fixture.  Every
    pass kernel / solver pair of test_gpu_parity.ctx; the A/Y-state pass keeps the ill-conditioned windows within 1e-6."""
    from swiftwatcher_amd import _lib
    c = _lib.Context(0)
    c.set_ialm_variant(setting[0])
    c.set_eig_method(setting[1])
    try:
        _fixture_call(c, golden_dir, 64, ae=True, companion=False, tight=setting[0] in (0, 2))
    finally:
        c.close()


# ------------------------------------------------------------------ 2. plan edges
@pytest.mark.parametrize("ae", [False, True], ids=["mstate", "with_A_E"])
@pytest.mark.parametrize("case", ["boundary", "all_below_n", "three_below_n"])
def test_sub_batch_boundary(ctx, orc, case, ae):
    """n = 24: a group with P < n runs as a sub-batch of its own at its true P; P = n (4 x 6) is padded into the main sub-batch with
    P = n + 1 (5 x 5) and 64 x 96.  A call where every group has P < n has no main sub-batch (subs[0] is erased), one with three of them."""
    n = 24
    shapes = {"boundary": [(4, 5), (4, 6), (5, 5), (64, 96)], "all_below_n": [(4, 4), (4, 5)],
              "three_below_n": [(4, 5), (4, 4), (5, 4)]}[case]
    rois = [roi_stack(600 + 10 * k, 1 + (k == 0), H, W, n=n) for k, (H, W) in enumerate(shapes)]
    specs = [dict(frames=r, nwin=1 + (k == 0), n=n) for k, r in enumerate(rois)]
    check_against_lone_and_oracle(ctx, orc, specs, rois, ae)


@pytest.mark.parametrize("shapes", [[(64, 96), (32, 40), (48, 64)], [(64, 96), (33, 47)]], ids=["vec4", "vec1"])
def test_labeller_vector_widths(ctx, orc, shapes):
    """swk_api.hip picks the word width of the per-frame-geometry labeller from every group's P, pitch and plane offset: vec4 -- all of
    them multiples of 4 (P = 6144, 1280, 3072; pitch 6144; offsets k * 21 * 6144), so vec stays 4; vec1 -- 33 x 47 = 1551 pixels is odd,
    so vec = 1.  (vec = 2 is what test_video_groups_gpu.py's mix takes.)"""
    rois = [roi_stack(700 + 10 * k, 1 + (k == 1), H, W) for k, (H, W) in enumerate(shapes)]
    specs = [dict(frames=r, nwin=1 + (k == 1), n=N) for k, r in enumerate(rois)]
    check_against_lone_and_oracle(ctx, orc, specs, rois, ae=False)


def _speckled(seed, n, H, W, spots=300, side=4, drop=100.0):
    """BGR frames of a sky with `spots` dark side x side squares per frame at new places every frame: ~290 components per frame
    survive RPCA, the filter and the opening at 600 x 900"""
    from swiftwatcher_amd import synthetic
    rng = np.random.default_rng(seed)
    bgr, _ = synthetic._background(H, W)
    out = np.empty((n, H, W, 3), np.uint8)
    for t in range(n):
        f = bgr + rng.normal(0.0, 2.5, size=(H, W, 1))
        r, c = rng.integers(0, H - side, spots), rng.integers(0, W - side, spots)
        for dy in range(side):
            for dx in range(side):
                f[r + dy, c + dx] -= drop
        out[t] = np.clip(np.rint(f), 0, 255).astype(np.uint8)
    return out


def test_multi_kernel_labeller_in_a_groups_call(ctx, orc):
    """600 x 900 frames need more LDS than the one-workgroup labeller has: inside a groups call they are copied dense into a scratch
    plane, labelled by the multi-kernel path (ncomp + f0, records at f0 * capmax) and copied back at the call's pitch.  Second of three
    groups, two windows, frames of more than 255 components; labels and records against the oracle's labelling of the call's own
    opened images."""
    big = np.concatenate([_speckled(800 + w, N, 600, 900) for w in range(2)])
    rois = [roi_stack(810, 1, 64, 96), big, roi_stack(820, 1, 47, 94)]
    specs = [dict(frames=rois[0], nwin=1, n=N), dict(frames=big, nwin=2, n=N), dict(frames=rois[2], nwin=1, n=N)]
    got = ctx.batch_run_groups(specs)
    for g, (spec, roi, res) in enumerate(zip(specs, rois, got)):
        check_against_lone(g, res, lone_run(ctx, spec), ae=False)
        if g != 1:
            check_against_oracle(orc, g, spec, roi, res)
    res = got[1]
    most = 0
    for f in range(2 * N):
        ncomp, lab = orc.ccl_u8(res["opened"][f])
        most = max(most, ncomp)
        lab8 = orc.labels_to_u8(lab)
        np.testing.assert_array_equal(res["labels"][f], lab8, err_msg="frame %d" % f)
        assert seg_tuples(res, f) == orc_seg_tuples(orc.regionprops_u8(lab8)), f
    assert most > 255


def _inputs(ctx, generation, total):
    """swk_segment_inputs_last of the batch `generation`: (network inputs, frame index per segment, skipped boxes)"""
    import torch
    from swiftwatcher_amd.segment_classification import IMAGENET_MEAN, IMAGENET_STD
    side = 24 + 2 * 8
    net = torch.zeros((max(total, 1), 3, side, side), dtype=torch.float32, device="cuda")
    fr = torch.zeros((max(total, 1),), dtype=torch.int32, device="cuda")
    t, skipped = ctx.segment_inputs_last(generation, IMAGENET_MEAN, IMAGENET_STD, net.data_ptr(), max(total, 1), pad=8,
                                         seg_frame_ptr=fr.data_ptr(), known_total=total)
    assert t == total
    return net[:total].cpu(), fr[:total].cpu(), skipped


def _inputs_against_lone_runs(ctx, specs, got):
    """the groups call's classifier inputs (got: that call's results, nothing run since) = every group's lone inputs, concatenated
    (frame indices shifted by the group's first frame).  Returns how many segments the call served."""
    import torch
    total = sum(int(np.minimum(r["nseg"], s.get("seg_cap", 255)).sum()) for s, r in zip(specs, got))
    net_g, fr_g, sk_g = _inputs(ctx, got[0]["generation"], total)
    nets, frs, sk, f0 = [], [], 0, 0
    for spec in specs:
        lone = lone_run(ctx, spec)
        t = int(np.minimum(lone["nseg"], spec.get("seg_cap", 255)).sum())
        net, fr, s = _inputs(ctx, lone["generation"], t)
        nets.append(net)
        frs.append(fr + f0)
        sk += s
        f0 += spec["nwin"] * spec["n"]
    assert torch.equal(net_g, torch.cat(nets))
    assert torch.equal(fr_g, torch.cat(frs))
    assert sk_g == sk
    return total


def test_region_record_cap_per_group(ctx):
    """Caps 255, 17 and 1 in one call (records strided by the largest): every group equals its lone run at its own cap, and the
    classifier inputs cover sum(min(nseg, cap)) segments -- the lone runs' inputs, concatenated."""
    from swiftwatcher_amd import synthetic
    crowd = dict(birds=40, bird_len=(5, 8), bird_wid=(3, 5))
    specs = [dict(frames=synthetic.roi_window(900 + k, N, 64, 96, **crowd), nwin=1, n=N, seg_cap=cap) for k, cap in enumerate((255, 17, 1))]
    got = ctx.batch_run_groups(specs)
    assert _inputs_against_lone_runs(ctx, specs, got) > 21          # (the groups call's batch is read before any lone run)
    for g, (spec, res) in enumerate(zip(specs, got)):
        assert res["segs"].shape == (N, spec["seg_cap"])
        check_against_lone(g, res, lone_run(ctx, spec), ae=False)
        assert (res["nseg"] > 17).any(), g


def test_group_order_does_not_change_results(ctx):
    """The same groups in two orders (every offset, sub-batch position and padded pitch moves): each group's results identical,
    A and E included."""
    rois = [roi_stack(1000, 2, 64, 96), roi_stack(1010, 1, 4, 5), roi_stack(1020, 1, 47, 94), roi_stack(1030, 1, 30, 40)]
    specs = [dict(frames=r, nwin=2 if k == 0 else 1, n=N) for k, r in enumerate(rois)]
    kw = dict(want_A=True, want_E=True)
    a = ctx.batch_run_groups(specs, **kw)
    perm = [2, 0, 3, 1]
    b = ctx.batch_run_groups([specs[k] for k in perm], **kw)
    for j, k in enumerate(perm):
        for key in STAGES + ("iters", "nseg", "segs", "A", "E"):
            assert np.array_equal(a[k][key], b[j][key]), (k, key)


@pytest.mark.parametrize("ae", [False, True], ids=["mstate", "with_A_E"])
@pytest.mark.parametrize("n", [7, 64, 65, 128])
def test_frames_per_window(ctx, orc, n, ae):
    """Mixed calls at 7 and 64 frames (matrix-core kernels) and 65 and 128 (the wide f64 kernels)."""
    shapes = {7: [(96, 128, 2), (64, 100, 1), (72, 88, 1)], 64: [(48, 64, 1), (40, 56, 2), (33, 47, 1)],
              65: [(40, 56, 1), (33, 47, 1), (48, 64, 1)], 128: [(37, 51, 1), (32, 40, 1), (40, 48, 1)]}[n]
    rois = [roi_stack(1100 + 10 * k + n, nwin, H, W, n=n) for k, (H, W, nwin) in enumerate(shapes)]
    specs = [dict(frames=r, nwin=s[2], n=n) for r, s in zip(rois, shapes)]
    check_against_lone_and_oracle(ctx, orc, specs, rois, ae)


def test_device_outputs(ctx):
    """Two groups through raw swk_input / swk_output structs with every output in device memory (torch tensors, pre-filled with a
    sentinel): stage planes, A, E, iterations, segment counts and records equal the same call with host outputs."""
    import torch
    from swiftwatcher_amd import _lib
    specs = [dict(frames=roi_stack(1200, 2, 64, 96), nwin=2, n=N), dict(frames=roi_stack(1210, 1, 47, 94), nwin=1, n=N)]
    host = ctx.batch_run_groups(specs, want_A=True, want_E=True)
    ins = (_lib.Input * 2)()
    outs = (_lib.Output * 2)()
    dev = []
    for g, spec in enumerate(specs):
        nwin = spec["nwin"]
        F, H, W = nwin * N, spec["frames"].shape[1], spec["frames"].shape[2]
        ins[g], _, _ = ctx._group_io(spec["frames"], nwin, N, None, False, 255, (), False, False)
        t = {k: torch.full((F, H, W), 7, dtype=torch.uint8, device="cuda") for k in STAGES}
        t["A"] = torch.full((nwin, H * W, N), -1.0, dtype=torch.float64, device="cuda")
        t["E"] = torch.full((nwin, H * W, N), -1.0, dtype=torch.float64, device="cuda")
        t["iters"] = torch.full((nwin,), -1, dtype=torch.int32, device="cuda")
        t["nseg"] = torch.full((F,), -1, dtype=torch.int32, device="cuda")
        t["segs"] = torch.full((F, 255 * _lib.SEGMENT_DTYPE.itemsize), 7, dtype=torch.uint8, device="cuda")
        outs[g] = _lib.Output(mem=_lib.MEM_DEVICE, seg_cap=255, **{k: v.data_ptr() for k, v in t.items()})
        dev.append(t)
    lib = _lib.load()
    assert lib.swk_batch_run_groups(ctx._h, ins, 2, ctypes.byref(_lib.default_params()), outs) == 0
    torch.cuda.synchronize()
    for g, (t, res) in enumerate(zip(dev, host)):
        for key in STAGES + ("A", "E", "iters", "nseg"):
            assert np.array_equal(t[key].cpu().numpy(), res[key]), (g, key)
        segs = np.frombuffer(t["segs"].cpu().numpy().tobytes(), _lib.SEGMENT_DTYPE).reshape(res["segs"].shape)
        assert np.array_equal(segs, res["segs"]), g


def test_segment_inputs_at_frame_corners(ctx):
    """BGR groups whose crops touch the top-left and the bottom-right corner of their frames (the classifier's crop boxes are pushed
    back inside the frame there), and one with a negative frame stride: classifier inputs and frame indices equal the lone runs'."""
    from swiftwatcher_amd import synthetic
    Hf, Wf, Hc, Wc = 90, 140, 64, 96
    crowd = dict(birds=10, bird_len=(6, 10), bird_wid=(3, 5))
    tl = synthetic.full_frames(1300, N, [(0, 0), (Wc, Hc)], frame_hw=(Hf, Wf), **crowd)
    br = synthetic.full_frames(1301, N, [(Wf - Wc, Hf - Hc), (Wf, Hf)], frame_hw=(Hf, Wf), **crowd)
    rv = synthetic.roi_window(1302, N, 48, 80, **crowd)
    specs = [dict(frames=tl, nwin=1, n=N, crop=(0, 0, Wc, Hc)), dict(frames=br, nwin=1, n=N, crop=(Wf - Wc, Hf - Hc, Wc, Hc)),
             dict(frames=np.ascontiguousarray(rv[::-1]), nwin=1, n=N, reverse_frames=True)]
    got = ctx.batch_run_groups(specs)
    assert _inputs_against_lone_runs(ctx, specs, got) > 20
    for g, (spec, res) in enumerate(zip(specs, got)):
        check_against_lone(g, res, lone_run(ctx, spec), ae=False)
    np.testing.assert_array_equal(got[2]["gray"], ctx.bgr2gray(rv))
