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
