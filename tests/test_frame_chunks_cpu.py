"""The helpers of the size-edge tests (tests/frame_chunks.py), without a GPU: periodic stacks, the distinct-output rule, the comparison
against a host stand-in of a stale f0, the generators' outputs on the CPU restatements, and the inventory of every place in
csrc/*.hip where a frame or window count meets a grid's y / z extent."""
import numpy as np
import pytest

import frame_chunks as fc
from frame_chunks import F1, F2, K


@pytest.fixture(scope="module")
def orc():
    from oracle import reference_path
    return reference_path


# ------------------------------------------------------------------ the helpers
def test_frame_counts():
    assert F1 == 32768 + 37 and F2 == 2 * 32768 + 5
    assert F1 // fc.CHUNK == 1 and F1 % fc.CHUNK == 37          # two launches, the second ragged
    assert F2 // fc.CHUNK == 2 and 0 < F2 % fc.CHUNK < K          # three: the middle one full
    assert np.gcd(K, fc.CHUNK) == 1 and np.gcd(K, fc.BATCH_N) == 1
    assert fc.BATCH_NWIN * fc.BATCH_N == F1 and fc.CHUNK % fc.BATCH_N != 0          # the boundary falls inside a window
    # every phase of the period starts a launch somewhere, over the launches of a call: at least the second launch starts off phase 0
    assert fc.CHUNK % K != 0 and (2 * fc.CHUNK) % K not in (0, fc.CHUNK % K)


def test_periodic_and_tile_round_trip():
    stack = np.arange(K * 6, dtype=np.uint8).reshape(K, 2, 3)
    for F in (K, 100, F1):
        big = fc.periodic(stack, F)
        assert big.shape == (F, 2, 3) and big.flags.c_contiguous
        assert all(np.array_equal(big[f], stack[f % K]) for f in (0, 1, K - 1, min(K, F - 1), F - 1))
        fc.assert_periodic(big, stack)
        assert np.array_equal(fc.tile(stack, F), big)
    recs = np.zeros(K, np.dtype([("a", "<i4"), ("b", "<u8")]))
    recs["a"] = np.arange(K)
    fc.assert_periodic(fc.tile(recs, 100), recs)
    with pytest.raises(AssertionError):
        fc.periodic(stack[:5], 10)


def test_distinct_outputs_are_required():
    stack = np.arange(K * 8, dtype=np.int32).reshape(K, 8)
    fc.assert_distinct(stack)
    fc.assert_outputs_tell_frames_apart(stack)
    twin = stack.copy()
    twin[20] = twin[3]
    with pytest.raises(AssertionError, match="3 and 20"):
        fc.assert_distinct(twin)
    with pytest.raises(AssertionError):
        fc.assert_outputs_tell_frames_apart(twin)
    # a count: 37 different values are not to be had, but the frame a stale launch would read must differ
    counts = (np.arange(K) % 5).astype(np.int32)
    fc.assert_outputs_tell_frames_apart(counts)
    stale_twin = (0 - fc.CHUNK) % K          # the distinct frame launch 1 would hand to distinct frame 0
    counts[stale_twin] = counts[0]
    with pytest.raises(AssertionError, match="stale twin"):
        fc.assert_outputs_tell_frames_apart(counts)


@pytest.mark.parametrize("F", [F1, F2])
def test_a_stale_f0_is_rejected(F):
    """the second launch reading the first launch's slice: right up to frame 32767, frame 0's results from 32768 on"""
    want = np.arange(K * 4, dtype=np.uint8).reshape(K, 4)
    stale = fc.stale_second_chunk(want, F)
    assert np.array_equal(stale[:fc.CHUNK], fc.tile(want, F)[:fc.CHUNK])
    with pytest.raises(AssertionError, match="first is frame 32768 .launch 1"):
        fc.assert_periodic(stale, want)
    # ... and only because the outputs differ: with two equal outputs at the boundary's phases it could pass
    assert fc.CHUNK % K != 0
    # one wrong byte in the last frame
    big = fc.tile(want, F)
    big[-1, 0] ^= 1
    with pytest.raises(AssertionError, match="1 of %d frames differ, the first is frame %d" % (F, F - 1)):
        fc.assert_periodic(big, want)


def test_sizing_rule():
    for name, (F, up, down) in fc.SIZES.items():
        assert F * up <= fc.MB64 and F * down <= fc.MB64, name
    assert F1 * 255 * 48 > 6 * fc.MB64          # why seg_cap is 4
    assert F1 * 256 * 17 * 8 > 1e9              # the device-only exception


# ------------------------------------------------------------------ the generators, on the CPU restatements
def test_stage_generators_give_distinct_outputs(orc):
    import shape_props_ref  # noqa: F401
    for H, W in [fc.SHAPE_ALIGNED, (9, 13)]:
        for mode in (0, 1):
            fc.assert_distinct(fc.orc_gray(orc, fc.bgr_frames(H, W), mode), "gray")
    for d in (7, 5):
        fc.assert_distinct(fc.orc_bilateral(orc, fc.gray_planes(9, 13), d), "bilateral")
    for H, W in fc.SHAPES_ODD:
        fc.assert_distinct(fc.orc_open(orc, fc.gray_planes(H, W, seed=1), (3, 3)), "open3x3")
    fc.assert_distinct(fc.orc_open(orc, fc.gray_planes(9, 13, seed=2), (4, 7)), "open (4, 7)")
    for cap in (fc.SEG_CAP, 1):
        segs, nseg = fc.orc_regionprops(orc, fc.label_planes(9, 13), cap)
        assert nseg.tolist() == list(range(1, K + 1))
        fc.assert_distinct(segs, "regionprops cap %d" % cap)
        fc.assert_outputs_tell_frames_apart(nseg, "nseg")
    shapes, nseg = fc.ref_shapes(fc.label_planes(9, 13, seed=1), fc.SEG_CAP)
    fc.assert_distinct(shapes, "shapes")
    assert nseg.tolist() == list(range(1, K + 1))
    for conn, order in [(8, 1), (4, 0)]:
        ncomp, lab = fc.orc_ccl(orc, fc.binary_planes(9, 13), conn, order)
        fc.assert_distinct(lab, "ccl")
        fc.assert_differs_across_launches(ncomp, "ncomp")
        assert ncomp.min() >= 1 and ncomp.max() >= 8


def test_stabilize_case_has_every_shift():
    import stabilize_ref
    frames, rect, anchor, moved = fc.stabilize_case()
    shifts, table, pixels = stabilize_ref.stabilize(frames, rect, fc.STAB_S, anchor)
    assert [(int(s["dy"]), int(s["dx"])) for s in shifts] == moved and len(set(moved)) == 25
    assert (table != stabilize_ref.EXCLUDED).all()
    for a in (shifts, table, pixels):
        fc.assert_distinct(a, "stabilize")


def test_committed_window_seeds_meet_the_conditions(orc):
    for (H, W), seed in fc.WINDOW_SEEDS.items():
        refs, with_segs, masked = fc.window_conditions(orc, fc.batch_windows(H, W, seed))
        assert 3 * with_segs >= K and masked == 0, (H, W, with_segs, masked)
        fc.assert_distinct(np.stack([r["gray"] for r in refs]), "window gray")
        # at the reference's lmbda the same windows leave nothing: why the batch tests raise it
        assert not any(orc.window(np.ascontiguousarray(w))["rpca"].any() for w in fc.batch_windows(H, W, seed)[:6])


# ------------------------------------------------------------------ the inventory
LAUNCHERS = ["launch_gray", "launch_bilateral", "launch_grey_open", "launch_open3x3", "launch_filter_fused", "launch_filter_fused_geom",
             "launch_ccl", "launch_regionprops", "launch_segment_shapes", "launch_stabilize", "launch_stabilize_subpel",
             "launch_yuv420_to_bgr", "launch_yuv_to_bgr", "launch_review", "launch_review_panels", "launch_gray_groups"]


def test_inventory_covers_every_frame_loop_and_window_grid():
    hits = fc.check_inventory()
    loops = [h for h in hits if h[0] == "loop"]
    assert sorted({h[2] for h in loops}) == sorted(LAUNCHERS)
    assert len(loops) == 18 and sum(1 for h in loops if h[2] == "launch_gray") == 3
    grids = [h for h in hits if h[0] == "grid"]
    # the window grids of the IALM: every pass family, the statistics, the integer Gram kernel, the slab sum, the sparse choice and
    # both (pixels, frames) scatters
    assert {(h[1], h[3]) for h in grids} >= {("ialm.hip", "b.nwin"), ("ialm_mfma.hip", "b.nwin"), ("ialm_mstate.hip", "b.nwin"),
                                            ("ialm_gram8.hip", "b.nwin"), ("ialm_small.hip", "b.nwin"), ("ialm.hip", "nwin"),
                                            ("groups.hip", "nwin")}
    assert len(grids) >= 9


def test_inventory_names_tests_that_exist():
    import os
    import re
    names = set(re.findall(r"^def (test_\w+)", open(os.path.join(os.path.dirname(__file__), "test_frame_chunks_gpu.py")).read(), re.M))
    for key, entry in fc.INVENTORY.items():
        if isinstance(entry, tuple):
            assert entry[0] == "none" and len(entry[1]) > 20, key
            continue
        assert entry.startswith(fc.GPU), key
        assert entry[len(fc.GPU):].split("[")[0] in names, (key, entry)


def test_a_new_launcher_without_an_entry_fails(tmp_path):
    src = tmp_path / "new.hip"
    src.write_text("void launch_new(hipStream_t s, int F)\n{\n    for (int f0 = 0; f0 < F; f0 += 32768) {\n    }\n"
                   "    hipLaunchKernelGGL(k_new, dim3(4, nwin), dim3(256), 0, s);\n}\n")
    hits = fc.sweep_sources(str(tmp_path))
    assert hits == [("loop", "new.hip", "launch_new", 1), ("grid", "new.hip", "launch_new", "nwin")]
    with pytest.raises(AssertionError, match="no test named"):
        fc.check_inventory(fc.sweep_sources() + hits)
