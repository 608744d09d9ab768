"""The host side of the history-independence tests (tests/history_cases.py; the GPU side is tests/test_history_independence_gpu.py).

  1. the slot table names every slot of enum Slot (csrc/swk_api.hip) and nothing else: a slot added later without a history case
     fails here;
  2. the geometry restated in history_cases.py is the sources';
  3. for every (dirtier, victim) pair, from the geometry alone: the dirtier's footprint in each shared slot covers the victim's --
     the stale bytes the GPU test relies on were really there;
  4. the groups calls through the library's own plan_batch (tests/history_plan_check.cpp, a program of its own);
  5. the victims' references, once, on the host."""
import os
import re
import subprocess

import numpy as np
import pytest

import history_cases as hc

ROOT = hc.ROOT


def _src(name):
    return open(os.path.join(hc.CSRC, name)).read()


# ------------------------------------------------------------------ 1. the slot table
def test_every_slot_has_a_history_case():
    names, sites = hc.parse_slots()
    assert len(names) >= 57 and names[0] == "SL_ROI"
    hc.check_slots(names, sites)
    text = _src("swk_api.hip")
    for s in names:          # (a slot the library reserves nowhere would need no case: none is)
        assert len(re.findall(r"\b%s\b" % s, text)) >= 2, "%s is named in enum Slot only" % s
    # every GPU test the table names exists
    gpu = open(os.path.join(ROOT, "tests", "test_history_independence_gpu.py")).read()
    for s, entry in hc.SLOTS.items():
        if isinstance(entry, hc.Filled):
            fn = entry.victim[len(hc.GPU):].split("[")[0]
            assert re.search(r"^def %s\(" % fn, gpu, re.M), "%s: no test %s" % (s, fn)


def test_a_slot_without_a_case_is_reported():
    names, sites = hc.parse_slots()
    table = dict(hc.SLOTS)
    del table["SL_GPART"]
    with pytest.raises(AssertionError, match="SL_GPART"):
        hc.check_slots(names, sites, table)
    with pytest.raises(AssertionError, match="SL_NEW"):
        hc.check_slots(names + ["SL_NEW"], sites, hc.SLOTS)
    with pytest.raises(AssertionError, match="does not have"):
        hc.check_slots(names[1:], sites, hc.SLOTS)


# ------------------------------------------------------------------ 2. the restated geometry is the sources'
def test_restated_geometry_matches_the_sources():
    api, mstate, ialm = _src("swk_api.hip"), _src("ialm_mstate.hip"), _src("ialm.hip")
    assert "int ialm_mstate_fpad(int n) { return (n + 3) & ~3; }" in mstate
    assert "int ialm_fpad(bool mstate, int n) { return mstate ? ialm_mstate_fpad(n) : (n + 15) & ~15; }" in api
    assert "int64_t ialm_pstride(int64_t P) { return (P + 127) & ~(int64_t)127; }" in api
    assert re.search(r"constexpr int kMaxN\s*=\s*64;", _src("swk_internal.h"))
    # plan_ialm's choice of the pass
    for line in ("if (variant == 0) variant = 4;", "if (variant >= 4 && variant != 6 && want_AE) variant = 2;", "if (n > kMaxN) variant = 6;",
                 "pl.mstate = variant == 4 || variant == 5;"):
        assert line in api, line
    # ialm_pass_nblk, statement by statement
    body = ialm[ialm.index("int ialm_pass_nblk("):ialm.index("void launch_ialm_stats(")]
    for line in ("if (variant >= 2 && variant != 6) {", "const int ntiles = (P + 15) / 16;", "int per_win = (256 * 2 * 3 + nwin - 1) / nwin;",
                 "const int cap = (ntiles + 7) / 8;", "if (per_win > 512) per_win = 512;", "const int ntiles = (P + 63) / 64;",
                 "int per_win = (256 * 8 + nwin - 1) / nwin;", "if (per_win < 4) per_win = 4;", "if (per_win > 128) per_win = 128;",
                 "if (per_win > ntiles) per_win = ntiles;"):
        assert line in body, line
    # the slot sizes of ialm_start
    for line in ("NEED(ctx, SL_A, felems * 8, b.A);", "NEED(ctx, SL_Y, felems * 8, b.Y);", "NEED(ctx, SL_SALT, elems, b.Salt);",
                 "NEED(ctx, SL_BM, (size_t)nwin * n * n * 8, b.Bm);", "NEED(ctx, SL_GPART, (size_t)nwin * b.nblk * n * n * 8, b.gpart);",
                 "NEED(ctx, SL_ZZPART, (size_t)2 * nwin * b.nblk * 8, b.zzpart);",
                 "const size_t felems = (size_t)nwin * b.fpad * b.pstride;"):
        assert line in api, line
    assert hc.ialm_geom(1, 21, 6144) == hc.IalmGeom(1, 21, 6144, 4, True, 24, 6144, 48)
    assert hc.ialm_geom(1, 21, 6144, want_AE=True)[3:] == (2, False, 32, 6144, 48)
    assert hc.ialm_geom(2, 70, 8970)[3:] == (6, False, 80, 9088, 128)


# ------------------------------------------------------------------ 3. footprints
def _victim_geoms(name):
    """the routes a victim runs on in the GPU test: (label, geometry, want_E)"""
    n, H, W = hc.victim_geometry(name)
    P = H * W
    out = [("mstate", hc.ialm_geom(1, n, P), False)]
    if name not in hc.WIDE_VICTIMS or name == "plain21":
        out += [("mfma_ae", hc.ialm_geom(1, n, P, 2, True), True), ("lds_ae", hc.ialm_geom(1, n, P, 1, True), True)]
    if name in hc.WIDE_VICTIMS:
        out.append(("wide", hc.ialm_geom(1, n, P, 6, True), True))
    return out


def _dirtier_geoms(dirtiers=hc.IALM_DIRTIERS):
    """every dirtier call of the GPU test's sequence: each dirtier with A / E not wanted, then wanted"""
    return [(d.name, hc.ialm_geom(d.nwin, d.n, d.H * d.W, 0, ae), ae) for d in dirtiers for ae in (False, True)]


def check_ialm_pair(victim, dirtiers=hc.IALM_DIRTIERS):
    """The footprint conditions of one victim against the dirtier sequence; returns the smallest covered share of a padded plane."""
    worst = 1.0
    dg = _dirtier_geoms(dirtiers)
    for label, v, want_E in _victim_geoms(victim):
        vb = hc.ialm_slot_bytes(v, want_E)
        for slot, need in vb.items():
            have = max(hc.ialm_slot_bytes(g, ae).get(slot, 0) for _, g, ae in dg)
            assert have >= need, "%s %s: the dirtiers leave %d bytes in %s, the victim uses %d" % (victim, label, have, slot, need)
        # fpad x pstride x nwin nests
        assert max(g.fpad * g.pstride * g.nwin for _, g, _ in dg) >= v.fpad * v.pstride * v.nwin
        # more windows, and a pixel count of another residue mod 16
        assert all(g.nwin > v.nwin for _, g, _ in dg)
        assert all(g.P % 16 != v.P % 16 for _, g, _ in dg)
        # the victim's padded planes and columns lie on bytes a dirtier wrote
        for slot in ("SL_A", "SL_Y") + (("SL_E",) if want_E else ()):
            eb = hc.plane_elem_bytes(slot, v)
            total, pad = hc.padding_granules(v, eb)
            if not pad.any():
                continue
            wrote = np.zeros(total, bool)
            for _, g, ae in dg:
                if slot == "SL_E" and not ae:
                    continue
                wrote |= hc.written_granules(g, hc.plane_elem_bytes(slot, g), total)
            per = eb // 2
            plane = v.pstride * per
            for w in range(v.nwin):
                for j in range(v.fpad):
                    a = (w * v.fpad + j) * plane
                    p = pad[a:a + plane]
                    if p.any():
                        share = float((wrote[a:a + plane] & p).sum()) / float(p.sum())
                        worst = min(worst, share)
                        # (what is not covered is the dirtiers' own padded columns: 58 of 9088 and 118 of 9088 elements)
                        assert share >= 0.98, "%s %s %s: plane %d of the victim is padding, %.1f %% of it was written by a dirtier" % (
                            victim, label, slot, j, 100 * share)
    return worst


@pytest.mark.parametrize("victim", hc.TRAJECTORY_VICTIMS + hc.SCENE_VICTIMS + ("wide70",))
def test_ialm_dirtiers_cover_the_victims_padding(victim):
    n, H, W = hc.victim_geometry(victim)
    _, mstate, _ = _victim_geoms(victim)[0]
    if victim in hc.SCENE_VICTIMS:
        assert (H * W) % 16 and (H * W) % 4 and mstate.pstride > mstate.P          # padded columns, no whole labeller word
    elif victim != "wide70":
        assert n % 4 and n % 16 and mstate.fpad > n                                # padded frames on every route
    worst = min(check_ialm_pair(victim), check_ialm_pair(victim, (hc.D64,)))          # the GPU test's two sequences: d64 and d70, d64 alone
    print("HISTORY %s: the least covered padded plane is %.2f %% stale" % (victim, 100 * worst))


def test_a_shrunk_dirtier_is_reported():
    """the same conditions with d64 and d70 cut to one window of 16 x 16: not enough bytes in SL_A for any victim"""
    small = tuple(d._replace(nwin=1, H=16, W=16) for d in hc.IALM_DIRTIERS)
    with pytest.raises(AssertionError, match="the dirtiers leave"):
        check_ialm_pair("plain21", small)
    # and with frames cut to 8: every slot is large enough for short5, but its padded planes 8..15 were never written
    few = (hc.D64._replace(n=8, nwin=40, H=70, W=129),)
    with pytest.raises(AssertionError, match="is padding"):
        check_ialm_pair("short5", few)


def test_dirtier_frames_are_saturated_checkerboards():
    for d in hc.IALM_DIRTIERS:
        f = hc.dirtier_frames(d)
        assert f.shape == (d.nwin * d.n, d.H, d.W) and d.H <= 70 and d.W <= 130
        assert (f[4] == 255).mean() > 0.97 and 0.4 < (f[0] == 255).mean() < 0.6
        assert set(np.unique(f)) == {0, 255}
        flat = f.reshape(len(f), -1)
        assert len({r.tobytes() for r in flat}) == len(flat)
        for w in range(d.nwin):
            assert f[w * d.n:(w + 1) * d.n].all(axis=(1, 2)).sum() == 0          # no frame is constant: none is a null frame
    assert hc.D64.n == 64 and hc.D70.n == 70


def test_plane_dirtiers_cover_their_victims():
    """the u8 planes of the other families nest: more bytes, and larger in H and in W, so that a victim is smaller in either direction"""
    for fam, (d, victims) in hc.PLANE_PAIRS.items():
        assert d.H <= 70 and d.W <= 130 and d.count <= 40, fam
        for v in victims:
            assert hc.plane_bytes(d) >= hc.plane_bytes(v), (fam, v)
            assert d.count >= v.count, "%s: a per-frame slot of the victim would be a new allocation" % fam
            assert d.H >= v.H and d.W >= v.W and (d.H > v.H or d.W > v.W), (fam, v)
            assert v.count <= 21 or fam == "filter_fused", (fam, v)
    fused = hc.PLANE_PAIRS["filter_fused"][1]
    d = hc.PLANE_PAIRS["filter_fused"][0]
    assert any(v.H == d.H and v.W < d.W for v in fused) and any(v.W == d.W and v.H < d.H for v in fused)
    (cd, Hd, Wd, Sd), (cv, Hv, Wv, Sv) = hc.STAB_DIRTIER, hc.STAB_VICTIM
    assert Sd == 16 and Sv < Sd and cv < cd <= 21 and Hv < Hd and Wv < Wd
    assert cd * (2 * Sd + 1) ** 2 >= cv * (2 * Sv + 1) ** 2
    assert hc.CROPS_DIRTIER[0] > hc.CROPS_VICTIM[0] and hc.CROPS_DIRTIER[1] > hc.CROPS_VICTIM[1]
    # the IALM dirtiers' u8 planes (X, S, the alternate S) cover every victim's
    for name in hc.TRAJECTORY_VICTIMS + hc.SCENE_VICTIMS:
        n, H, W = hc.victim_geometry(name)
        assert hc.D64.nwin * hc.D64.n * hc.D64.H * hc.D64.W >= n * H * W


# ------------------------------------------------------------------ 4. the groups calls through the library's own plan
@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("history") / "history_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", hc.CSRC,
                           os.path.join(ROOT, "tests", "history_plan_check.cpp"), os.path.join(hc.CSRC, "batch_plan.cpp"), "-o", exe])

    def run(groups):
        args = [str(hc.GROUPS_N)] + [str(v) for g in groups for v in g]
        out = subprocess.run([exe] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert out.returncode == 0, out.stdout
        lines = out.stdout.strip().splitlines()
        head = dict(zip(lines[0].split()[0::2], (int(v) for v in lines[0].split()[1::2])))
        rows = [dict(zip(ln.split()[2::2], (int(v) for v in ln.split()[3::2]))) for ln in lines[1:]]
        return head, rows
    return run


def test_groups_victim_is_padded_and_its_dirtier_covers_it(plan):
    head, rows = plan(hc.GROUPS_VICTIM)
    assert head["subs"] == 2
    tiny, scene, small = rows
    assert tiny["P"] < hc.GROUPS_N and tiny["sub"] == 1 and tiny["pitch"] == tiny["P"]          # a sub-batch of its own, at its true P
    assert scene["sub"] == small["sub"] == 0 and scene["pitch"] == scene["P"]
    assert small["pitch"] == scene["P"] > small["P"]                                            # padded to the larger ROI's pitch
    assert head["vec"] == 2 and scene["P"] % 4 == 2
    dhead, drows = plan(hc.GROUPS_DIRTIER)
    assert dhead["subs"] == 1 and drows[0]["pitch"] == drows[0]["P"] == 70 * 129
    assert dhead["total"] >= head["total"], "the dense call's stage planes cover the groups call's"
    # the padding pixels of the small group's X planes (which the IALM reads and batch_plan.h promises are zero) lie inside what the
    # dense call wrote: every byte of its planes is a pixel
    assert small["goff"] + 21 * small["pitch"] <= dhead["total"]
    # a groups dirtier for the descriptor tables: more windows than the single-group victim that follows it
    vhead, _ = plan(hc.GROUPS_SINGLE_VICTIM)
    assert vhead["subs"] == 1 and head["tab"] > 0 and vhead["total"] <= dhead["total"]


# ------------------------------------------------------------------ 5. the victims' references
def test_trajectory_victims_are_the_proven_windows():
    """(tests/test_ialm_trajectory_cpu.py proves the windows and their trajectories; here: the victims are among them, stop by the
    tolerance at the K the table gives, and the null and duplicated frames are where the table says)"""
    import ialm_trajectory_cases as tc
    for name in hc.TRAJECTORY_VICTIMS + ("wide70",):
        case = tc.CASES[name]
        assert tc.steps(name) == case.K < 100
        x = tc.planes(name)
        assert x.shape == (case.n, case.Hc * case.Wc)
        assert not x[:case.null].any() and x[case.null:].any(axis=1).all()
        if case.dup is not None:
            assert np.array_equal(x[case.dup], x[case.dup + 1])
        last = tc.reference(name)[-1]
        assert last.ratio < 1e-3 and not last.A[:, :case.null].any() and not last.E[:, :case.null].any()


@pytest.mark.parametrize("name", hc.SCENE_VICTIMS)
def test_scene_victims_have_something_in_every_stage(name):
    """the oracle's window of a scene: segments on several frames (a stale record or label would show), its loop restated with the
    iterates kept stops at the same iteration with the same sparse image, and few elements of E lie at a byte boundary"""
    import ialm_trajectory_cases as tc
    from oracle import reference_path as orc
    ref = hc.scene_oracle(name)
    n, H, W = hc.victim_geometry(name)
    assert ref["opened"].shape == (n, H, W)
    assert sum(1 for s in ref["segments"] if len(s)) >= 3 and ref["labels"].max() >= 30
    tr = hc.scene_trajectory(name)
    assert len(tr) == int(ref["iters"])
    np.testing.assert_array_equal(orc.rpca_epilogue(tr[-1].E).T.reshape(n, H, W), ref["rpca"])
    assert tc.boundary_mask(tr[-1].E, tc.BAND).mean() <= tc.MASK_CAP


def test_small_plane_references_agree_with_scipy():
    """the restatements the stage-level victims are held to, on the victims' own planes (the _cpu twins of the reused modules hold
    them on theirs)"""
    from scipy import ndimage
    import frame_chunks as fc
    from oracle import reference_path as orc
    planes = fc.gray_planes(9, 13, seed=2)[:21]
    for p in planes[:5]:
        assert np.array_equal(orc.grey_open_u8(p, (4, 7)), ndimage.grey_opening(p, size=(4, 7)))
    masks = fc.binary_planes(9, 13)[:21]
    for m in masks[:5]:
        n8, lab = orc.ccl_u8(m, 8, 0)
        assert n8 == ndimage.label(m, np.ones((3, 3)))[1] and np.array_equal(lab != 0, m != 0)
    labels = fc.label_planes(9, 13)[:21]
    segs, nseg = fc.orc_regionprops(orc, labels, 255)
    assert nseg.tolist() == list(range(1, 22))
    for k in (0, 20):
        rr, cc = np.nonzero(labels[k] == 1)
        assert (int(segs[k, 0]["area"]), int(segs[k, 0]["sum_r"]), int(segs[k, 0]["sum_c"])) == (rr.size, rr.sum(), cc.sum())
