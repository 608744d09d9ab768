"""tests/ialm_start_cases.py checked on the host, so that tests/test_ialm_start_gpu.py cannot silently test nothing: the builders
give the shapes, alignments and contents they promise, the references agree with each other, the windows next to the switch
between the two starts lie on their intended sides, and every window labelled clipped clips."""
import numpy as np

import ialm_start_cases as cases
from ialm_start_cases import LMBDA, LMBDA_ALL


def _windows(lmbda=LMBDA):
    for shape in cases.SHAPES:
        for case in cases.shape_cases(shape):
            for w in range(case.x.shape[0]):
                yield shape, case, w, cases.window_ref((case.name, w), case.x[w], lmbda)


def test_covering_subset():
    shapes = cases.SHAPES
    assert len(set(shapes)) == len(shapes)
    assert {n for n, _, _ in shapes} == set(cases.N_LIST)
    assert {P for _, P, _ in shapes} == set(cases.P_LIST) | set(cases.EXTRA_P)
    assert {P % 4 for P in cases.P_LIST} == {0, 1, 2, 3} and any(P % 16 == 0 for P in cases.P_LIST)
    for P in cases.P_LIST + cases.EXTRA_P:                      # every pixel count with 21 and with 64 frames
        assert {n for n, p, _ in shapes if p == P} >= {21, 64}
    for n in cases.N_LIST:                                      # every frame count with the 16-byte loads and with the dword loads
        assert any(p % 16 == 0 for m, p, _ in shapes if m == n), n
        assert any(p % 16 != 0 for m, p, _ in shapes if m == n), n
    assert {nwin for _, _, nwin in shapes} == {1, 3, 4}
    # batches of windows of an odd number of bytes: windows start at every byte offset of a dword, under several frame-block counts
    offsets = {}
    for n, P, nwin in shapes:
        if nwin > 1 and (n * P) % 2:
            offsets.setdefault((n + 15) // 16, set()).update((w * n * P) % 4 for w in range(nwin))
    assert all(v == {0, 1, 2, 3} for v in offsets.values()) and set(offsets) == {1, 2, 3, 4}, offsets
    assert max(n * P * nwin for n, P, nwin in shapes) == 64 * 107 * 214 * 3
    assert (64, 107 * 214, 3) in shapes
    # frame counts on both sides of 16, 32 and 48 among the batches whose windows start off a dword boundary
    odd = {n for n, P, nwin in shapes if nwin > 1 and (n * P) % 2}
    assert odd >= {15, 17, 31, 33, 49, 63}


def test_contents_are_what_they_say():
    for shape in cases.SHAPES:
        n, P, nwin = shape
        batch = cases.shape_cases(shape)
        assert [c.name.rsplit("_", 1)[1] for c in batch] == list(cases.CONTENTS)
        for ci, case in enumerate(batch):
            assert case.x.shape == (nwin, n, P) and case.x.dtype == np.uint8 and case.x.flags["C_CONTIGUOUS"]
            for w in range(nwin):
                x, content = case.x[w], cases.CONTENTS[(ci + w) % len(cases.CONTENTS)]
                assert x.any(), (case.name, w)                   # no window is done before it starts
                if content == "one":
                    assert x.sum() == 1 and x.max() == 1
                elif content == "all255":
                    assert x.min() == 255
                elif content == "alt":
                    assert (x[0::2] == 255).all() and not x[1::2].any()
                elif content == "last255":
                    assert x.sum() == 255 and x[-1, -1] == 255
                elif content == "rowend255":
                    assert x.sum() == 255 * n and (x[:, -1] == 255).all()
                elif content == "tail37":
                    tail = min(cases.PAD_TAIL, P - 1)
                    assert not x[:, P - tail:].any() and x[:, :P - tail].all()
                else:
                    assert content == "random" and (len(np.unique(x)) > 1 or x.size < 4)
    for n, P in cases.NEIGHBOUR_SHAPES:
        a, b = cases.neighbour_cases(n, P)
        assert (a.x[1] == 255).all() and (b.x[0] == 255).all() and np.array_equal(a.x[0], b.x[1]) and len(np.unique(a.x[0])) > 1
    assert {P % 16 == 0 for _, P in cases.NEIGHBOUR_SHAPES} == {True, False}


def test_integer_reference_against_plain_integers():
    rng = np.random.default_rng(3)
    for n, P in ((1, 1), (17, 65), (64, 1021)):
        x = rng.integers(0, 256, size=(n, P), dtype=np.uint8)
        x[0, 0] = 255
        g, sumsq, maxv = cases.int_ref(x)
        xi = x.astype(np.int64)
        want = np.einsum("ip,jp->ij", xi, xi)
        assert g.dtype == np.int64 and np.array_equal(g, want) and sumsq == int((xi * xi).sum()) and maxv == 255


def test_both_lambdas_split_the_windows_as_intended():
    """lmbda = 0.01: both starts occur among the shapes, and no window sits closer to the switch than rounding could decide;
    lmbda = 4: every window starts from integers."""
    integer = clipped = 0
    for shape, case, w, ref in _windows(LMBDA):
        assert abs(ref["margin"]) >= cases.MIN_MARGIN, (case.name, w)
        assert ref["integer"] == (ref["margin"] <= 0), (case.name, w)
        integer += ref["integer"]
        clipped += not ref["integer"]
    assert integer >= 20 and clipped >= 100
    for shape, case, w, ref in _windows(LMBDA_ALL):
        assert ref["integer"] and ref["margin"] <= -cases.MIN_MARGIN, (case.name, w)


def test_windows_labelled_clipped_clip():
    """... in the float64 restatement: its E_1 has a nonzero element exactly where the start choice says so."""
    for shape, case, w, ref in _windows(LMBDA):
        if not ref["integer"]:
            assert ref["clipped"], (case.name, w)
            assert ref["Gabs"].shape == ref["Gld"].shape == ref["G"].shape and ref["Gld"].dtype == np.longdouble
    seen = 0
    for shape in cases.SHAPES[::5]:
        x = cases.shape_cases(shape)[3].x[0]
        for lmbda in (LMBDA, LMBDA_ALL):
            assert cases.float_start(x, lmbda)["clipped"] == (not cases.expected_integer_start(x, lmbda))
            seen += 1
    assert seen >= 10
    for case, clipped in cases.clipped_cases():
        assert len(clipped) == case.x.shape[0]
        for w, c in enumerate(clipped):
            ref = cases.window_ref((case.name, w), case.x[w])
            assert ref["integer"] == (not c) and abs(ref["margin"]) >= cases.MIN_MARGIN
            if c:
                assert ref["clipped"]
    assert cases.toy_window().shape == (7, 256) and cases.dark_window().max() == 255


def test_unclipped_start_is_c_times_x():
    """Where the first shrinkage removes nothing the restatement, run in long double, gives M_1^T M_1 = c^2 X^T X with
    c = 1 + 1 / (mu_0 dual) to 1e-17 relative: the closed form the integer start (gram_reduce's scale) and the GPU test's bound for
    the f64 start pass rest on."""
    assert np.finfo(np.longdouble).eps < 2e-19
    done = 0
    for lmbda, picks in ((LMBDA, ((21, 107 * 214, 1), (64, 4096, 1))), (LMBDA_ALL, ((17, 1021, 4), (33, 63, 3), (1, 16, 1), (21, 1, 4)))):
        for shape in picks:
            for case in cases.shape_cases(shape)[1:5]:
                x = case.x[0]
                if not cases.expected_integer_start(x, lmbda):
                    continue
                fs = cases.float_start(x, lmbda, dtype=np.longdouble)
                assert not fs["clipped"]
                got = cases.gram_ld(fs["M"])
                want = cases.scale_c2(fs["dual"], fs["mu"]) * cases.int_ref(x)[0].astype(np.longdouble)
                assert (np.abs(got - want) <= np.longdouble(1e-17) * want).all(), case.name
                # ... and the float64 scalars the GPU test scales by differ from these by roundings of 1e-16 of c - 1 < 1
                ref = cases.window_ref((case.name, 0), x, lmbda)
                assert abs(float(ref["c2"] / cases.scale_c2(fs["dual"], fs["mu"])) - 1) < 1e-15
                done += 1
    assert done >= 12


def test_boundary_windows_lie_on_their_sides():
    for (n, P, v, raised, integer), case in zip(cases.BOUNDARY, cases.boundary_cases()):
        x = case.x[0]
        assert x.shape == (n, P) and int(x.max()) == (255 if raised else v) and int((x != v).sum()) == int(raised)
        m = cases.start_margin(x)
        assert abs(m) >= cases.MIN_MARGIN and (m <= 0) == integer == bool(cases.expected_integer_start(x)), (n, P, m)
        assert cases.float_start(x)["clipped"] == (not integer)
    # the closest sizes on either side of the switch that leave the margin: the exact tie 15 x 3375 is none of them
    assert abs(cases.margin_from_stats(255 * 255 * 50625, 255)) < cases.MIN_MARGIN
    for v, raised, rows in ((255, False, cases.BOUNDARY[0:2]), (254, True, cases.BOUNDARY[4:6])):
        assert cases.closest_boundary_sizes(v, raised) == tuple(n * P for n, P, _, _, _ in rows)
        assert [r[2:4] for r in rows] == [(v, raised)] * 2
    margins = [abs(cases.start_margin(c.x[0])) for c in cases.boundary_cases()]
    assert max(margins) < 2e-4 and min(margins) > 1e-6
