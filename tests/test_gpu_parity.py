"""GPU parity tests: the HIP path (through the C ABI, swiftwatcher_amd/_lib.py) against the CPU
oracle on the same seeded inputs, against the committed golden fixtures, and -- at full
benchmark size -- through size-independent properties.  Integer/byte/index results must be
bit-exact; float64 RPCA factors within 1e-5 (BASELINE.json north_star)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ATOL_AE = 1e-5


@pytest.fixture(scope="module", params=[(0, 0), (2, 0), (1, 1), (2, 1)],
                ids=["auto_pass+newton_schulz", "mfma_pass+newton_schulz", "lds_pass+jacobi", "mfma_pass+jacobi"])
def ctx(request):
    """Every test runs against the IALM pass kernels (0 = auto: the M-state MFMA pass, or the A/Y-state one when
    A / E are requested; 2 = A/Y-state MFMA pass; 1 = LDS/VALU) and both G^(-1/2) solvers (0 = Newton-Schulz on
    MFMA, the default; 1 = cyclic Jacobi)."""
    from swiftwatcher_amd import _lib
    c = _lib.Context(0)
    c.set_ialm_variant(request.param[0])
    c.set_eig_method(request.param[1])
    yield c
    c.close()


@pytest.fixture(scope="module")
def orc():
    from oracle import reference_path
    return reference_path


def _segs(res, i):
    return [(int(s["label"]), int(s["r0"]), int(s["c0"]), int(s["r1"]), int(s["c1"]), int(s["area"]),
             int(s["sum_r"]), int(s["sum_c"])) for s in res["segs"][i, :res["nseg"][i]]]


def _orc_segs(seglist):
    return [(s["label"],) + s["bbox"] + (s["area"], s["sum_r"], s["sum_c"]) for s in seglist]


# ------------------------------------------------------------------ stage level
def test_bgr2gray(ctx, orc):
    rng = np.random.default_rng(1)
    img = rng.integers(0, 256, size=(3, 37, 61, 3), dtype=np.uint8)
    for mode in (0, 1):
        got = ctx.bgr2gray(img, mode)
        for i in range(3):
            np.testing.assert_array_equal(got[i], orc.bgr2gray(img[i], mode))


def test_rpca_epilogue(ctx, orc):
    rng = np.random.default_rng(2)
    E = rng.normal(0, 80, size=5000)
    E[:8] = [0.0, -0.0, -0.999999, -1.0, -255.0, -255.5, -300.0, 12.0]
    np.testing.assert_array_equal(ctx.rpca_epilogue(E), orc.rpca_epilogue(E))


@pytest.mark.parametrize("shape", [(12, 13), (64, 96), (107, 214), (33, 65)])
@pytest.mark.parametrize("fma", [False, True])
def test_bilateral(ctx, orc, shape, fma):
    rng = np.random.default_rng(3)
    sparse = (rng.random((3,) + shape) < 0.15) * rng.integers(1, 256, size=(3,) + shape)
    dense = rng.integers(0, 256, size=(1,) + shape)
    imgs = np.concatenate([sparse, dense]).astype(np.uint8)
    got = ctx.bilateral_u8(imgs, 7, 15.0, 1.0, fma)
    for i in range(imgs.shape[0]):
        np.testing.assert_array_equal(got[i], orc.bilateral_u8(imgs[i], 7, 15.0, 1.0, fma))
    # other diameters through the generic kernel
    got5 = ctx.bilateral_u8(imgs[0], 5, 20.0, 2.0, fma)
    np.testing.assert_array_equal(got5, orc.bilateral_u8(imgs[0], 5, 20.0, 2.0, fma))


def test_thresh(ctx, orc):
    src = np.arange(256, dtype=np.uint8).repeat(3)
    np.testing.assert_array_equal(ctx.thresh_tozero_u8(src, 15), orc.thresh_tozero_u8(src, 15))
    np.testing.assert_array_equal(ctx.thresh_tozero_u8(src, 200), orc.thresh_tozero_u8(src, 200))


def test_grey_opening_golden_and_random(ctx, orc, golden_dir):
    g = np.load(os.path.join(golden_dir, "grey_opening.npz"))
    for i in range(int(g["count"])):
        np.testing.assert_array_equal(ctx.grey_open3x3_u8(g["in%d" % i]), g["out%d" % i])
    rng = np.random.default_rng(4)
    for shape in [(212, 424), (31, 33), (32, 64), (33, 65), (2, 2)]:
        im = rng.integers(0, 256, size=shape, dtype=np.uint8)
        np.testing.assert_array_equal(ctx.grey_open3x3_u8(im), orc.grey_open_u8(im))


def test_grey_opening_with_other_windows(ctx, orc, golden_dir):
    """grayscale_opening(frame, SE) takes any SE in the reference (image_filtering.py:319-322); the loop only asks for (3, 3).  The general
    kernel against fixtures made by the reference's own function (scipy: odd, even, rectangular and 1-wide windows, an image smaller
    than the window) and against the oracle on random images; (3, 3) through it equals the tiled kernel."""
    from swiftwatcher_amd import image_filtering as img
    g = np.load(os.path.join(golden_dir, "grey_opening_windows.npz"))
    for i in range(int(g["count"])):
        for kh, kw in g["sizes"]:
            np.testing.assert_array_equal(ctx.grey_open_u8(g["in%d" % i], (kh, kw)), g["out%d_%dx%d" % (i, kh, kw)], err_msg="%d %dx%d" % (i, kh, kw))
    rng = np.random.default_rng(44)
    for shape, size in [((212, 424), (5, 5)), ((33, 65), (4, 7)), ((64, 64), (11, 2)), ((3, 3), (5, 5)), ((50, 70), (3, 3))]:
        im = rng.integers(0, 256, size=shape, dtype=np.uint8)
        np.testing.assert_array_equal(ctx.grey_open_u8(im, size), orc.grey_open_u8(im, size), err_msg=str(size))
    im = rng.integers(0, 256, size=(90, 130), dtype=np.uint8)
    np.testing.assert_array_equal(ctx.grey_open_u8(im, (3, 3)), ctx.grey_open3x3_u8(im))
    np.testing.assert_array_equal(img.grayscale_opening(im, (5, 3)), orc.grey_open_u8(im, (5, 3)))


def test_resize_frame(ctx, orc):
    """resize_frame (image_filtering.py:206-212: cv2.resize, INTER_LINEAR; dead code in the reference, PARITY UNPINNED): the kernel against
    the C restatement of OpenCV 4.1.0's 8-bit arithmetic -- down, up, one axis only, grey and BGR -- and two properties the arithmetic
    has whatever the rounding: a constant image stays constant, the same size is the identity."""
    from swiftwatcher_amd import image_filtering as img
    rng = np.random.default_rng(45)
    for shape, dsize in [((212, 424, 3), (300, 150)), ((107, 214), (300, 150)), ((40, 60, 3), (60, 40)), ((40, 60, 3), (121, 77)),
                         ((5, 7), (3, 2)), ((33, 65, 3), (65, 20))]:
        im = rng.integers(0, 256, size=shape, dtype=np.uint8)
        got = img.resize_frame(im, dsize)
        assert got.shape[:2] == (dsize[1], dsize[0])
        np.testing.assert_array_equal(got, orc.resize_linear_u8(im, dsize), err_msg=str((shape, dsize)))
    flat = np.full((37, 53, 3), 171, np.uint8)
    assert (ctx.resize_linear_u8(flat, (300, 150)) == 171).all()
    im = rng.integers(0, 256, size=(37, 53, 3), dtype=np.uint8)
    np.testing.assert_array_equal(ctx.resize_linear_u8(im, (53, 37)), im)


@pytest.mark.parametrize("conn,order", [(8, 1), (8, 0), (4, 0), (4, 1)])
def test_ccl(ctx, orc, conn, order):
    rng = np.random.default_rng(5)
    cases = [((31, 45), 0.45), ((64, 64), 0.6), ((5, 9), 0.5), ((212, 424), 0.08), ((107, 213), 0.3),
             ((16, 16), 0.0), ((16, 16), 1.0), ((1, 40), 0.5), ((40, 1), 0.5)]
    for shape, dens in cases:
        im = ((rng.random(shape) < dens) * rng.integers(1, 256, size=shape)).astype(np.uint8)
        n, lab = ctx.ccl_u8(im, conn, order)
        nref, ref = orc.ccl_u8(im, conn, order)
        assert n == nref
        np.testing.assert_array_equal(lab, ref)
    # spiral / comb shapes stress long union chains
    comb = np.zeros((64, 128), np.uint8)
    comb[::2, :] = 9
    comb[:, 0] = 9
    n, lab = ctx.ccl_u8(comb, conn, order)
    nref, ref = orc.ccl_u8(comb, conn, order)
    assert n == nref == 1
    np.testing.assert_array_equal(lab, ref)


def test_ccl_large_frame_multi_kernel_path(ctx, orc):
    """Frames too large for the one-workgroup-per-frame kernel's LDS bitmap take the multi-kernel path."""
    rng = np.random.default_rng(8)
    im = ((rng.random((800, 808)) < 0.3) * 255).astype(np.uint8)
    n, lab = ctx.ccl_u8(im, 8, 1)
    nref, ref = orc.ccl_u8(im, 8, 1)
    assert n == nref
    np.testing.assert_array_equal(lab, ref)


def test_ccl_batch_more_than_255_components(ctx, orc):
    rng = np.random.default_rng(6)
    ims = ((rng.random((4, 80, 120)) < 0.2) * 200).astype(np.uint8)
    nc, lab = ctx.ccl_u8(ims, 8, 1)
    for i in range(4):
        nref, ref = orc.ccl_u8(ims[i], 8, 1)
        assert nc[i] == nref and nref > 255
        np.testing.assert_array_equal(lab[i], ref)


def test_regionprops_golden_and_wrap(ctx, orc, golden_dir):
    g = np.load(os.path.join(golden_dir, "regionprops.npz"))
    for i in range(int(g["count"])):
        segs, n = ctx.regionprops_u8(g["lab%d" % i])
        assert n == len(g["labels%d" % i])
        assert [int(s["label"]) for s in segs] == list(g["labels%d" % i])
        assert [(int(s["r0"]), int(s["c0"]), int(s["r1"]), int(s["c1"])) for s in segs] == [tuple(b) for b in g["bbox%d" % i]]
        cen = np.array([(int(s["sum_r"]) / int(s["area"]), int(s["sum_c"]) / int(s["area"])) for s in segs])
        np.testing.assert_array_equal(cen, g["centroid%d" % i])
    rng = np.random.default_rng(7)
    lab = rng.integers(0, 256, size=(3, 90, 130)).astype(np.uint8)
    segs, nseg = ctx.regionprops_u8(lab)
    for i in range(3):
        exp = orc.regionprops_u8(lab[i])
        assert nseg[i] == len(exp) == 255
        got = [(int(s["label"]), int(s["r0"]), int(s["c0"]), int(s["r1"]), int(s["c1"]), int(s["area"]), int(s["sum_r"]), int(s["sum_c"]))
               for s in segs[i, :nseg[i]]]
        assert got == _orc_segs(exp)


# ------------------------------------------------------------------ IALM
# Few pixels per frame against a queue of 64 (ialm_40x48x64: 1,920 pixels; ialm_47x94x64[_quiet]: config 1's ROI with FrameQueue(queue_size=64);
# ialm_30x40x64: 1,200 pixels, and its first shrinkage clips): cond(M_1)^2 enters the Gram-matrix route in the iteration where 1/mu is
# largest, and 23-25 iterations carry that error to the end (the quiet window: 2-3e-5 with the Jacobi solver).  Those windows get their
# first iteration from a double-double Cholesky factor (csrc/ialm_refine.hip) and meet the SAME bound as every other fixture.
@pytest.mark.parametrize("name,atol", [("ialm_128x160x7", ATOL_AE), ("ialm_64x96x21", ATOL_AE),
                                       ("ialm_64x96x64", ATOL_AE), ("ialm_107x214x21", ATOL_AE),
                                       ("ialm_40x48x64", ATOL_AE), ("ialm_47x94x64", ATOL_AE), ("ialm_47x94x64_quiet", ATOL_AE),
                                       ("ialm_30x40x64", ATOL_AE)])
def test_ialm_golden(ctx, orc, golden_dir, name, atol):
    """HIP IALM against fixtures produced by the reference's own function."""
    g = np.load(os.path.join(golden_dir, name + ".npz"))
    frames = g["frames"]
    n, H, W = frames.shape
    A, E, iters = ctx.ialm(frames.reshape(n, H * W))
    assert iters == int(g["iters"])
    rows = g["rows"]
    np.testing.assert_allclose(A[rows], g["A_rows"], atol=atol, rtol=0)
    np.testing.assert_allclose(E[rows], g["E_rows"], atol=atol, rtol=0)
    np.testing.assert_allclose(A.sum(axis=0), g["A_colsum"], rtol=1e-8)
    np.testing.assert_array_equal(ctx.rpca_epilogue(E).T.reshape(n, H, W), g["sparse"])


def test_accurate_first_iteration_of_ill_conditioned_windows(golden_dir):
    """The reference-made windows of 64 frames on config 1's ROI: with the accurate first iteration (the default) A and E land within
    1e-6 of the reference's SVD route with EITHER small-matrix solver; the counter says the window took it; switched off, the quiet
    window misses 1e-5 with the Jacobi solver -- the refinement is what the bound rests on, not luck of one solver.  The window whose
    first shrinkage clips (no integer start: double-double Gram matrix from the pixels) is refined too."""
    from swiftwatcher_amd import _lib
    c = _lib.Context(0)
    worst_off = 0.0
    for name in ("ialm_47x94x64_quiet", "ialm_47x94x64", "ialm_40x48x64", "ialm_30x40x64"):
        g = np.load(os.path.join(golden_dir, name + ".npz"))
        frames = g["frames"]
        n, H, W = frames.shape
        rows = g["rows"]
        for method in (0, 1):
            c.set_eig_method(method)
            c.set_start_refine(1e-5)
            before = c.refined_windows
            A, E, iters = c.ialm(frames.reshape(n, H * W))
            after = c.refined_windows
            assert (after[0] - before[0], after[1] - before[1]) == (1, 0), name
            assert iters == int(g["iters"])
            assert np.abs(A[rows] - g["A_rows"]).max() < 1e-6 and np.abs(E[rows] - g["E_rows"]).max() < 1e-6, name
            np.testing.assert_array_equal(c.rpca_epilogue(E).T.reshape(n, H, W), g["sparse"])
            if name == "ialm_47x94x64_quiet":
                c.set_start_refine(0.0)
                A0, E0, _ = c.ialm(frames.reshape(n, H * W))
                assert c.refined_windows == after
                worst_off = max(worst_off, np.abs(A0[rows] - g["A_rows"]).max(), np.abs(E0[rows] - g["E_rows"]).max())
    assert worst_off > 1e-5
    # the refinement forced (tau = 1e-12) on well-conditioned fixtures of 7, 21 and 64 frames, from the integer start and -- integer start
    # off, or a window whose first shrinkage clips (47x94x21) -- from the double-double Gram matrix of the pixels: every staging-tile
    # width of the kernel (16, 32, 64 pixels per chunk); results stay the reference's
    c.set_start_refine(1e-12)
    for name in ("ialm_128x160x7", "ialm_64x96x21", "ialm_47x94x21", "ialm_64x96x64"):
        g = np.load(os.path.join(golden_dir, name + ".npz"))
        frames = g["frames"]
        n, H, W = frames.shape
        for int_start in (1, 0):
            c.set_integer_start(int_start)
            before = c.refined_windows
            A, E, iters = c.ialm(frames.reshape(n, H * W))
            assert c.refined_windows[0] - before[0] == 1, (name, int_start)
            assert iters == int(g["iters"]), (name, int_start)
            assert np.abs(A[g["rows"]] - g["A_rows"]).max() < 1e-6 and np.abs(E[g["rows"]] - g["E_rows"]).max() < 1e-6, (name, int_start)
    c.set_integer_start(1)
    # a window of the 21-frame CLI queue at config 1's size is well enough conditioned: not touched
    g = np.load(os.path.join(golden_dir, "ialm_47x94x21.npz"))
    c.set_start_refine(1e-5)
    before = c.refined_windows
    c.ialm(g["frames"].reshape(21, -1))
    assert c.refined_windows == before
    c.close()


@pytest.mark.parametrize("name", ["ialm_128x160x7", "ialm_64x96x21", "ialm_64x96x64", "ialm_107x214x21", "ialm_40x48x64", "ialm_47x94x64",
                                  "ialm_47x94x64_quiet", "ialm_30x40x64"])
def test_sparse_image_golden_without_float_outputs(ctx, golden_dir, name):
    """The hot path asks for neither A nor E: the default (M-state) pass must still deliver the reference's
    sparse u8 image and iteration count bit for bit."""
    g = np.load(os.path.join(golden_dir, name + ".npz"))
    frames = g["frames"]
    n = frames.shape[0]
    res = ctx.batch_run(frames, 1, n, stages=("gray", "rpca"))
    assert int(res["iters"][0]) == int(g["iters"])
    np.testing.assert_array_equal(res["gray"], frames)
    np.testing.assert_array_equal(res["rpca"], g["sparse"])


def test_pass_kernels_agree_at_full_size():
    """424x212 x 64 frames, four windows with different content: the M-state pass (21 B/element) and the
    A/Y-state pass (34 B/element) give the same iteration counts, sparse images, labels and regions."""
    from swiftwatcher_amd import _lib, synthetic
    roi = np.concatenate([synthetic.roi_window(70 + w, 64, 212, 424, birds=4 + 5 * w) for w in range(4)])
    out = []
    for variant in (0, 2):
        c = _lib.Context(0)
        c.set_ialm_variant(variant)
        out.append(c.batch_run(roi, 4, 64, stages=("rpca", "opened", "labels")))
        c.close()
    a, b = out
    np.testing.assert_array_equal(a["iters"], b["iters"])
    assert len(set(int(i) & 1 for i in a["iters"])) >= 1
    for key in ("rpca", "opened", "labels", "nseg"):
        np.testing.assert_array_equal(a[key], b[key], err_msg=key)
    assert a["segs"].tobytes() == b["segs"].tobytes()


@pytest.mark.parametrize("n,Hc,Wc", [(1, 300, 400), (2, 240, 320), (3, 200, 256), (17, 96, 128), (33, 64, 96), (49, 64, 80)])
def test_window_sizes_between_the_mfma_block_counts(ctx, orc, n, Hc, Wc):
    """Frames per window that are not multiples of 16 (padded MFMA blocks, 1..4 of them), down to a single frame."""
    from swiftwatcher_amd import synthetic
    roi = synthetic.roi_window(500 + n, n, Hc, Wc, birds=3, bird_len=(10, 16), bird_wid=(4, 8))
    res = ctx.batch_run(roi, 1, n)
    ref = orc.window(roi)
    gray = np.stack([orc.bgr2gray(f) for f in roi]).reshape(n, -1).T
    assert int(res["iters"][0]) == orc.ialm(gray, return_iters=True)[2]
    for key in ("gray", "rpca", "opened", "labels"):
        np.testing.assert_array_equal(res[key], ref[key], err_msg=key)
    for i in range(n):
        assert _segs(res, i) == _orc_segs(ref["segments"][i])


def test_integer_start_matches_f64_start():
    """First Gram matrix from the i8 matrix cores (exact X^T X, scaled) against the f64 start pass: same iteration
    counts, sparse images and regions; a toy window whose first shrinkage is active must fall back by itself."""
    from swiftwatcher_amd import _lib, synthetic
    roi = np.concatenate([synthetic.roi_window(90 + w, 64, 212, 424, birds=3 + 4 * w) for w in range(2)] +
                         [synthetic.roi_window(95, 64, 212, 424, birds=5, null_frames=3)])
    out = []
    for on in (1, 0):
        c = _lib.Context(0)
        c.set_integer_start(on)
        out.append(c.batch_run(roi, 3, 64, stages=("rpca", "labels")))
        small = synthetic.roi_window(7, 7, 16, 16, birds=1, bird_len=(4, 6), bird_wid=(2, 3))     # lmbda / mu_0 < max(X)
        out.append(c.batch_run(small, 1, 7, stages=("rpca",)))
        c.close()
    for a, b in ((out[0], out[2]), (out[1], out[3])):
        np.testing.assert_array_equal(a["iters"], b["iters"])
        np.testing.assert_array_equal(a["rpca"], b["rpca"])
    np.testing.assert_array_equal(out[0]["labels"], out[2]["labels"])
    assert out[0]["segs"].tobytes() == out[2]["segs"].tobytes()
    # ROI rows that do not start on 16-byte boundaries (P1 = 214 x 107, and 21 frames so that odd windows start on a
    # 2-byte boundary): the unaligned variant of the integer kernel against the f64 start
    roi = np.concatenate([synthetic.roi_window(120 + w, 21, 212, 427, birds=6) for w in range(3)] )
    roi64 = np.concatenate([synthetic.roi_window(130 + w, 64, 107, 214, birds=6, bird_len=(10, 15), bird_wid=(4, 7)) for w in range(2)])
    res = []
    for on in (1, 0):
        c = _lib.Context(0)
        c.set_integer_start(on)
        res.append((c.batch_run(roi, 3, 21, stages=("rpca",)), c.batch_run(roi64, 2, 64, stages=("rpca",))))
        c.close()
    for a, b in zip(res[0], res[1]):
        np.testing.assert_array_equal(a["iters"], b["iters"])
        np.testing.assert_array_equal(a["rpca"], b["rpca"])


def test_sparse_store_speculation_never_changes_results(orc):
    """The M-state pass skips the per-iteration stores of the sparse image while ||Z|| is far above the stopping
    threshold, and further out forms ||Z|| every other iteration only.  Whatever the factors -- speculation off (0),
    the defaults (16 / 64 x tol), or factors so small that the guess is still in force when the iteration stops,
    which forces the rerun path -- iteration counts and outputs are the oracle's."""
    from swiftwatcher_amd import _lib, synthetic
    roi = np.concatenate([synthetic.roi_window(40 + w, 21, 64, 96, birds=3 + w, bird_len=(8, 14), bird_wid=(3, 6))
                          for w in range(3)])
    refs = [orc.window(np.ascontiguousarray(roi[w * 21:(w + 1) * 21])) for w in range(3)]
    ref_iters = []
    for w in range(3):
        gray = np.stack([orc.bgr2gray(f) for f in roi[w * 21:(w + 1) * 21]]).reshape(21, -1).T
        ref_iters.append(orc.ialm(gray, return_iters=True)[2])
    # want_redo None: alternating to the very end reruns only the windows whose last iteration is an unformed one
    for factor, nfactor, want_redo in ((0.0, 0.0, False), (16.0, 64.0, False), (1e-9, 0.0, True), (0.0, 1e-9, None),
                                       (16.0, 0.0, False), (0.0, 64.0, False)):
        c = _lib.Context(0)
        c.set_sparse_speculation(factor)
        c.set_norm_speculation(nfactor)
        res = c.batch_run(roi, 3, 21, stages=("rpca", "labels"))
        assert want_redo is None or (c.redo_batches > 0) == want_redo, (factor, nfactor, c.redo_batches)
        # only the windows whose guess failed run again (all three when the stores never start; none without a failed guess)
        assert c.redo_windows == (3 if want_redo else 0) or want_redo is None
        assert c.redo_windows <= 3 * c.redo_batches
        assert [int(i) for i in res["iters"]] == [orc_it for orc_it in ref_iters]
        for w in range(3):
            sl = slice(w * 21, (w + 1) * 21)
            np.testing.assert_array_equal(res["rpca"][sl], refs[w]["rpca"], err_msg="factor %g window %d" % (factor, w))
            np.testing.assert_array_equal(res["labels"][sl], refs[w]["labels"])
        # an iteration cap that stops the loop early must also go through the rerun and still be exact
        p = _lib.default_params()
        p.maxiter = 4
        res = c.batch_run(roi[:21], 1, 21, params=p, stages=("rpca",))
        ref = orc.window(np.ascontiguousarray(roi[:21]), maxiter=4)
        assert int(res["iters"][0]) == 4
        np.testing.assert_array_equal(res["rpca"], ref["rpca"])
        c.close()


def test_only_the_windows_whose_guess_failed_run_again(orc):
    """Eight windows of two kinds in one call.  The stores of the sparse image start once ||Z|| < factor x tol x ||X||
    (swk_set_sparse_speculation); the answer is the image the pass BEFORE the last wrote, so a window fails the guess when its ratio two
    iterations before the end was still above the factor.  The reference's ratios there (numpy, tol units): 1.72-1.76 for the one kind
    (23 iterations), 2.47-2.55 for the other (22: 12 large birds, noisy sensor) -- with a factor of 2.1 exactly the second kind fails.
    Those four windows -- and only those -- run again (one chain of their own, guesses off); every window's iteration count, sparse image,
    labels and region records are the oracle's, the untouched windows' included."""
    from swiftwatcher_amd import _lib, synthetic
    n, Hc, Wc, nwin = 21, 64, 96, 8
    kinds = (dict(birds=3, noise=2.0, bird_len=(8, 14), bird_wid=(3, 6)), dict(birds=12, noise=6.0, bird_len=(20, 30), bird_wid=(10, 14)))
    roi = np.concatenate([synthetic.roi_window(4100 + 7 * w, n, Hc, Wc, **kinds[w % 2]) for w in range(nwin)])
    c = _lib.Context(0)
    c.set_norm_speculation(0.0)
    c.set_sparse_speculation(2.1)
    res = c.batch_run(roi, nwin, n, stages=("rpca", "labels"))
    redone = c.redo_windows
    assert c.redo_batches == 1 and redone == 4, (c.redo_batches, redone)
    c.set_sparse_speculation(0.0)
    plain = c.batch_run(roi, nwin, n, stages=("rpca", "labels"))
    assert c.redo_windows == redone
    np.testing.assert_array_equal(res["iters"], plain["iters"])
    assert [int(i) for i in res["iters"]] == [23, 22] * 4
    for key in ("rpca", "labels", "nseg"):
        np.testing.assert_array_equal(res[key], plain[key], err_msg=key)
    assert res["segs"].tobytes() == plain["segs"].tobytes()
    for w in range(nwin):
        ref = orc.window(np.ascontiguousarray(roi[w * n:(w + 1) * n]))
        np.testing.assert_array_equal(res["rpca"][w * n:(w + 1) * n], ref["rpca"], err_msg="window %d" % w)
        np.testing.assert_array_equal(res["labels"][w * n:(w + 1) * n], ref["labels"])
    c.close()


def test_ialm_vs_oracle_and_null_frames(ctx, orc):
    from swiftwatcher_amd import synthetic
    roi = synthetic.roi_window(11, 21, 64, 96, birds=4, bird_len=(8, 14), bird_wid=(3, 6), null_frames=4)
    gray = np.stack([orc.bgr2gray(f) for f in roi])
    X = gray.reshape(21, -1)
    A, E, it = ctx.ialm(X)
    A0, E0, it0 = orc.ialm_defined(X.T, return_iters=True)
    assert it == it0
    np.testing.assert_allclose(A, A0, atol=ATOL_AE, rtol=0)
    np.testing.assert_allclose(E, E0, atol=ATOL_AE, rtol=0)
    assert not A[:, :4].any() and not E[:, :4].any()
    # all-zero window: defined as zeros, zero iterations
    A, E, it = ctx.ialm(np.zeros((5, 300), np.uint8))
    assert it == 0 and not A.any() and not E.any()


def test_mstate_pass_every_kstep_count(orc):
    """The M-state pass is instantiated per k-step count NK = ceil(n / 4), 1..16: every NK (and n that are / are not
    multiples of 4) on a ROI with a ragged last tile, the pipelined and the plain tile loop, with and without the
    priority / stagger knobs -- all bit-identical to one another, and to the oracle directly for n = 5, the CLI's queue of 21,
    37 and 49."""
    from swiftwatcher_amd import _lib, synthetic
    # every window holds >= 1.4e5 elements: below about 1.1e5 the first shrinkage clips most of the sky, iteration 1 sees a
    # rank-deficient M and the trajectory is chaotic in the last bit of the arithmetic (the reference itself is
    # LAPACK-dependent there) -- no two correct kernels have to agree on such a window
    cases = []
    for n in (1, 3, 4, 5, 9, 13, 18, 21, 26, 31, 36, 37, 45, 49, 52, 57, 61, 64):
        Wc = 61 + 2 * (n % 7) + (140000 // n) // 300
        cases.append((n, -(-140000 // (n * Wc)) + 1, Wc))
    ctxs = {}
    for key, (variant, tune) in {"plain": (5, 0), "pipe": (4, 0), "pipe+prio": (4, 1), "pipe+prio+stagger": (4, 3),
                                 "plain+prio": (5, 1)}.items():
        c = _lib.Context(0)
        c.set_ialm_variant(variant)
        c.set_pass_tuning(tune)
        ctxs[key] = c
    for n, Hc, Wc in cases:
        roi = np.concatenate([synthetic.roi_window(900 + n + w, n, Hc, Wc, birds=3, bird_len=(8, 14), bird_wid=(3, 6))
                              for w in range(2)])
        base = ctxs["plain"].batch_run(roi, 2, n, stages=("rpca", "labels"))
        for key, c in ctxs.items():
            if key == "plain":
                continue
            res = c.batch_run(roi, 2, n, stages=("rpca", "labels"))
            np.testing.assert_array_equal(res["iters"], base["iters"], err_msg="%s n=%d" % (key, n))
            np.testing.assert_array_equal(res["rpca"], base["rpca"], err_msg="%s n=%d" % (key, n))
            np.testing.assert_array_equal(res["labels"], base["labels"], err_msg="%s n=%d" % (key, n))
            assert res["segs"].tobytes() == base["segs"].tobytes()
        if n in (5, 21, 37, 49):
            for w in range(2):
                ref = orc.window(np.ascontiguousarray(roi[w * n:(w + 1) * n]))
                np.testing.assert_array_equal(base["rpca"][w * n:(w + 1) * n], ref["rpca"])
    for c in ctxs.values():
        c.close()


def test_short_windows_at_config1_element_count_against_oracle(orc):
    """n = 3 ... 9 frames at 9e4 to 1e5 elements per window -- the element count of BASELINE config 1's window (94 x 47 x 21 =
    92.8 k), inside the range the k-step test above leaves out -- against the ORACLE (not only kernel against kernel):
    iteration count and the uint8 sparse image, for the default k-step kernel, the plain tile loop and the A/Y-state pass."""
    from swiftwatcher_amd import _lib, synthetic
    ctxs = {}
    for key, variant in {"default": 0, "plain": 5, "ay_state": 2}.items():
        c = _lib.Context(0)
        c.set_ialm_variant(variant)
        ctxs[key] = c
    for n, Hc, Wc in ((3, 150, 208), (4, 133, 175), (5, 120, 160), (7, 101, 133), (9, 90, 117)):
        assert 9.0e4 <= n * Hc * Wc <= 1.0e5
        roi = synthetic.roi_window(1300 + n, n, Hc, Wc, birds=3, bird_len=(8, 14), bird_wid=(3, 6))
        ref = orc.window(roi)
        gray = ref["gray"].reshape(n, -1).T
        k_ref = orc.ialm(gray, return_iters=True)[2]
        for key, c in ctxs.items():
            res = c.batch_run(roi, 1, n, stages=("rpca", "labels"))
            assert int(res["iters"][0]) == k_ref, "%s n=%d: %d iterations, oracle %d" % (key, n, int(res["iters"][0]), k_ref)
            np.testing.assert_array_equal(res["rpca"], ref["rpca"], err_msg="%s n=%d" % (key, n))
            np.testing.assert_array_equal(res["labels"], ref["labels"], err_msg="%s n=%d" % (key, n))
    for c in ctxs.values():
        c.close()


def test_stopping_decision_guard_band(orc):
    """The M-state pass forms the stopping norm ||Z||_F in float32 from a binary16 copy of Y/mu (relative error about 1e-6).  A
    window whose ratio ||Z|| / (tol ||X||) lands within the guard band of 1 (default 1e-3) is not decided on that number: it is
    run again by the A/Y-state pass, which forms the norm in float64 like the reference (image_filtering.py:293-297).  Forced here
    with a band of 0.9 (every window's stopping iteration falls inside): outputs and iteration counts are unchanged, and the
    reruns are counted.

    Then a failed guess whose rerun lands in the guard band.  The norm speculation stays on to the end (factor 1e-9: the full norm is
    formed every other iteration), so a window whose ratio first comes within the band on an unformed iteration fails its guess, and
    one where that happens on a formed iteration goes to the band directly.  The rerun forms every norm, so it stops in the band as
    well.  Every window is thus counted in the band exactly once, by the first chain or by its rerun: guard_windows == nwin together
    with redo_windows >= 1 proves that at least one window went from a failed guess to the guard band and through the A/Y-state pass."""
    from swiftwatcher_amd import synthetic, _lib
    ctx = _lib.Context(0)                        # the default (M-state) pass; the parametrised fixture runs the A/Y-state kernels
    n, Hc, Wc = 21, 64, 96
    roi = np.concatenate([synthetic.roi_window(2100 + w, n, Hc, Wc, birds=3, bird_len=(8, 14), bird_wid=(3, 6)) for w in range(3)])
    base = ctx.batch_run(roi, 3, n)
    assert ctx.guard_windows == 0
    ctx.set_norm_guard(0.9)
    try:
        forced = ctx.batch_run(roi, 3, n)
        assert ctx.guard_windows == 3
    finally:
        ctx.set_norm_guard(1e-3)
    np.testing.assert_array_equal(forced["iters"], base["iters"])
    for key in ("rpca", "bilateral", "thresh", "opened", "labels"):
        np.testing.assert_array_equal(forced[key], base[key], err_msg=key)
    assert forced["segs"].tobytes() == base["segs"].tobytes()
    for w in range(3):
        ref = orc.window(np.ascontiguousarray(roi[w * n:(w + 1) * n]))
        np.testing.assert_array_equal(forced["rpca"][w * n:(w + 1) * n], ref["rpca"])
    # how often the default band fires on ordinary windows: a handful of percent at most
    many = np.concatenate([synthetic.roi_window(2200 + w, n, Hc, Wc, birds=3, bird_len=(8, 14), bird_wid=(3, 6)) for w in range(24)])
    before = ctx.guard_windows
    ctx.batch_run(many, 24, n, stages=())
    assert ctx.guard_windows - before <= 3
    ctx.close()
    # a failed guess, then the guard band (docstring)
    nwin = 6
    roi = np.concatenate([synthetic.roi_window(2100 + w, n, Hc, Wc, birds=3, bird_len=(8, 14), bird_wid=(3, 6)) for w in range(nwin)])
    ctx = _lib.Context(0)
    ctx.set_norm_speculation(1e-9)
    ctx.set_norm_guard(0.9)
    res = ctx.batch_run(roi, nwin, n, stages=("rpca", "labels"))
    assert ctx.guard_windows == nwin and ctx.redo_windows >= 1, (ctx.guard_windows, ctx.redo_windows)
    for w in range(nwin):
        ref = orc.window(np.ascontiguousarray(roi[w * n:(w + 1) * n]))
        assert int(res["iters"][w]) == ref["iters"], w
        np.testing.assert_array_equal(res["rpca"][w * n:(w + 1) * n], ref["rpca"], err_msg="window %d" % w)
        np.testing.assert_array_equal(res["labels"][w * n:(w + 1) * n], ref["labels"], err_msg="window %d" % w)
    ctx.close()


def test_stopping_norm_error_stays_below_its_derived_bound():
    """The band around tol in which the M-state pass's float32 / binary16 stopping norm is not trusted is derived per window, not chosen
    (csrc/ialm_small_dev.h: Hoeffding bound on the cross term with the measured max |U|, the exactly known ||U||_F = sqrt(n) / mu for the
    bias, the worst case of the float32 accumulation).  Checked against the truth: the A/Y-state pass forms the same norm in float64
    (the reference's statement, image_filtering.py:293-297).  Over windows of several sizes, frame counts and noise levels the two
    ratios of the LAST stopping test differ by less than the bound -- and the effective band, max(1e-3, 4 x bound), is the configured
    1e-3 at workload size (4 x bound = 0.6-1.0e-3: the derived number confirms the chosen one)."""
    from swiftwatcher_amd import _lib, synthetic
    m, a = _lib.Context(0), _lib.Context(0)
    a.set_ialm_variant(2)
    m.set_norm_guard(0.0)              # decide on the float32 number everywhere: the last ratio is then the stopping iteration's
    worst = 0.0
    cases = [(21, 64, 96, 6, dict(birds=3, bird_len=(8, 14), bird_wid=(3, 6))), (64, 64, 96, 3, dict(birds=3, bird_len=(8, 14), bird_wid=(3, 6))),
             (21, 212, 424, 4, dict()), (64, 212, 424, 2, dict()), (21, 107, 214, 4, dict(bird_len=(10, 15), bird_wid=(4, 7), noise=0.3)),
             (7, 128, 160, 3, dict(birds=2, bird_len=(8, 14), bird_wid=(3, 6), noise=6.0))]
    for n, Hc, Wc, nwin, kw in cases:
        roi = np.concatenate([synthetic.roi_window(8800 + 13 * w + n, n, Hc, Wc, **kw) for w in range(nwin)])
        rm = m.batch_run(roi, nwin, n, stages=("rpca",))
        ratio_m, bound = m.last_stopping_norms()
        ra = a.batch_run(roi, nwin, n, stages=("rpca",))
        ratio_a, zero = a.last_stopping_norms()
        np.testing.assert_array_equal(rm["iters"], ra["iters"])
        np.testing.assert_array_equal(rm["rpca"], ra["rpca"])
        assert len(ratio_m) == nwin and (zero == 0).all() and (bound > 0).all()
        rel = np.abs(ratio_m / ratio_a - 1.0)
        assert (rel < bound).all(), (n, Hc, Wc, rel, bound)
        assert (ratio_a < 1e-3).all()
        worst = max(worst, float((rel / bound).max()))
        if Hc * Wc >= 212 * 424:
            assert (4.0 * bound < 1.2e-3).all(), (n, Hc, Wc, bound)        # at workload size the derived band IS the configured 1e-3 (0.6-1.0e-3)
    assert worst < 0.5          # observed / bound: the bound has room (rounding errors average out far better than Hoeffding assumes)
    m.close()
    a.close()


def test_duplicated_last_frame_and_null_padding(ctx, orc):
    """The last window of every video: real frames, ONE duplicate of the last real frame (io_video.py:51-53 re-delivers
    it when the frame one past the end is requested) and null frames (io_video.py:40-44).  Two equal columns make M
    rank deficient exactly like the zero columns do; the zero direction gets weight 0 (oracle.ialm_defined), whichever
    solver finds it: Newton-Schulz has to notice and hand over to Jacobi."""
    from swiftwatcher_amd import synthetic
    for n, real, Hc, Wc in [(21, 8, 96, 128), (21, 20, 64, 96), (64, 30, 48, 80)]:
        roi = synthetic.roi_window(700 + n + real, n, Hc, Wc, birds=3, bird_len=(8, 14), bird_wid=(3, 6))
        # queue order, newest first: [null ... null, duplicate, last real frame, older frames ...]
        pad = n - real - 1
        roi[:pad] = 0
        roi[pad] = roi[pad + 1]
        res = ctx.batch_run(roi, 1, n)
        ref = orc.window(roi)
        gray = ref["gray"].reshape(n, -1).T
        assert int(res["iters"][0]) == orc.ialm_defined(gray, return_iters=True)[2]
        for key in ("rpca", "opened", "labels"):
            np.testing.assert_array_equal(res[key], ref[key], err_msg="%s n=%d real=%d" % (key, n, real))
        for i in range(n):
            assert _segs(res, i) == _orc_segs(ref["segments"][i])
        assert not res["rpca"][:pad].any()
        np.testing.assert_array_equal(res["rpca"][pad], res["rpca"][pad + 1])       # the two copies share one decomposition
        A, E, it = ctx.ialm(gray.T.copy())
        A0, E0 = orc.ialm_defined(gray)
        np.testing.assert_allclose(A, A0, atol=ATOL_AE, rtol=0)
        np.testing.assert_allclose(E, E0, atol=ATOL_AE, rtol=0)


# ------------------------------------------------------------------ whole window
@pytest.mark.parametrize("n,Hc,Wc,birds", [(21, 107, 214, 6), (7, 128, 160, 3), (64, 48, 80, 3)])
def test_window_all_stages(ctx, orc, n, Hc, Wc, birds):
    from swiftwatcher_amd import synthetic
    roi = synthetic.roi_window(100 + n, n, Hc, Wc, birds=birds, bird_len=(10, 15), bird_wid=(4, 7))
    res = ctx.batch_run(roi, 1, n, want_A=True, want_E=True)
    ref = orc.window(roi)
    for key in ("gray", "rpca", "bilateral", "thresh", "opened", "labels"):
        np.testing.assert_array_equal(res[key], ref[key], err_msg=key)
    assert int(res["nseg"].sum()) > 0
    for i in range(n):
        assert _segs(res, i) == _orc_segs(ref["segments"][i])


def test_4k_scale_roi(ctx, orc):
    """P3 = 850x425 (the 4K scale-up of BASELINE config 5): every stage and the per-frame labelling kernel's
    LDS bitmaps at that size, against the oracle."""
    from swiftwatcher_amd import synthetic
    roi = synthetic.roi_window(31, 7, 425, 850, birds=14, bird_len=(40, 70), bird_wid=(16, 28))
    res = ctx.batch_run(roi, 1, 7)
    ref = orc.window(roi)
    for key in ("gray", "rpca", "bilateral", "thresh", "opened", "labels"):
        np.testing.assert_array_equal(res[key], ref[key], err_msg=key)
    for i in range(7):
        assert _segs(res, i) == _orc_segs(ref["segments"][i])
    assert int(res["nseg"].sum()) >= 1


def test_batch_of_windows_with_crop_from_full_frames(ctx, orc):
    """Several windows per call, ROI cropped on the device side of the boundary from whole frames,
    different content per window (so per-window iteration counts may differ)."""
    from swiftwatcher_amd import synthetic
    crop_region = [(40, 30), (40 + 120, 30 + 60)]
    nwin, n = 3, 21
    frames = np.concatenate([synthetic.full_frames(200 + w, n, crop_region, frame_hw=(128, 200), birds=2 + w,
                                                   bird_len=(8, 12), bird_wid=(3, 5)) for w in range(nwin)])
    res = ctx.batch_run(frames, nwin, n, crop=(40, 30, 120, 60))
    for w in range(nwin):
        roi = frames[w * n:(w + 1) * n, 30:90, 40:160]
        ref = orc.window(np.ascontiguousarray(roi))
        sl = slice(w * n, (w + 1) * n)
        for key in ("gray", "rpca", "opened", "labels"):
            np.testing.assert_array_equal(res[key][sl], ref[key], err_msg="%s window %d" % (key, w))
        for i in range(n):
            assert _segs(res, w * n + i) == _orc_segs(ref["segments"][i])


def test_full_size_properties(ctx):
    """BASELINE config 2 size (424x212 ROI, 64-frame window): properties that need no oracle run.
    A + E must reproduce X to the IALM tolerance, the sparse image equals clip(-E), labels are
    consistent with the opened image, region areas sum to the foreground count."""
    from swiftwatcher_amd import synthetic
    roi = synthetic.roi_window(5, 64, 212, 424, birds=12)
    res = ctx.batch_run(roi, 1, 64, want_A=True, want_E=True)
    X = res["gray"].reshape(64, -1).T.astype(np.float64)
    A, E = res["A"][0], res["E"][0]
    assert 5 <= res["iters"][0] < 100
    assert np.linalg.norm(X - A - E) / np.linalg.norm(X) < 1e-3
    S = np.clip(-E, 0, 255).astype(np.uint8).T.reshape(64, 212, 424)
    np.testing.assert_array_equal(S, res["rpca"])
    assert np.array_equal(res["labels"] != 0, res["opened"] != 0)
    for i in range(64):
        seg = res["segs"][i, :res["nseg"][i]]
        assert int(seg["area"].sum()) == int((res["opened"][i] != 0).sum())
        assert list(seg["label"]) == sorted(seg["label"])
    assert res["nseg"].max() >= 6


# ------------------------------------------------------------------ drop-in surface
def test_framequeue_drop_in(orc):
    from swiftwatcher_amd import synthetic
    from swiftwatcher_amd.data_structures import FrameQueue
    crop_region = [(40, 30), (40 + 120, 30 + 60)]
    n = 21
    frames = synthetic.full_frames(9, n, crop_region, frame_hw=(128, 200), birds=3, bird_len=(8, 12), bird_wid=(3, 5))
    q = FrameQueue()
    assert q.maxlen == 21
    # the reader hands frames oldest first; the queue keeps the newest at index 0
    order = list(range(n - 1, -1, -1))
    q.push_list_of_frames([frames[i] for i in order], list(range(n)), ["t%d" % i for i in range(n)])
    q.preprocess_queue(crop_region, (300, 150))
    q.segment_queue((24, 24), crop_region)
    roi = np.ascontiguousarray(frames[:, 30:90, 40:160])
    ref = orc.window(roi)
    keys = ["crop", "grayscale", "RPCA", "bilateral", "thresh_15", "opened", "cc_labeling"]
    for pos in range(n):
        f = q[pos]
        assert list(f.processed_frames.keys()) == keys
        np.testing.assert_array_equal(f.processed_frames["cc_labeling"], ref["labels"][pos])
        np.testing.assert_array_equal(f.processed_frames["RPCA"], ref["rpca"][pos])
        assert [s.label for s in f.segments] == [s["label"] for s in ref["segments"][pos]]
        for s, r in zip(f.segments, ref["segments"][pos]):
            assert s.bbox == r["bbox"] and s.centroid == r["centroid"]
            box = orc.segment_crop_box(r["bbox"], (24, 24), crop_region)
            np.testing.assert_array_equal(s.segment_image, f.frame[box[0]:box[2], box[1]:box[3]])
            assert s.status is None and s.segment_history == []
    popped = q.pop_frame()
    assert popped.frame_number == 0 and q.frames_processed == 1


# ------------------------------------------------------------------ parameter variants, errors, end-to-end loop
@pytest.mark.parametrize("over", [dict(connectivity=4), dict(label_order=0), dict(bil_fma=1), dict(thresh=40),
                                  dict(gray_mode=1), dict(lmbda=0.02, tol=0.01), dict(maxiter=5)])
def test_window_parameter_variants(ctx, orc, over):
    """Every swk_params field reaches the kernels: non-default values against the oracle run the same way."""
    from swiftwatcher_amd import _lib, synthetic
    roi = synthetic.roi_window(77, 21, 64, 100, birds=4, bird_len=(10, 15), bird_wid=(4, 7))
    res = ctx.batch_run(roi, 1, 21, params=_lib.default_params(**over))
    okw = dict(over)
    if "bil_fma" in okw:
        okw["bil_fma"] = bool(okw["bil_fma"])
    ref = orc.window(roi, **okw)
    for key in ("gray", "rpca", "bilateral", "thresh", "opened", "labels"):
        np.testing.assert_array_equal(res[key], ref[key], err_msg="%s %r" % (key, over))
    for i in range(21):
        assert _segs(res, i) == _orc_segs(ref["segments"][i])
    if "maxiter" in over:
        assert res["iters"][0] == 5


def test_odd_sizes_and_gray_input(ctx, orc):
    """ROI sizes that defeat every vector path (odd width, odd pixel count), gray input passing through
    convert_grayscale (image_filtering.py:193-194), and a window of a single frame pair."""
    from swiftwatcher_amd import synthetic
    # (sizes stay above P*n ~ 1.1e5, below which the reference itself is LAPACK-dependent: DESIGN.md section 2)
    for n, Hc, Wc in [(9, 121, 183), (21, 67, 94), (2, 251, 231)]:
        roi = synthetic.roi_window(300 + n, n, Hc, Wc, birds=3, bird_len=(8, 12), bird_wid=(3, 5))
        gray = np.stack([orc.bgr2gray(f) for f in roi])
        res_c = ctx.batch_run(roi, 1, n)
        res_g = ctx.batch_run(gray, 1, n)
        ref = orc.window(roi)
        for key in ("rpca", "opened", "labels"):
            np.testing.assert_array_equal(res_c[key], ref[key], err_msg="%s %dx%dx%d" % (key, n, Hc, Wc))
            np.testing.assert_array_equal(res_g[key], ref[key])
        for i in range(n):
            assert _segs(res_c, i) == _orc_segs(ref["segments"][i])


def test_error_paths(ctx):
    from swiftwatcher_amd import _lib
    rng = np.random.default_rng(0)
    with pytest.raises(_lib.SwkError):          # more than 128 frames per window
        ctx.batch_run(rng.integers(0, 255, size=(129, 16, 16), dtype=np.uint8), 1, 129)
    with pytest.raises(_lib.SwkError):          # only the (3, 3) opening exists
        ctx.batch_run(rng.integers(0, 255, size=(4, 16, 16), dtype=np.uint8), 1, 4, params=_lib.default_params(open_kh=5))
    with pytest.raises(_lib.SwkError):
        ctx.batch_run(rng.integers(0, 255, size=(4, 16, 16), dtype=np.uint8), 1, 4, params=_lib.default_params(connectivity=6))
    with pytest.raises(_lib.SwkError):          # ROI too small for the 7x7 bilateral support
        ctx.batch_run(rng.integers(0, 255, size=(4, 3, 16), dtype=np.uint8), 1, 4)
    with pytest.raises(ValueError):
        ctx.batch_run(rng.integers(0, 255, size=(4, 16, 16), dtype=np.uint8), 1, 4, crop=(10, 10, 16, 16))
    for gone in (3, 7, -1):                     # 3 was round 1's M-state kernel
        with pytest.raises(_lib.SwkError):
            ctx.set_ialm_variant(gone)
    # the context survives errors
    out = ctx.thresh_tozero_u8(np.arange(32, dtype=np.uint8), 15)
    assert out[16] == 16 and out[15] == 0


def test_counting_loop_over_a_clip(orc):
    """The reference's per-video loop (__main__.py:71-98) over a synthetic clip whose length is not a multiple
    of the queue size: windows of 21 frames, the last one padded with null frames (io_video.py:40-44).
    Per-frame segment lists must equal the oracle's for every real frame; null frames are not counted."""
    from swiftwatcher_amd import synthetic
    from swiftwatcher_amd.data_structures import FrameQueue
    crop_region = [(30, 20), (30 + 96, 20 + 64)]
    total = 52                      # 2 full windows + 10 real frames
    clip = synthetic.full_frames(4242, total, crop_region, frame_hw=(110, 160), birds=3, bird_len=(8, 12), bird_wid=(3, 5))
    clip = clip[::-1].copy()        # synthetic stacks are newest-first; a reader delivers oldest first
    q = FrameQueue()
    per_frame = {}
    read = 0
    while q.frames_processed < total:
        frames, numbers, stamps = [], [], []
        for _ in range(q.maxlen):                           # reader.get_n_frames(n): pads past the end
            if read < total:
                frames.append(clip[read]); numbers.append(read); stamps.append("t%d" % read)
            else:
                frames.append(np.zeros_like(clip[0])); numbers.append(-1); stamps.append("00:00:00.000")
            read += 1
        q.push_list_of_frames(frames, numbers, stamps)
        q.preprocess_queue(crop_region, (300, 150))
        q.segment_queue((24, 24), crop_region)
        while not q.is_empty():
            f = q.pop_frame()
            if not f.null:
                per_frame[f.frame_number] = [(s.label, s.bbox, s.centroid) for s in f.segments]
            else:
                assert f.segments == []                     # null frames are excluded from RPCA: nothing found
    assert q.frames_processed == total and sorted(per_frame) == list(range(total))
    # oracle, window by window, in queue order (newest first)
    for w0 in range(0, total, 21):
        idx = list(range(w0, min(w0 + 21, total)))
        stack = [clip[i][20:84, 30:126] for i in idx] + [np.zeros((64, 96, 3), np.uint8)] * (21 - len(idx))
        roi = np.ascontiguousarray(np.stack(stack[::-1]))
        ref = orc.window(roi)
        for pos, seglist in enumerate(ref["segments"]):
            fn_ = w0 + 20 - pos
            if fn_ < total and fn_ in idx:
                assert per_frame[fn_] == [(s["label"], s["bbox"], s["centroid"]) for s in seglist], "frame %d" % fn_
    assert sum(len(v) for v in per_frame.values()) > 50


def test_swift_count_on_a_clip_matches_cpu_pipeline(orc):
    """Segments from the HIP path -> tracker -> events -> count, against the same tracker fed by the CPU
    oracle's segments (the tracker itself is pinned to the reference's traces in tests/test_tracking_counts.py)."""
    from swiftwatcher_amd import synthetic, pipeline
    from swiftwatcher_amd import event_classification as ec
    from swiftwatcher_amd.segment_tracking import SegmentTracker
    from swiftwatcher_amd.data_structures import Frame, Segment
    from swiftwatcher_amd.image_filtering import RegionProps
    crop_region = [(30, 20), (30 + 160, 20 + 96)]
    total = 63
    clip = synthetic.full_frames(77, total, crop_region, frame_hw=(140, 230), birds=4, bird_len=(10, 14), bird_wid=(4, 6))[::-1].copy()
    roi_mask = np.zeros((96, 160), np.uint8)
    roi_mask[40:, :] = 255
    count, events = pipeline.count_swifts(list(clip), crop_region, roi_mask)
    # CPU side: the same reader bookkeeping (null padding, duplicated last frame), oracle windows, same tracker
    from swiftwatcher_amd.io_frames import ArrayReader
    reader = ArrayReader(list(clip))
    tracker = SegmentTracker(roi_mask)
    processed = 0
    while processed < reader.total_frames:
        frames, numbers, stamps = reader.get_n_frames(21)
        roi = np.stack([f[20:116, 30:190] for f in frames][::-1])       # queue order: newest first
        ref = orc.window(np.ascontiguousarray(roi))
        for pos in range(20, -1, -1):                                     # pop order: oldest first
            k = 20 - pos
            fr = Frame(None, numbers[k], stamps[k])
            fr.segments = [Segment(RegionProps(s["label"], s["bbox"], s["centroid"], s["area"]), fr.frame_number, fr.timestamp, None)
                           for s in ref["segments"][pos]]
            tracker.step(fr)
            processed += 0 if fr.null else 1
    assert [(e[-1].parent_frame_number, len(e)) for e in events] == [(e[-1].parent_frame_number, len(e)) for e in tracker.detected_events]
    assert count == ec.count_swifts(tracker.detected_events)
    assert len(events) >= 1
    # several queue-fuls per GPU call: same frames to the tracker in the same order, so the same events
    for wpc in (2, 8):
        count_b, events_b = pipeline.count_swifts(list(clip), crop_region, roi_mask, windows_per_call=wpc)
        assert count_b == count
        assert [[(s.parent_frame_number, s.label, s.bbox, s.centroid) for s in e] for e in events_b] == \
               [[(s.parent_frame_number, s.label, s.bbox, s.centroid) for s in e] for e in events]


def test_framequeue_stage_images_stay_on_the_gpu_until_read(orc):
    """The default FrameQueue() (keep_stages=True, as the reference constructs it, data_structures.py:120) stores the six
    stage images as device-resident values: nothing is copied until a key is read, a read copies ONE image, the values
    survive the queue's next window (each window has its own device buffer, handed back to the context's free list when
    the last Frame that refers to it is gone)."""
    from swiftwatcher_amd import synthetic, _lib
    from swiftwatcher_amd.data_structures import FrameQueue, _LazyStages
    from collections import OrderedDict
    crop_region = [(40, 30), (40 + 124, 30 + 62)]          # a ROI size no other test uses: its free list starts empty
    n = 21
    q = FrameQueue()
    kept = []
    refs = []
    for seed in (9, 10):
        frames = synthetic.full_frames(seed, n, crop_region, frame_hw=(128, 200), birds=3, bird_len=(8, 12), bird_wid=(3, 5))
        q.push_list_of_frames([frames[i] for i in range(n - 1, -1, -1)], list(range(n)), ["t"] * n)
        q.preprocess_queue(crop_region, (300, 150))
        q.segment_queue((24, 24), crop_region)
        for f in q:                                          # nothing resolved yet
            raw = [OrderedDict.__getitem__(f.processed_frames, k) for k in ("RPCA", "bilateral", "thresh_15", "opened", "cc_labeling")]
            assert all(callable(v) for v in raw)
        refs.append(orc.window(np.ascontiguousarray(frames[:, 30:92, 40:164])))
        kept.append([q.pop_frame() for _ in range(n)][::-1])          # queue order again: index 0 = newest
    ctx = _lib.default_context(0)
    pool_key = (21 * 62 * 124 + 3) // 4 * 4 * 6
    assert len(ctx._plane_pool.get(pool_key, [])) == 0                     # both windows' buffers are still in use
    names = {"grayscale": "gray", "RPCA": "rpca", "bilateral": "bilateral", "thresh_15": "thresh", "opened": "opened",
             "cc_labeling": "labels"}
    for frames_of_window, ref in zip(kept, refs):                     # the FIRST window is read after the second ran
        for pos in (0, 7, 20):
            f = frames_of_window[pos]
            assert isinstance(f.processed_frames, _LazyStages)
            for name, key in names.items():
                np.testing.assert_array_equal(f.get_processed_frame(name), ref[key][pos], err_msg=name)
            assert not callable(OrderedDict.__getitem__(f.processed_frames, "opened"))        # resolved values are kept
    del kept, frames_of_window, f, raw
    import gc
    gc.collect()
    assert len(ctx._plane_pool[pool_key]) == 2                             # handed back, ready for the next windows
    q2 = FrameQueue(keep_stages=False)
    frames = synthetic.full_frames(11, n, crop_region, frame_hw=(128, 200), birds=3, bird_len=(8, 12), bird_wid=(3, 5))
    q2.push_list_of_frames([frames[i] for i in range(n - 1, -1, -1)], list(range(n)), ["t"] * n)
    q2.preprocess_queue(crop_region, None)
    q2.segment_queue((24, 24), crop_region)
    assert list(q2[0].processed_frames.keys()) == ["crop", "grayscale"]


def test_roi_at_the_frame_corner_and_gray_frames(orc):
    """The margin FrameQueue stages around the ROI is clipped to the frame (ROI in the top-left corner: no margin on two
    sides); single-channel frames (image_filtering.py:193-194) go through without a classifier batch."""
    from swiftwatcher_amd import synthetic
    from swiftwatcher_amd.data_structures import FrameQueue
    n = 21
    for crop_region, hw in (([(0, 0), (120, 60)], (70, 130)), ([(10, 4), (130, 64)], (64, 130))):
        frames = synthetic.full_frames(5, n, crop_region, frame_hw=hw, birds=3, bird_len=(8, 12), bird_wid=(3, 5))
        (x0, y0), (x1, y1) = crop_region
        ref = orc.window(np.ascontiguousarray(frames[:, y0:y1, x0:x1]))
        q = FrameQueue()
        q.push_list_of_frames([frames[i] for i in range(n - 1, -1, -1)], list(range(n)), ["t"] * n)
        q.preprocess_queue(crop_region, None)
        q.segment_queue((24, 24), crop_region)
        for pos in range(n):
            np.testing.assert_array_equal(q[pos].processed_frames["cc_labeling"], ref["labels"][pos])
            assert [(s.label, s.bbox, s.centroid) for s in q[pos].segments] == [(s["label"], s["bbox"], s["centroid"]) for s in ref["segments"][pos]]
    gray = np.ascontiguousarray(ref["gray"])
    full = np.full((n, 64, 130), 128, np.uint8)
    full[:, 4:64, 10:130] = gray
    q = FrameQueue()
    q.push_list_of_frames([full[i] for i in range(n - 1, -1, -1)], list(range(n)), ["t"] * n)
    q.preprocess_queue(crop_region, None)
    q.segment_queue((24, 24), crop_region)
    for pos in range(n):
        np.testing.assert_array_equal(q[pos].processed_frames["cc_labeling"], ref["labels"][pos])
        assert all(not hasattr(s, "_batch") for s in q[pos].segments)


def test_windows_of_more_than_64_frames(orc):
    """FrameQueue(queue_size) is free in the reference (data_structures.py:120).  Up to 64 frames the matrix-core kernels run; 65 .. 128
    frames take the plain float64 kernels (k_ialm_pass_lds<4>: variant 1 with four waves per tile; k_ialm_small_wide: cyclic Jacobi with
    its matrices in global memory).  (a) below 65 frames the wide kernels agree with variant 1 + Jacobi: same iteration count, same u8
    image, A and E to the last bits (only the order of the stopping norm's sum differs); (b) windows of 65, 96 and 128 frames against
    the oracle: every stage image, the region records, A and E within 1e-5; (c) the drop-in: FrameQueue(queue_size=96)."""
    from swiftwatcher_amd import _lib, synthetic
    from swiftwatcher_amd.data_structures import FrameQueue
    wide, v1 = _lib.Context(0), _lib.Context(0)
    wide.set_ialm_variant(6)
    v1.set_ialm_variant(1)
    v1.set_eig_method(1)
    # (the wide kernels start with the f64 pass and never take the accurate first iteration: variant 1 the same way here, so that the
    #  two differ in the summation order of the stopping norm alone)
    v1.set_integer_start(0)
    v1.set_start_refine(0.0)
    for n, Hc, Wc in ((21, 40, 60), (64, 33, 47)):
        roi = synthetic.roi_window(3000 + n, n, Hc, Wc, birds=3, bird_len=(8, 14), bird_wid=(3, 6))
        a, b = wide.batch_run(roi, 1, n, want_A=True, want_E=True), v1.batch_run(roi, 1, n, want_A=True, want_E=True)
        np.testing.assert_array_equal(a["iters"], b["iters"])
        for key in ("rpca", "labels"):
            np.testing.assert_array_equal(a[key], b[key], err_msg=key)
        np.testing.assert_allclose(a["A"], b["A"], atol=1e-11, rtol=0)
        np.testing.assert_allclose(a["E"], b["E"], atol=1e-11, rtol=0)
    v1.close()
    wide.close()
    ctx = _lib.Context(0)                                  # default context: n > 64 selects the wide kernels by itself
    for n, Hc, Wc in ((65, 40, 56), (96, 48, 64), (128, 37, 51)):
        roi = synthetic.roi_window(3100 + n, n, Hc, Wc, birds=3, bird_len=(8, 14), bird_wid=(3, 6))
        res = ctx.batch_run(roi, 1, n, want_A=True, want_E=True)
        ref = orc.window(roi)
        gray = ref["gray"].reshape(n, -1).T
        A0, E0, k0 = orc.ialm(gray, return_iters=True)
        assert int(res["iters"][0]) == k0, n
        np.testing.assert_allclose(res["A"][0], A0, atol=ATOL_AE, rtol=0)
        np.testing.assert_allclose(res["E"][0], E0, atol=ATOL_AE, rtol=0)
        for key in ("gray", "rpca", "bilateral", "thresh", "opened", "labels"):
            np.testing.assert_array_equal(res[key], ref[key], err_msg="%s n=%d" % (key, n))
        for i in range(n):
            got = [(int(s["label"]), int(s["r0"]), int(s["c0"]), int(s["r1"]), int(s["c1"]), int(s["area"])) for s in res["segs"][i, :res["nseg"][i]]]
            assert got == [(s["label"],) + s["bbox"] + (s["area"],) for s in ref["segments"][i]]
    with pytest.raises(_lib.SwkError):
        ctx.batch_run(np.zeros((129, 8, 8), np.uint8), 1, 129)
    ctx.close()
    crop_region = [(20, 10), (20 + 64, 10 + 48)]
    n = 96
    frames = synthetic.full_frames(3200, n, crop_region, frame_hw=(70, 110), birds=3, bird_len=(8, 12), bird_wid=(3, 5))
    q = FrameQueue(queue_size=n)
    q.push_list_of_frames([frames[i] for i in range(n - 1, -1, -1)], list(range(n)), ["t"] * n)
    q.preprocess_queue(crop_region, None)
    q.segment_queue((24, 24), crop_region)
    ref = orc.window(np.ascontiguousarray(frames[:, 10:58, 20:84]))
    for pos in (0, 50, 95):
        np.testing.assert_array_equal(q[pos].processed_frames["cc_labeling"], ref["labels"][pos])
        assert [(s.label, s.bbox, s.centroid) for s in q[pos].segments] == [(s["label"], s["bbox"], s["centroid"]) for s in ref["segments"][pos]]
    assert sum(len(f.segments) for f in q) >= 20
