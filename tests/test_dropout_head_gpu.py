"""swk_nhwc_head2_dropout_relu_mean (the classifier's head under the reference's live Dropout(0.5), many realisations per launch) and
what SegmentClassifier builds on it, against the formula of include/swk.h in float64 with the mask restated in numpy
(tests/dropout_ref.py; the restatement itself is checked in tests/test_dropout_mask_cpu.py)."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

import dropout_ref as D

pytestmark = pytest.mark.gpu

# (c, px, n_pos, n, S): one live pixel and one sample; the ring taken from bg, S no multiple of 32; no ring at all; three blocks of samples
SHAPES = ((256, 1, 4, 3, 1), (512, 121, 256, 5, 33), (768, 16, 16, 2, 32), (1024, 9, 64, 2, 70))
SEED = 0x9E3779B97F4A7C15
SWK_ERR_ARG = -1               # include/swk.h


def _env():
    from swiftwatcher_amd import _lib
    dev = torch.device("cuda", 0)
    return _lib.load(), dev, ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _positions(px, n_pos):
    """px distinct positions of an n_pos map in raster order: a square inside the map's square, as the network's live square lies."""
    if px == n_pos:
        return np.arange(n_pos, dtype=np.int32)
    side, live = int(round(n_pos ** 0.5)), int(round(px ** 0.5))
    assert side * side == n_pos and live * live == px
    r0, c0 = (side - live) // 2, side - live - (side - live) // 3
    return np.array([(r0 + r) * side + c0 + c for r in range(live) for c in range(live)], dtype=np.int32)


def _keys(rng, n):
    k = rng.integers(0, 2 ** 63, size=n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=n, dtype=np.uint64)
    k[0] |= np.uint64(1 << 63)                                  # a null frame's key has the top bits set
    return k


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _launch(env, x, pos, bg, n_pos, w, b, keys, seed, S, n=None, px=None, c=None):
    """x (n, px, c) float32, pos int32, bg (n_pos, c) or None, keys uint64: -> (rc, out (n, S, 2) on the CPU or None)."""
    lib, dev, stream = env
    n = x.shape[0] if n is None else n
    px = x.shape[1] if px is None else px
    c = x.shape[2] if c is None else c
    kd = _dev(np.asarray(keys, dtype=np.uint64).view(np.int64), dev)
    out = torch.full((max(n, 1), max(S, 1), 2), -7.0, dtype=torch.float32, device=dev)
    rc = lib.swk_nhwc_head2_dropout_relu_mean(stream, x.data_ptr(), n, px, c, pos.data_ptr(), None if bg is None else bg.data_ptr(), n_pos,
                                              w.data_ptr(), b.data_ptr(), kd.data_ptr(), ctypes.c_uint64(seed), S, out.data_ptr())
    torch.cuda.synchronize()
    return rc, (out.cpu().numpy() if rc == 0 else None)


def test_exact_on_integers():
    """Small integer x, bg, w, bias and a power-of-two n_pos: every product, partial sum, the doubling and the division are exact in
    float32, so the kernel equals the float64 formula bit for bit -- which pins the mask (a wrong bit changes a sum), the x 2 scale,
    the ring taken from bg under its own mask, bg = NULL without a ring, and S that is no multiple of 32."""
    env = _env()
    dev = env[1]
    rng = np.random.default_rng(11)
    for c, px, n_pos, n, S in SHAPES:
        for signed in (False, True):
            lo = -7 if signed else 0
            x = rng.integers(lo, 8, size=(n, px, c)).astype(np.float32)
            bg = rng.integers(lo, 8, size=(n_pos, c)).astype(np.float32)
            w = rng.integers(-4, 5, size=(2, c)).astype(np.float32)
            b = rng.integers(-64, 65, size=(2,)).astype(np.float32)
            assert n_pos * (2 * c * 7 * 4 + 64) < 2 ** 24                  # every partial sum is an integer float32 holds
            pos, keys = _positions(px, n_pos), _keys(rng, n)
            ring = px < n_pos
            rc, out = _launch(env, _dev(x, dev), _dev(pos, dev), _dev(bg, dev) if ring else None, n_pos, _dev(w, dev), _dev(b, dev), keys, SEED, S)
            assert rc == 0, (c, px, n_pos, n, S)
            want = D.head_reference(x, pos, bg if ring else None, n_pos, w, b, keys, SEED, S)
            assert out.shape == want.shape
            assert np.array_equal(out.astype(np.float64), want), (c, px, n_pos, n, S, signed, float(np.abs(out - want).max()))
            # the samples differ from each other and from the eval-mode head (all kept, not doubled)
            if S > 1:
                assert len({out[0, s].tobytes() for s in range(S)}) > S // 2


def test_float_data_within_the_eval_heads_bound():
    """randn features on the same four shapes: within rtol = atol = 2e-6 of float64, the bound
    test_head_kernel_against_torch_and_batch_independence holds the eval head to (the kept terms are doubled exactly, the rest vanish)."""
    env = _env()
    dev = env[1]
    g = torch.Generator().manual_seed(12)
    rng = np.random.default_rng(12)
    worst = 0.0
    for c, px, n_pos, n, S in SHAPES:
        x = torch.randn((n, px, c), generator=g)
        bg = torch.randn((n_pos, c), generator=g)
        w = torch.randn((2, c), generator=g) * 0.05
        b = torch.randn((2,), generator=g)
        pos, keys = _positions(px, n_pos), _keys(rng, n)
        ring = px < n_pos
        rc, out = _launch(env, x.to(dev), _dev(pos, dev), bg.to(dev) if ring else None, n_pos, w.to(dev), b.to(dev), keys, 5, S)
        assert rc == 0
        want = D.head_reference(x.numpy(), pos, bg.numpy() if ring else None, n_pos, w.numpy(), b.numpy(), keys, 5, S)
        err = float((np.abs(out - want) / (2e-6 + 2e-6 * np.abs(want))).max())
        worst = max(worst, err)
        print("c %d px %d n_pos %d S %d: max |kernel - float64| %.3g, %.3f of the bound" % (c, px, n_pos, S, float(np.abs(out - want).max()), err))
        np.testing.assert_allclose(out, want, rtol=2e-6, atol=2e-6)
        assert float(want.std()) > 1e-3                         # the samples do spread


def test_batch_independence():
    """A segment's S x 2 scores are a function of its features and its key: rows 64..96 of a 300-row call equal those rows scored
    alone, permuting rows with their keys permutes the output, and changing one row's key changes that row only."""
    env = _env()
    dev = env[1]
    c, px, n_pos, n, S = 512, 121, 169, 300, 33
    g = torch.Generator().manual_seed(13)
    rng = np.random.default_rng(13)
    x = torch.randn((n, px, c), generator=g).to(dev)
    bg, w, b = torch.randn((n_pos, c), generator=g).to(dev), (torch.randn((2, c), generator=g) * 0.05).to(dev), torch.randn((2,), generator=g).to(dev)
    pos = _dev(_positions(px, n_pos), dev)
    keys = _keys(rng, n)
    rc, whole = _launch(env, x, pos, bg, n_pos, w, b, keys, 77, S)
    assert rc == 0
    rc, part = _launch(env, x[64:96].contiguous(), pos, bg, n_pos, w, b, keys[64:96], 77, S)
    assert rc == 0 and np.array_equal(part, whole[64:96])
    want = D.head_reference(x[64:66].cpu().numpy(), pos.cpu().numpy(), bg.cpu().numpy(), n_pos, w.cpu().numpy(), b.cpu().numpy(), keys[64:66], 77, S)
    np.testing.assert_allclose(whole[64:66], want, rtol=2e-6, atol=2e-6)
    perm = rng.permutation(n)
    rc, shuffled = _launch(env, x[torch.from_numpy(perm).to(dev)].contiguous(), pos, bg, n_pos, w, b, keys[perm], 77, S)
    assert rc == 0 and np.array_equal(shuffled, whole[perm])
    other = keys.copy()
    other[150] ^= np.uint64(1)
    rc, changed = _launch(env, x, pos, bg, n_pos, w, b, other, 77, S)
    assert rc == 0
    rows = np.flatnonzero((changed != whole).any(axis=(1, 2)))
    assert rows.tolist() == [150]
    assert (changed[150] != whole[150]).mean() > 0.9
    rc, reseeded = _launch(env, x, pos, bg, n_pos, w, b, keys, 78, S)
    assert rc == 0 and (reseeded != whole).mean() > 0.9
    # fewer samples are the first ones of more, bit for bit (a block of at most four samples crosses the wave another way)
    for few in (1, 3, 4, 5):
        rc, first = _launch(env, x[:40].contiguous(), pos, bg, n_pos, w, b, keys[:40], 77, few)
        assert rc == 0 and np.array_equal(first, whole[:40, :few]), few


def test_refusals_and_a_good_call_after_them():
    """SWK_ERR_ARG on a null pointer, a bad c, samples outside 1..256, px > n_pos and misaligned x / w / bg; a good call on the same stream
    then still gives what it gave before."""
    env = _env()
    dev = env[1]
    c, px, n_pos, n, S = 512, 9, 16, 4, 5
    g = torch.Generator().manual_seed(14)
    x, bg = torch.randn((n, px, c), generator=g).to(dev), torch.randn((n_pos + 1, c), generator=g).to(dev)
    wbuf, b = (torch.randn((2 * c + 4,), generator=g) * 0.05).to(dev), torch.randn((2,), generator=g).to(dev)
    w = wbuf[:2 * c]
    pos = _dev(_positions(px, n_pos), dev)
    keys = _keys(np.random.default_rng(14), n)
    rc, good = _launch(env, x, pos, bg, n_pos, w, b, keys, 1, S)
    assert rc == 0

    class Null:
        @staticmethod
        def data_ptr():
            return None

    def off(t):
        return t.view(-1)[1:]                   # 4 bytes past a 16-byte boundary

    bad = [dict(x=Null), dict(pos=Null), dict(bg=Null), dict(w=Null), dict(b=Null),                # null pointers (bg: px < n_pos)
           dict(c=c + 4), dict(c=128), dict(c=1280), dict(S=0), dict(S=257), dict(S=-1),
           dict(px=n_pos + 1), dict(n=0), dict(x=off(x)), dict(w=off(wbuf)), dict(bg=off(bg))]
    for kw in bad:
        a = dict(x=x, pos=pos, bg=bg, n_pos=n_pos, w=w, b=b, keys=keys, seed=1, S=S)
        extra = {k: kw[k] for k in ("c", "px", "n") if k in kw}
        a.update({k: v for k, v in kw.items() if k not in extra})
        rc, _ = _launch(env, a["x"], a["pos"], a["bg"], a["n_pos"], a["w"], a["b"], a["keys"], a["seed"], a["S"], n=extra.get("n", n),
                        px=extra.get("px", px), c=extra.get("c", c))
        assert rc == SWK_ERR_ARG, kw
    lib, _, stream = env
    out = torch.empty((n, S, 2), dtype=torch.float32, device=dev)
    kd = _dev(keys.view(np.int64), dev)
    assert lib.swk_nhwc_head2_dropout_relu_mean(stream, x.data_ptr(), n, px, c, pos.data_ptr(), bg.data_ptr(), n_pos, w.data_ptr(), b.data_ptr(),
                                                None, ctypes.c_uint64(1), S, out.data_ptr()) == SWK_ERR_ARG
    assert lib.swk_nhwc_head2_dropout_relu_mean(stream, x.data_ptr(), n, px, c, pos.data_ptr(), bg.data_ptr(), n_pos, w.data_ptr(), b.data_ptr(),
                                                kd.data_ptr(), ctypes.c_uint64(1), S, None) == SWK_ERR_ARG
    rc, again = _launch(env, x, pos, bg, n_pos, w, b, keys, 1, S)
    assert rc == 0 and np.array_equal(again, good)


# ------------------------------------------------------------------ the classifier
CLF_SEED, CLF_SAMPLES, CLF_CROPS = 0, 32, 40
_CASE = {}


def _crops(seed, n):
    """Synthetic segment crops of the kind model.pt is undecided about: 24..30 px of graded sky with one small faint dark blob and
    pixel noise (the fixture's own crops are nearly all dropped in every realisation).  Seed 1 chosen on the CPU: the float64 forward
    splits its decision on five of the 40 and has one of the 1,280 samples within 4e-4 of a tie."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        h, w = int(rng.integers(24, 31)), int(rng.integers(24, 31))
        yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
        img = np.repeat((150 + 65 * rng.random() + 0.4 * yy)[:, :, None], 3, 2) * np.array([1.0, 0.97, 0.93])
        a, b, th = rng.uniform(2.5, 4.5), rng.uniform(2, 3.2), rng.uniform(0, np.pi)
        cy, cx = h / 2 + rng.uniform(-3, 3), w / 2 + rng.uniform(-3, 3)
        u = (xx - cx) * np.cos(th) + (yy - cy) * np.sin(th)
        v = -(xx - cx) * np.sin(th) + (yy - cy) * np.cos(th)
        img -= rng.uniform(20, 45) * np.clip(1.5 - np.sqrt((u / a) ** 2 + (v / b) ** 2), 0, 1)[:, :, None]
        img += rng.normal(0, 2.5, img.shape)
        out.append(np.clip(np.rint(img), 0, 255).astype(np.uint8))
    return out


def _classifier_case(golden_dir):
    """model.pt's weights, 40 synthetic crops (_crops), their keys, and the float64 reference: a torch float64 forward of
    SqueezeNet10 with the restated mask (x 2) applied in front of classifier[1].  Made once, shared, never changed."""
    if not _CASE:
        from swiftwatcher_amd.data_structures import segment_keys
        from swiftwatcher_amd.segment_classification import SegmentClassifier, SqueezeNet10
        g = np.load(os.path.join(golden_dir, "classifier_model_pt.npz"))
        sd = {k[2:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("w:")}
        crops = _crops(1, CLF_CROPS)
        segments = [types.SimpleNamespace(parent_frame_number=(-1 if i == 7 else 40 + i // 3), label=1 + i % 3, segment_image=crops[i])
                    for i in range(CLF_CROPS)]
        keys = segment_keys([s.parent_frame_number for s in segments], [s.label for s in segments])
        cpu = SegmentClassifier.from_state_dict(sd, device="cpu", cropped=False)
        model = SqueezeNet10(2).double().eval()
        model.load_state_dict({k: v.double() for k, v in sd.items()}, strict=True)
        with torch.no_grad():
            feats = model.features(cpu.preprocess(crops).double())                              # (k, 512, 13, 13)
            _, ch, h, w = feats.shape
            ref = np.empty((CLF_CROPS, CLF_SAMPLES, 2))
            for i in range(CLF_CROPS):
                m = D.mask(CLF_SEED, keys[i], CLF_SAMPLES, h * w, ch).reshape(CLF_SAMPLES, h, w, ch)
                dropped = feats[i][None] * 2.0 * torch.from_numpy(m).permute(0, 3, 1, 2).double()  # nn.Dropout(0.5) with this mask
                ref[i] = torch.relu(model.classifier[1](dropped)).mean(dim=(2, 3)).numpy()
        _CASE.update(sd=sd, crops=crops, segments=segments, keys=keys, ref=ref)
    return _CASE


def test_classifier_dropout_scores_cropped_full_and_float64(golden_dir):
    """dropout_scores on the cropped and on the full network path against each other and against the float64 forward (2e-4, what the
    suite uses between those paths); keep_probability equals the share that forward gives.  Samples whose float64 margin |s1 - s0| is
    below 4e-4 are left out of the decision comparison -- at most 2 % of them, which the float64 forward alone must satisfy."""
    from swiftwatcher_amd.segment_classification import SegmentClassifier
    c = _classifier_case(golden_dir)
    ref = c["ref"]
    margin = np.abs(ref[:, :, 1] - ref[:, :, 0])
    near = margin < 4e-4
    keep64 = ref[:, :, 1] > ref[:, :, 0]
    print("float64: %d of %d samples within 4e-4 of a tie; kept share %.3f; segments with a split decision %d of %d" % (
        near.sum(), near.size, keep64.mean(), int(((keep64.mean(1) > 0) & (keep64.mean(1) < 1)).sum()), len(ref)))
    assert near.mean() <= 0.02
    split = (keep64.mean(1) > 0) & (keep64.mean(1) < 1)
    assert 0.02 < keep64.mean() < 0.98 and split.sum() >= 3         # the dropout decides both ways on this set
    got = {}
    for cropped in (True, False):
        clf = SegmentClassifier.from_state_dict(c["sd"], cropped=cropped)
        clf._cudnn_benchmark = False            # the full path's features: MIOpen's immediate mode, no search per batch shape
        sc = clf.dropout_scores(c["crops"], c["keys"], samples=CLF_SAMPLES, seed=CLF_SEED)
        assert sc.shape == (CLF_CROPS, CLF_SAMPLES, 2) and sc.dtype == torch.float32 and sc.is_cuda
        got[cropped] = sc.cpu().numpy()
        print("cropped=%s: max |scores - float64| %.3g" % (cropped, float(np.abs(got[cropped] - ref).max())))
        np.testing.assert_allclose(got[cropped], ref, rtol=0, atol=2e-4)
        keep = got[cropped][:, :, 1] > got[cropped][:, :, 0]
        assert np.array_equal(keep[~near], keep64[~near])
        kp = clf.keep_probability(c["segments"], samples=CLF_SAMPLES, seed=CLF_SEED)
        assert kp.shape == (CLF_CROPS,)
        assert np.array_equal(kp, keep.mean(axis=1))
        assert (np.abs(kp * CLF_SAMPLES - keep64.sum(axis=1)) <= near.sum(axis=1)).all()
        clean = near.sum(axis=1) == 0
        assert clean.sum() > CLF_CROPS // 2 and np.array_equal(kp[clean], keep64[clean].mean(axis=1))
        # fewer samples are the first ones of more, fewer segments the same segments: bit for bit on the library's own kernels (the
        # full path's features come from MIOpen, which picks its convolution by the batch size)
        if cropped:
            few = clf.dropout_scores(c["crops"][:9], c["keys"][:9], samples=3, seed=CLF_SEED).cpu().numpy()
            assert np.array_equal(few, got[cropped][:9, :3])
    np.testing.assert_allclose(got[True], got[False], rtol=0, atol=2e-4)
    with pytest.raises(ValueError):
        clf.dropout_scores(c["crops"][:2], c["keys"][:3])
    with pytest.raises(ValueError):
        clf.dropout_scores(c["crops"][:2], c["keys"][:2], samples=257)


def test_dropout_seed_none_is_untouched(golden_dir):
    """Without a dropout_seed nothing changes: the public calls give clf._forward's eval-mode scores bit for bit -- also right after
    dropout sampling went through the same persistent tiles -- and the kept segments are that forward's argmax."""
    from swiftwatcher_amd.segment_classification import SegmentClassifier
    c = _classifier_case(golden_dir)
    clf = SegmentClassifier.from_state_dict(c["sd"])
    assert clf.dropout_seed is None
    x = clf.preprocess(c["crops"], window=True)
    b = clf._bucket(CLF_CROPS)
    direct = clf._forward(torch.cat([x, x[:1].expand(b - CLF_CROPS, -1, -1, -1)]))[:CLF_CROPS].clone()
    first = clf.scores(c["crops"]).clone()
    assert torch.equal(first, direct)
    clf.dropout_scores(c["crops"], c["keys"], samples=40, seed=9)
    assert torch.equal(clf.scores(c["crops"]), direct)
    seeded = SegmentClassifier.from_state_dict(c["sd"], dropout_seed=4)
    assert torch.equal(seeded.scores(c["crops"]), direct)            # scores() is the eval-mode definition in either mode
    segs = [types.SimpleNamespace(**vars(s)) for s in c["segments"]]
    kept = clf(segs)
    want = [i for i in range(CLF_CROPS) if int(torch.max(direct, 1)[1][i]) == 1]
    assert [s.segment_image is c["crops"][i] for s, i in zip(kept, want)] == [True] * len(want) and len(kept) == len(want)
    assert [s.label for s in kept] == list(range(1, len(kept) + 1))
    # with a seed the decision is sample 0 of dropout_scores under the segments' keys
    segs = [types.SimpleNamespace(**vars(s)) for s in c["segments"]]
    kept = seeded(segs)
    s0 = seeded.dropout_scores(c["crops"], c["keys"], samples=1, seed=4)[:, 0].cpu().numpy()
    want = [i for i in range(CLF_CROPS) if s0[i, 1] > s0[i, 0]]
    assert len(kept) == len(want) and all(s.segment_image is c["crops"][i] for s, i in zip(kept, want))


def test_one_realisation_through_the_counting_loop(golden_dir, monkeypatch):
    """pipeline.count_swifts over 2 windows + a padded one with SegmentClassifier(dropout_seed=3), one window per call (the serial loop:
    the window's table from the device hand-over, looked up frame by frame) and two windows per call (a batch of windows scored ahead):
    the segments the tracker is handed are the same, and they are the ones sample 0 of dropout_scores keeps under keys built from
    (frame number, label)."""
    from swiftwatcher_amd import pipeline, synthetic
    from swiftwatcher_amd.data_structures import segment_keys
    from swiftwatcher_amd.segment_classification import SegmentClassifier
    c = _classifier_case(golden_dir)
    crop_region = [(30, 20), (30 + 96, 20 + 64)]
    clip = synthetic.full_frames(4343, 52, crop_region, frame_hw=(110, 160), birds=6, bird_len=(5, 8), bird_wid=(4, 6), contrast=(25, 40))[::-1].copy()
    roi_mask = np.zeros((64, 96), np.uint8)
    roi_mask[32:, 10:86] = 255
    offered, seen = {}, {}

    class Recording(SegmentClassifier):
        def _note(self, segments):
            for s in segments:
                if s.parent_frame_number >= 0:
                    offered[(s.parent_frame_number, s.label)] = (tuple(s.bbox), np.array(s.segment_image))

        def __call__(self, segments):
            self._note(segments)
            return super().__call__(segments)

        def classify_frames(self, frames):
            for fr in frames:
                self._note(fr.segments)
            return super().classify_frames(frames)

    class Spy(pipeline.SegmentTracker):
        def set_current_frame(self, frame):
            if frame.frame_number >= 0:
                seen[frame.frame_number] = [tuple(s.bbox) for s in frame.segments]
            super().set_current_frame(frame)

    monkeypatch.setattr(pipeline, "SegmentTracker", Spy)
    clf = Recording.from_state_dict(c["sd"], dropout_seed=3)
    handed = []
    inner = clf.predict_last_batch
    clf.predict_last_batch = lambda *a, **k: (handed.append(len(k["keys"])), inner(*a, **k))[1]
    runs = []
    for wpc in (1, 2):
        seen.clear()
        pipeline.count_swifts(list(clip), crop_region, roi_mask, classifier=clf, windows_per_call=wpc)
        runs.append({k: list(v) for k, v in seen.items()})
    assert len(handed) == 3 + 2 and sum(handed[:3]) == sum(handed[3:]) >= len(offered)          # every window went through the device hand-over
    assert runs[0] == runs[1]
    order = sorted(offered)
    keys = segment_keys([f for f, _ in order], [lab for _, lab in order])
    s0 = clf.dropout_scores([offered[k][1] for k in order], keys, samples=1, seed=3)[:, 0].cpu().numpy()
    keep = s0[:, 1] > s0[:, 0]
    print("%d segments offered, %d kept under seed 3" % (len(order), int(keep.sum())))
    assert len(order) > 100 and 0 < keep.sum() < len(order)
    expected = {}
    for (frame, _), k in zip(order, keep):
        expected.setdefault(frame, [])
        if k:
            expected[frame].append(offered[(frame, _)][0])
    for frame in sorted(runs[0]):
        assert runs[0][frame] == expected.get(frame, []), "frame %d" % frame
    # another seed is another realisation
    other = clf.dropout_scores([offered[k][1] for k in order], keys, samples=1, seed=4)[:, 0].cpu().numpy()
    assert not np.array_equal(other[:, 1] > other[:, 0], keep)


def _windows(total, n):
    """`total` frames of a small clip as get_n_frames hands them out: (clip, crop region, list of (frames, numbers, stamps))."""
    from swiftwatcher_amd import synthetic
    from swiftwatcher_amd.io_frames import ArrayReader
    crop_region = [(30, 20), (30 + 96, 20 + 64)]
    clip = synthetic.full_frames(4344, total, crop_region, frame_hw=(110, 160), birds=6, bird_len=(5, 8), bird_wid=(4, 6), contrast=(25, 40))[::-1].copy()
    reader = ArrayReader(list(clip))
    return clip, crop_region, [reader.get_n_frames(n) for _ in range(total // n)]


def _assert_one_realisation(clf, frames, seed):
    """classify_frames on frames whose batch was segmented WITHOUT a classifier (the keys are made when the scores are asked for): the
    kept segments are the ones sample 0 of dropout_scores keeps under keys made from (frame number, label), through the device hand-over."""
    from swiftwatcher_amd.data_structures import segment_keys
    segs = [s for fr in frames for s in fr.segments]
    before = [(s.parent_frame_number, s.label, tuple(s.bbox), np.array(s.segment_image)) for s in segs]
    handed = []
    inner = clf.predict_last_batch
    clf.predict_last_batch = lambda *a, **k: (handed.append(len(k["keys"])), inner(*a, **k))[1]
    clf.classify_frames(frames)
    clf.predict_last_batch = inner
    assert handed == [len(segs)]
    keys = segment_keys([b[0] for b in before], [b[1] for b in before])
    s0 = clf.dropout_scores([b[3] for b in before], keys, samples=1, seed=seed)[:, 0].cpu().numpy()
    keep = s0[:, 1] > s0[:, 0]
    want = [(b[0], b[2]) for b, k in zip(before, keep) if k]
    got = [(s.parent_frame_number, tuple(s.bbox)) for fr in frames for s in fr.segments]
    assert got == want
    return len(segs), int(keep.sum())


@pytest.mark.parametrize("nwin", [1, 2])
def test_keys_made_late_for_a_batch_of_windows(golden_dir, nwin):
    """segment_windows(classifier=None), then a seeded classifier asks for the batch's scores: the keys are built at that moment, from
    the batch's own frame numbers (newest frame first, window by window) -- one window and two."""
    from swiftwatcher_amd.data_structures import segment_windows
    from swiftwatcher_amd.segment_classification import SegmentClassifier
    c = _classifier_case(golden_dir)
    _, crop_region, windows = _windows(42, 21)
    popped = segment_windows(windows[:nwin], crop_region, classifier=None)
    clf = SegmentClassifier.from_state_dict(c["sd"], dropout_seed=3)
    total, kept = _assert_one_realisation(clf, [fr for w in popped for fr in w], 3)
    print("%d window(s): %d segments, %d kept" % (nwin, total, kept))
    assert total > 30 * nwin and 0 < kept < total


def test_keys_of_a_group_call(golden_dir):
    """segment_window_groups over two videos at their own crop regions (the second one's frames numbered from 1000), scored in one
    batch: every segment gets the draw its (frame number, label) key gives it in the serial loop."""
    from swiftwatcher_amd.data_structures import segment_window_groups
    from swiftwatcher_amd.segment_classification import SegmentClassifier
    c = _classifier_case(golden_dir)
    _, crop_region, windows = _windows(42, 21)
    other = [(frames, [k + 1000 for k in numbers], stamps) for frames, numbers, stamps in windows[:1]]
    region_b = [(crop_region[0][0] + 4, crop_region[0][1] + 2), (crop_region[1][0] - 12, crop_region[1][1] - 6)]
    out = segment_window_groups([(windows, crop_region), (other, region_b)], classifier=None)
    assert [len(g) for g in out] == [2, 1]
    frames = [fr for g in out for w in g for fr in w]
    assert {fr.frame_number for fr in frames} >= {0, 41, 1000, 1020}
    clf = SegmentClassifier.from_state_dict(c["sd"], dropout_seed=3)
    total, kept = _assert_one_realisation(clf, frames, 3)
    print("two groups: %d segments, %d kept" % (total, kept))
    assert total > 90 and 0 < kept < total
