"""The three kernels of csrc/classify_input.hip on the designed crops of tests/resize_taps.py: crops on which one outermost tap of the
horizontal or of the vertical pass decides an output byte, at every input size 1..512 (k_classifier_input, k_segment_inputs) and at
the 299 sizes of the large route where the tap count grows (k_segment_inputs_large), and formula crops on which both passes run.
tests/test_resize_taps_cpu.py shows what the crops detect.  Everything is compared bit for bit: the uint8 patches where the entry
point returns them, and the float32 network input -- (float32(byte) / float32(255) - mean) / std, held to the oracle's transform in
the CPU tests -- in sentinel-filled tensors with guard rows before and behind.  Expected tensors are put together on the device from
the host's 24 x 24 values (copies only)."""
import numpy as np
import pytest
import torch

import pil_resize_ref as P
import resize_taps as T

pytestmark = pytest.mark.gpu

SENTINEL = -7.25
GUARD = 2
ROUTES = [(100, False), (100, True), (8, False), (8, True)]          # (pad, channels-last)
PADS = [0, 1, 11, 12, 13, 99]


def _mean_std():
    from swiftwatcher_amd.segment_classification import IMAGENET_MEAN, IMAGENET_STD
    return IMAGENET_MEAN, IMAGENET_STD


def _dev():
    return torch.device("cuda", 0)


def _blank(rows, pad, nhwc):
    side = 24 + 2 * pad
    fmt = torch.channels_last if nhwc else torch.contiguous_format
    x = torch.full((rows + 2 * GUARD, 3, side, side), SENTINEL, dtype=torch.float32, device=_dev()).contiguous(memory_format=fmt)
    torch.cuda.synchronize()
    return x


def _expected(patches, pad, rows=None):
    """Logical (rows + 2 GUARD, 3, S, S): the network inputs of `patches` in rows GUARD.., the sentinel everywhere else."""
    mean, std = _mean_std()
    n = len(patches)
    rows = n if rows is None else rows
    side = 24 + 2 * pad
    exp = torch.full((rows + 2 * GUARD, 3, side, side), SENTINEL, dtype=torch.float32, device=_dev())
    exp[GUARD:GUARD + n] = torch.from_numpy(T.net_lut(mean, std)[:, 0].copy()).to(_dev()).view(1, 3, 1, 1)
    exp[GUARD:GUARD + n, :, pad:pad + 24, pad:pad + 24] = torch.from_numpy(T.net_interior(np.asarray(patches), mean, std)).to(_dev())
    return exp


def _assert_same(x, exp, names, what):
    """Every float of x, guard rows included, is exp's, bit for bit."""
    differs = (x.view(torch.int32) != exp.view(torch.int32)).flatten(1).any(1).nonzero().flatten().tolist()
    label = ["guard" if not 0 <= r - GUARD < len(names) else names[r - GUARD] for r in differs]
    assert not differs, "%s: %d rows differ: %s" % (what, len(differs), label[:12])


# ------------------------------------------------------------------ the crops
@pytest.fixture(scope="module")
def small_set():
    """name -> (crop, restated patch) of the designed crops of every size 1..512 on both axes and of the combined crops."""
    out = {}
    for s in T.SMALL_SIZES:
        d = T.design(s)
        assert not d.missing
        out["h%d" % s] = d.horizontal()
        out["v%d" % s] = d.vertical()
    for shape in T.COMBINED_SMALL:
        out["c%dx%d" % shape] = T.combined(shape)[0]
    return {name: (crop, P.patch(crop)) for name, crop in out.items()}


@pytest.fixture(scope="module")
def large_set():
    out = {}
    for s in T.LARGE_SIZES:
        d = T.design(s)
        assert not d.missing
        out["h%d" % s] = d.horizontal()
        out["v%d" % s] = d.vertical()
    return {name: (crop, P.patch(crop)) for name, crop in out.items()}


# ------------------------------------------------------------------ swk_classifier_input
@pytest.mark.parametrize("pad,nhwc", ROUTES)
def test_classifier_input_on_every_designed_crop(small_set, pad, nhwc):
    from swiftwatcher_amd import _lib
    mean, std = _mean_std()
    names = list(small_set)
    assert len(names) == 2 * 511 + len(T.COMBINED_SMALL)
    ctx = _lib.Context(0)
    step = 256 if pad == 100 else len(names)          # the full 224 x 224 input is 602 KB per crop
    for at in range(0, len(names), step):
        part = names[at:at + step]
        want = np.stack([small_set[k][1] for k in part])
        x = _blank(len(part), pad, nhwc)
        patches, _ = ctx.classifier_input([small_set[k][0] for k in part], mean, std, want_patches=True, net_ptr=x[GUARD:].data_ptr(),
                                          pad=pad, channels_last=nhwc)
        wrong = [k for k, got, exp in zip(part, patches, want) if not np.array_equal(got, exp)]
        assert not wrong, "%d patches differ: %s" % (len(wrong), wrong[:12])
        _assert_same(x, _expected(want, pad), part, "network input")
    ctx.close()


# ------------------------------------------------------------------ swk_segment_inputs
class Scene:
    """Frames (F, fh, fw, 3) inside a host buffer (F, fh + 1, fw * 3 + slack): the rows are `slack` bytes wider than the frame, and one
    row lies between two frames.  Background: a formula image; bytes outside the frames: 0xA5.  placements[f] = [(r0, c0, name), ...]:
    crops written at (r0, c0), each with a hand-written region record whose box is the crop's exact shape."""

    def __init__(self, fh, fw, slack, placements, crops):
        from swiftwatcher_amd import _lib
        F = len(placements)
        self.fh, self.fw, self.F = fh, fw, F
        self.buf = np.full((F, fh + 1, fw * 3 + slack), 0xA5, np.uint8)
        self.buf[:, :fh, :fw * 3] = P.formula_image(fh, fw, offset=91).reshape(fh, fw * 3)
        self.cap = max(1, max(len(p) for p in placements))
        self.records = np.zeros((F, self.cap), _lib.SEGMENT_DTYPE)
        self.counts = np.array([len(p) for p in placements], np.int32)
        self.names, self.frame_of = [], []
        for f, items in enumerate(placements):
            taken = np.zeros((fh, fw), bool)
            for i, (r0, c0, name) in enumerate(items):
                crop = crops[name][0]
                h, w = crop.shape[:2]
                assert 0 <= r0 and r0 + h <= fh and 0 <= c0 and c0 + w <= fw and not taken[r0:r0 + h, c0:c0 + w].any(), name
                taken[r0:r0 + h, c0:c0 + w] = True
                self.buf[f, r0:r0 + h, c0 * 3:(c0 + w) * 3] = crop.reshape(h, w * 3)
                self.records[f, i] = (i + 1, r0, c0, r0 + h, c0 + w, 0, h * w, 0, 0)
                self.names.append(name)
                self.frame_of.append(f)

    def check(self, ctx, crops, pad, nhwc, min_seg=(24, 24), chunk=None):
        """swk_segment_inputs over the scene in chunks of `chunk` segments: every row of every chunk, the guard rows and the rows behind
        a ragged last chunk, in net and in seg_frame; nothing skipped."""
        from swiftwatcher_amd import _lib
        mean, std = _mean_std()
        dev = _dev()
        frames = torch.from_numpy(self.buf).to(dev)
        segs = torch.from_numpy(self.records.view(np.uint8).reshape(self.F, self.cap, 48)).to(dev)
        nseg = torch.from_numpy(self.counts).to(dev)
        inp = _lib.Input(frames=frames.data_ptr(), mem=_lib.MEM_DEVICE, channels=3, nwin=1, n=self.F, Hc=self.fh, Wc=self.fw, x0=0, y0=0,
                         frame_stride=self.buf.shape[1] * self.buf.shape[2], row_stride=self.buf.shape[2])
        n = len(self.names)
        chunk = chunk or n
        for first in range(0, n, chunk):
            part = self.names[first:first + chunk]
            x = _blank(chunk, pad, nhwc)
            fidx = torch.full((chunk + 2 * GUARD,), -99, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            total, skipped = ctx.segment_inputs(inp, (self.fh, self.fw), segs.data_ptr(), nseg.data_ptr(), self.cap, mean, std,
                                                x[GUARD:].data_ptr(), chunk, first=first, pad=pad, min_seg_size=min_seg,
                                                seg_frame_ptr=fidx[GUARD:].data_ptr(), channels_last=nhwc)
            assert total == n and skipped == 0
            _assert_same(x, _expected(np.stack([crops[k][1] for k in part]), pad, rows=chunk), part, "segments from %d" % first)
            want = [-99] * GUARD + self.frame_of[first:first + chunk] + [-99] * (chunk - len(part) + GUARD)
            assert fidx.cpu().tolist() == want
        del frames, segs, nseg


@pytest.fixture(scope="module")
def small_scene(small_set):
    """Every size 25..512 on both axes and the combined crops in 552 x 552 frames with rows 37 bytes wider: 21 horizontal crops below
    one another per frame, an empty frame, 21 vertical crops side by side per frame, then one combined crop per frame."""
    sizes = [s for s in T.SMALL_SIZES if s > 24]
    placements = []
    for at in range(0, len(sizes), 21):
        placements.append([(2 + 26 * i, 1 + (5 * i) % 11, "h%d" % s) for i, s in enumerate(sizes[at:at + 21])])
    placements.append([])
    for at in range(0, len(sizes), 21):
        placements.append([(1 + (5 * i) % 11, 2 + 26 * i, "v%d" % s) for i, s in enumerate(sizes[at:at + 21])])
    for shape in T.COMBINED_SMALL:
        placements.append([(3, 5, "c%dx%d" % shape)])
    scene = Scene(552, 552, 37, placements, small_set)
    assert len(scene.names) == 2 * 488 + len(T.COMBINED_SMALL) and scene.F == 2 * 24 + 1 + len(T.COMBINED_SMALL)
    return scene


@pytest.mark.parametrize("pad,nhwc", ROUTES)
def test_segment_inputs_small_route_on_every_designed_crop(small_set, small_scene, pad, nhwc):
    """Boxes of height or width 24 are not grown (min_seg_size = (24, 24)); with pad = 100 the batch goes in chunks of 256 segments."""
    from swiftwatcher_amd import _lib
    ctx = _lib.Context(0)
    small_scene.check(ctx, small_set, pad, nhwc, chunk=256 if pad == 100 else None)
    ctx.close()


@pytest.fixture(scope="module")
def many_frames_scene(small_set):
    """300 frames of 96 x 96 (k_segment_prefix sums two frames per thread): frames 1, 6, 11, .. hold two crops, frames 3, 8, 13, ..
    one, every other frame none; the crops are the sizes 1..60 on both axes, cut with min_seg_size = (1, 1) so that no box grows."""
    names = ["%s%d" % (a, s) for a in "hv" for s in range(1, 61) if s != 24]
    queue = list(names)
    placements = []
    for f in range(300):
        k = min(len(queue), {1: 2, 3: 1}.get(f % 5, 0))
        placements.append([((2, 3), (30, 33))[i] + (queue.pop(0),) for i in range(k)])
    scene = Scene(96, 96, 5, placements, small_set)
    assert not queue and scene.names == names and scene.F == 300 > 256 and (scene.counts == 0).sum() > 100
    assert scene.counts[256:].sum() == 0 and scene.counts[128:256].sum() > 0          # frames of the upper half of the threads hold crops
    return scene


@pytest.mark.parametrize("nhwc,chunk", [(False, None), (True, 50)])
def test_segment_inputs_over_more_than_256_frames(small_set, many_frames_scene, nhwc, chunk):
    from swiftwatcher_amd import _lib
    ctx = _lib.Context(0)
    many_frames_scene.check(ctx, small_set, 8, nhwc, min_seg=(1, 1), chunk=chunk)
    ctx.close()


def _large_scene(large_set, axis):
    """One box per frame: horizontal crops in 24 x 4096 frames (rows 64 bytes wider), vertical crops in 4096 x 24 frames (8 bytes)."""
    if axis == "h":
        placements = [[(0, min(7, 4096 - s), "h%d" % s)] for s in T.LARGE_SIZES]
        return Scene(24, 4096, 64, placements, large_set)
    placements = [[(min(5, 4096 - s), 0, "v%d" % s)] for s in T.LARGE_SIZES]
    return Scene(4096, 24, 8, placements, large_set)


@pytest.fixture(scope="module")
def large_scenes(large_set):
    scenes = {axis: _large_scene(large_set, axis) for axis in "hv"}
    for s in scenes.values():
        assert s.F == 299 and s.buf.nbytes <= 100 << 20          # one call's frames: at most about 100 MB
    return scenes


@pytest.mark.parametrize("pad,nhwc", ROUTES)
@pytest.mark.parametrize("axis", ["h", "v"])
def test_segment_inputs_large_route_on_the_designed_sizes(large_set, large_scenes, axis, pad, nhwc):
    from swiftwatcher_amd import _lib
    ctx = _lib.Context(0)
    large_scenes[axis].check(ctx, large_set, pad, nhwc, chunk=150 if pad == 100 else None)
    ctx.close()


def _alone(name, crops, margin=(2, 3)):
    """A scene of one frame that holds one crop at `margin`."""
    h, w = crops[name][0].shape[:2]
    r0, c0 = (0 if h == 4096 else margin[0]), (0 if w == 4096 else margin[1])
    return Scene(max(h + r0 + 1, 24), max(w + c0 + 2, 24), 11, [[(r0, c0, name)]], crops)


def test_segment_inputs_large_route_with_both_passes():
    from swiftwatcher_amd import _lib
    crops = {}
    for shape in T.COMBINED_LARGE:
        image = T.combined(shape)[0]
        crops["c%dx%d" % shape] = (image, P.patch(image))
    ctx = _lib.Context(0)
    for name in crops:
        scene = _alone(name, crops)
        for pad, nhwc in ((8, True), (100, False)):
            scene.check(ctx, crops, pad, nhwc)
    ctx.close()


# ------------------------------------------------------------------ padding
def test_classifier_input_padding(small_set):
    from swiftwatcher_amd import _lib
    mean, std = _mean_std()
    names = ["c47x48", "h100", "v511"]
    want = np.stack([small_set[k][1] for k in names])
    ctx = _lib.Context(0)
    for pad in PADS:
        for nhwc in (False, True):
            x = _blank(3, pad, nhwc)
            ctx.classifier_input([small_set[k][0] for k in names], mean, std, net_ptr=x[GUARD:].data_ptr(), pad=pad, channels_last=nhwc)
            _assert_same(x, _expected(want, pad), names, "pad %d, channels-last %r" % (pad, nhwc))
    ctx.close()


def test_segment_inputs_padding_small_route(small_set):
    from swiftwatcher_amd import _lib
    scene = Scene(552, 552, 37, [[(2, 3, "c47x48"), (60, 7, "h100")], [], [(5, 9, "v511")]], small_set)
    ctx = _lib.Context(0)
    for pad in PADS:
        for nhwc in (False, True):
            scene.check(ctx, small_set, pad, nhwc)
    ctx.close()


def test_segment_inputs_padding_large_route(large_set):
    """The large kernel writes the padding rows by a formula of its own (every 24th row above and below the image row)."""
    from swiftwatcher_amd import _lib
    image = T.combined((513, 600))[0]
    crops = {"h4096": large_set["h4096"], "v529": large_set["v529"], "c513x600": (image, P.patch(image))}
    ctx = _lib.Context(0)
    for name in crops:
        scene = _alone(name, crops)
        for pad in PADS:
            for nhwc in (False, True):
                scene.check(ctx, crops, pad, nhwc)
    ctx.close()
