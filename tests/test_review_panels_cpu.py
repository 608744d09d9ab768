"""The review video's stage panels without a GPU: the mosaic's layout, the declarations and the record's layout, the palette, what
ReviewWriter plans with stages= (columns, gains, captions, the device and the host path) and the command line."""
import ctypes
import os
import re
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import review_text_ref as tref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------ layout
@pytest.mark.parametrize("Hc,Wc,Hp,Wp", [(2, 2, 2, 2), (3, 5, 4, 6), (6, 8, 6, 8), (7, 13, 8, 14), (47, 94, 48, 94), (212, 424, 212, 424)])
def test_layout(Hc, Wc, Hp, Wp):
    from swiftwatcher_amd._lib import panel_layout
    for cells in (1, 2, 4, 5):
        for cols in (1, 2, cells, 16):
            height, width, origins = panel_layout(Hc, Wc, cells, cols)
            rows = -(-cells // cols)
            assert (height, width) == (rows * Hp, cols * Wp) and len(origins) == cells
            assert origins == [((k // cols) * Hp, (k % cols) * Wp) for k in range(cells)]
            assert all(r % 2 == 0 and c % 2 == 0 and r + Hp <= height and c + Wp <= width for r, c in origins)
            assert len(set(origins)) == cells and origins[0] == (0, 0)
    # a last row that is not full: five cells in rows of two are three rows, the sixth place stays empty
    assert panel_layout(3, 5, 5, 2) == (12, 12, [(0, 0), (0, 6), (4, 0), (4, 6), (8, 0)])
    assert panel_layout(3, 5, 5, 1)[:2] == (20, 6) and panel_layout(3, 5, 5, 5)[:2] == (4, 30)
    for bad in [(0, 5, 1, 1), (3, 0, 1, 1), (3, 5, 0, 1), (3, 5, 1, 0)]:
        with pytest.raises(ValueError):
            panel_layout(*bad)


# ------------------------------------------------------------------------------------------ declarations and layout of the record
def test_header_declares_the_struct_and_both_functions():
    from swiftwatcher_amd import _lib
    header = open(os.path.join(ROOT, "include", "swk.h")).read()
    assert re.search(r"}\s*swk_review_panel\s*;", header)
    assert re.search(r"int32_t\s+swk_render_review_panels\s*\(", header) and re.search(r"void\s+swk_review_label_palette\s*\(", header)
    assert re.search(r"#define\s+SWK_PANEL_GRAY\s+0\b", header) and re.search(r"#define\s+SWK_PANEL_LABELS\s+1\b", header)
    assert "swk_render_review_panels" in _lib.EXPORTS and "swk_review_label_palette" in _lib.EXPORTS
    assert (_lib.PANEL_GRAY, _lib.PANEL_LABELS) == (0, 1)
    assert _lib.ABI_VERSION == 2 and "#define SWK_ABI_VERSION 2" in header
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "swk_render_review_panels" in doc and "swk_review_label_palette" in doc


def test_panel_struct_matches_the_header(tmp_path):
    """_lib.ReviewPanel against the C compiler's layout of swk_review_panel: size and every field's offset."""
    from swiftwatcher_amd import _lib
    fields = ["plane", "mem", "kind", "frame_stride", "row_stride", "gain", "layers", "caption"]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "swk.h"\nint main(){printf("%zu", sizeof(swk_review_panel));\n'
                   + "".join('printf(" %%zu", offsetof(swk_review_panel, %s));\n' % f for f in fields)
                   + 'printf(" %zu %zu", sizeof(swk_review_label), offsetof(swk_review_label, text));return 0;}')
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "sz")])
    got = [int(v) for v in subprocess.check_output([str(tmp_path / "sz")]).split()]
    assert got == ([ctypes.sizeof(_lib.ReviewPanel)] + [getattr(_lib.ReviewPanel, f).offset for f in fields]
                   + [ctypes.sizeof(_lib.ReviewLabel), _lib.ReviewLabel.text.offset])
    assert ctypes.sizeof(_lib.ReviewPanel) == 104 and ctypes.sizeof(_lib.ReviewLabel) == _lib.REVIEW_LABEL_DTYPE.itemsize == 64
    assert [(n, getattr(_lib.ReviewLabel, n).offset) for n, _ in _lib.ReviewLabel._fields_] == \
        [(n, _lib.REVIEW_LABEL_DTYPE.fields[n][1]) for n in _lib.REVIEW_LABEL_DTYPE.names]


def test_panel_structs_from_dicts():
    """Context._panel_structs without a context: what the library is handed for a host plane with strides, a raw device plane, a caption."""
    from swiftwatcher_amd import _lib
    inp = _lib.Input(nwin=1, n=3, Hc=4, Wc=6)
    back = np.zeros((3, 5, 9), np.uint8)
    host = back[::-1, :4, 2:8]
    structs, keep = _lib.Context._panel_structs(None, [
        dict(plane=host, kind="gray", gain=4, layers=14, caption=(5, 6, 5, 6, 2, "RPCA X4")),
        dict(plane={"ptr": 4096, "frame_stride": -24, "row_stride": 6}, kind="labels")], inp)
    a, b = structs[0], structs[1]
    assert (a.plane, a.mem, a.kind, a.frame_stride, a.row_stride, a.gain, a.layers) == (host.ctypes.data, _lib.MEM_HOST, 0, -45, 9, 4, 14)
    assert (a.caption.r, a.caption.c, a.caption.style, a.caption.plate, a.caption.scale, a.caption.len) == (5, 6, 5, 6, 2, 7)
    assert bytes(a.caption.text[:7]) == b"RPCA X4"
    assert (b.plane, b.mem, b.kind, b.frame_stride, b.row_stride, b.gain, b.layers, b.caption.len) == (4096, _lib.MEM_DEVICE, 1, -24, 6, 1, 0, 0)
    assert _lib.Context._panel_structs(None, [], inp) == (None, ())
    wide = np.zeros((3, 4, 12), np.uint8)
    for bad in [dict(plane=back[:, :4, :6], kind="colour"), dict(plane=back[:, :4, :5]), dict(plane=back[:, :4, :6].astype(np.int16)),
                dict(plane=back[:, :4, :6], gian=2), dict(plane=wide[:, :, ::2])]:          # (the last: not contiguous along columns)
        with pytest.raises(ValueError):
            _lib.Context._panel_structs(None, [bad], inp)


# ------------------------------------------------------------------------------------------ the palette
def test_palette():
    from swiftwatcher_amd import _lib
    pal = _lib.review_label_palette()
    assert pal.shape == (256, 3) and pal.dtype == np.uint8
    assert pal[0].tolist() == [0, 0, 0]
    assert pal[1:].any(axis=1).all()                                         # entries 1..255 are not black
    assert (pal[:-1] != pal[1:]).any(axis=1).all()                           # palette[v] != palette[v + 1]
    # the rule the header documents: twelve hues at three strengths
    hues = [(0, 0, 255), (0, 255, 0), (255, 0, 0), (0, 255, 255), (255, 0, 255), (255, 255, 0), (0, 128, 255), (128, 255, 0), (255, 0, 128),
            (255, 128, 0), (128, 0, 255), (0, 255, 128)]
    want = [[0, 0, 0]] + [[(x * (256, 176, 112)[((v - 1) // 12) % 3]) >> 8 for x in hues[(v - 1) % 12]] for v in range(1, 256)]
    assert pal.tolist() == want
    assert len({tuple(p) for p in pal[1:37].tolist()}) == 36                 # the first 36 labels of a frame are pairwise distinct


# ------------------------------------------------------------------------------------------ the writer
def _writer(tmp_path, size=(300, 120), **kw):
    from swiftwatcher_amd.review import ReviewWriter
    W, H = size
    return ReviewWriter(str(tmp_path / "review.y4m"), [(10, 20), (10 + W, 20 + H)], np.zeros((H, W), np.uint8), 30, **kw)


def test_stage_names():
    from swiftwatcher_amd import review
    from swiftwatcher_amd.data_structures import STAGE_KEYS
    assert review.stage_keys(()) == () and review.stage_keys(list(STAGE_KEYS)) == tuple(STAGE_KEYS)
    assert review.stage_keys(STAGE_KEYS.values()) == tuple(STAGE_KEYS)                                     # the processed_frames names
    assert review.stage_keys(["labels", "RPCA", "thresh_15", "rpca", "labels"]) == ("labels", "rpca", "thresh", "rpca", "labels")
    assert review.stage_keys("rpca, thresh,cc_labeling") == ("rpca", "thresh", "labels")
    for bad in (["rpcaa"], ["crop"], ["A"], "rpca;thresh", [""]):
        with pytest.raises(ValueError):
            review.stage_keys(bad)


def test_unknown_stage_and_too_few_styles(tmp_path):
    from swiftwatcher_amd import review
    with pytest.raises(ValueError):
        _writer(tmp_path, stages=("rpca", "canny"))
    four = review.DEFAULT_STYLES[:4]
    _writer(tmp_path, styles=four).close()
    with pytest.raises(ValueError):
        _writer(tmp_path, styles=four, stages=("rpca",))
    for kw in (dict(stage_gain={"rpca": 0}), dict(stage_gain={"rpca": 256}), dict(stage_gain={"RPCA": 2}), dict(stage_layers=16), dict(stage_layers=-1),
               dict(stage_cols=0), dict(stage_cols=17), dict(stages=("gray",) * 16)):
        with pytest.raises(ValueError):
            _writer(tmp_path, stages=kw.pop("stages", ("rpca",)), **kw)


def test_default_columns_and_sizes(tmp_path):
    from swiftwatcher_amd import review
    assert review.default_stage_cols(212, 424, 4) == 1 and review.default_stage_cols(424, 212, 4) == 4 and review.default_stage_cols(64, 64, 3) == 3
    with _writer(tmp_path) as w:                                             # no stages: the frame is the crop
        assert (w.frame_height, w.frame_width, w.height, w.width, w.stages) == (120, 300, 120, 300, ())
    with _writer(tmp_path, stages=("rpca", "thresh", "labels")) as w:         # wider than high: one column
        assert (w.stage_cols, w.frame_height, w.frame_width, w.height, w.width) == (1, 480, 300, 120, 300)
        assert w.cell_origins == [(0, 0), (120, 0), (240, 0), (360, 0)]
    with _writer(tmp_path, size=(95, 121), stages=("rpca", "labels")) as w:   # higher than wide, odd: one row of padded cells
        assert (w.stage_cols, w.frame_height, w.frame_width, w.height, w.width) == (3, 122, 288, 121, 95)
    with _writer(tmp_path, stages=("rpca", "thresh", "labels"), stage_cols=2) as w:
        assert (w.frame_height, w.frame_width) == (240, 600)


def test_y4m_header_carries_the_mosaic_size(tmp_path):
    with _writer(tmp_path, size=(95, 121), stages=("rpca", "labels")) as w:
        assert w._frame_bytes == 6 + 122 * 288 * 3 // 2
    assert open(str(tmp_path / "review.y4m"), "rb").readline().startswith(b"YUV4MPEG2 W288 H122 ")
    with _writer(tmp_path, size=(95, 121)):
        pass
    assert open(str(tmp_path / "review.y4m"), "rb").readline().startswith(b"YUV4MPEG2 W95 H121 ")


def test_captions_and_gains(tmp_path):
    from swiftwatcher_amd import review
    assert review.DEFAULT_STAGE_GAIN == {"gray": 1, "rpca": 4, "bilateral": 4, "thresh": 4, "opened": 4, "labels": 1}
    assert [review.stage_caption(k, g) for k, g in (("rpca", 4), ("gray", 1), ("labels", 1), ("labels", 9), ("thresh", 12), ("opened", 1))] == \
        ["RPCA X4", "GRAY", "LABELS", "LABELS", "THRESH X12", "OPENED"]
    assert all(b in tref.CHARSET for k in review.DEFAULT_STAGE_GAIN for b in review.stage_caption(k, 255).encode("ascii"))
    frames = [SimpleNamespace(frame_number=k, processed_frames={name: np.full((120, 300), 10 * k + j, np.uint8) for j, name in
                                                                enumerate(("grayscale", "RPCA", "bilateral", "thresh_15", "opened", "cc_labeling"))})
              for k in range(3)]
    with _writer(tmp_path, stages=("gray", "rpca", "cc_labeling", "rpca"), stage_gain={"rpca": 7}, text_scale=2, stage_layers=6) as w:
        panels, held = w.plan_panels(frames)
    assert held is None and [p["kind"] for p in panels] == ["gray", "gray", "labels", "gray"] and [p["gain"] for p in panels] == [1, 7, 1, 7]
    assert all(p["layers"] == 6 for p in panels)
    # style 5 on plate 6 at the writer's scale, ink origin BORDER + scale both ways
    assert [p["caption"] for p in panels] == [(5, 5, 5, 6, 2, "GRAY"), (5, 5, 5, 6, 2, "RPCA X7"), (5, 5, 5, 6, 2, "LABELS"), (5, 5, 5, 6, 2, "RPCA X7")]
    # the host path: processed_frames stacked in the frames' order
    assert all(p["plane"].shape == (3, 120, 300) and p["plane"].dtype == np.uint8 for p in panels)
    assert [int(p["plane"][k, 0, 0]) for p in panels for k in range(3)] == [0, 10, 20, 1, 11, 21, 5, 15, 25, 1, 11, 21]


class _Planes:
    """Stands in for _lib.DevicePlanes."""

    def __init__(self, stages, F, Hc, Wc, ptr=1 << 20):
        self.stages, self.F, self.Hc, self.Wc, self.ptr = stages, F, Hc, Wc, ptr

    def pointer(self, stage):
        return self.ptr + self.stages.index(stage) * self.F * self.Hc * self.Wc


def test_device_path_takes_the_planes_where_they_lie(tmp_path):
    """Popped frame k of a queue of n carries index n - 1 - k: the oldest frame's plane and a negative frame stride; null frames (the
    newest) are not among the written frames.  Anything else -- other planes, a missing stage, uneven steps -- is the host path."""
    from swiftwatcher_amd import _lib
    n, H, W = 21, 120, 300
    planes = _Planes(("rpca", "thresh", "labels"), 2 * n, H, W)
    host = {name: np.zeros((H, W), np.uint8) for name in ("RPCA", "thresh_15", "cc_labeling", "grayscale")}

    def frames(indices, p=planes):
        return [SimpleNamespace(frame_number=k, stage_planes=None if i is None else (p, i), processed_frames=host) for k, i in enumerate(indices)]
    with _writer(tmp_path, stages=("thresh", "labels")) as w:
        written = frames([n + n - 1 - k for k in range(n - 4)])               # the second window of a batch of two, four null frames at its end
        panels, held = w.plan_panels(written)
        assert held is planes
        image = H * W
        assert [p["plane"] for p in panels] == [
            {"ptr": planes.pointer("thresh") + (2 * n - 1) * image, "frame_stride": -image, "row_stride": W, "mem": _lib.MEM_DEVICE},
            {"ptr": planes.pointer("labels") + (2 * n - 1) * image, "frame_stride": -image, "row_stride": W, "mem": _lib.MEM_DEVICE}]
        one, held = w.plan_panels(frames([7]))
        assert held is planes and one[0]["plane"]["ptr"] == planes.pointer("thresh") + 7 * image and one[0]["plane"]["frame_stride"] == 0
        up, held = w.plan_panels(frames([3, 5, 7]))
        assert held is planes and up[0]["plane"]["frame_stride"] == 2 * image
        other = frames([5, 4, 3])
        other[1].stage_planes = (_Planes(("rpca", "thresh", "labels"), 2 * n, H, W), 4)
        for fallback in (frames([5, 4, 2]), frames([5, None, 3]), other, frames([5, 4, 3], _Planes(("rpca", "thresh"), 2 * n, H, W)),
                         frames([5, 4, 3], _Planes(("rpca", "thresh", "labels"), 2 * n, H, W + 2))):
            panels, held = w.plan_panels(fallback)
            assert held is None and all(isinstance(p["plane"], np.ndarray) and p["plane"].shape == (3, H, W) for p in panels)


def test_render_goes_through_the_panels_call(tmp_path, monkeypatch):
    """write_window with stages: one render_review_panels call with the plan's overlay, the panels and the columns, into a destination
    of the mosaic's strides; without stages the call stays render_review."""
    from swiftwatcher_amd import _lib, data_structures, review
    H, W = 120, 300
    calls = []

    class Ctx:
        _lib = SimpleNamespace(swk_device_read=lambda *a: 0)
        _h = None
        staging = None

        def device_alloc(self, n):
            return 1 << 12

        def device_free(self, p):
            pass

        def _check(self, rc):
            assert rc == 0

        def render_review(self, stack, **kw):
            calls.append(("review", kw))

        def render_review_panels(self, stack, **kw):
            calls.append(("panels", kw))
    monkeypatch.setattr(_lib, "default_context", lambda device=0: Ctx())
    monkeypatch.setattr(_lib, "pinned_empty", lambda shape, dtype=np.uint8, device=0: np.zeros(shape, dtype))
    monkeypatch.setattr(data_structures, "stack_frames", lambda frames, crop, m, buf, dev=0: (np.zeros((len(frames), H, W, 3), np.uint8), (0, 0), (H, W), False))
    stages = {name: np.zeros((H, W), np.uint8) for name in ("RPCA", "cc_labeling")}
    popped = [SimpleNamespace(frame_number=k, frame=None, timestamp="t", segments=[], processed_frames=stages) for k in (0, 1, -1)]
    with _writer(tmp_path, stages=("rpca", "labels"), text=True) as w:
        w.write_window(popped)
        assert w.frames == 2
    with _writer(tmp_path) as w:
        w.write_window(popped)
    (kind, kw), (plain_kind, plain_kw) = calls
    assert kind == "panels" and plain_kind == "review" and "panels" not in plain_kw and "cols" not in plain_kw
    assert kw["cols"] == 1 and [p["caption"][5] for p in kw["panels"]] == ["RPCA X4", "LABELS"] and len(kw["labels"]) == 2
    fb = 6 + 360 * 300 * 3 // 2
    assert (kw["dst"].y_row_stride, kw["dst"].c_row_stride, kw["dst"].y_frame_stride, kw["dst"].c_frame_stride) == (300, 150, fb, fb)
    assert kw["dst"].u - kw["dst"].y == 360 * 300 and kw["dst"].v - kw["dst"].u == 180 * 150
    assert (plain_kw["dst"].y_row_stride, plain_kw["dst"].y_frame_stride) == (300, 6 + 120 * 300 * 3 // 2)
    assert kw["rect"] == plain_kw["rect"] == (0, 0, W, H)
    assert os.path.getsize(str(tmp_path / "review.y4m")) > 0 and review.STYLE_TEXT == 5 and review.STYLE_PLATE == 6


def test_segmenters_and_loops_take_the_stages():
    """The arguments exist where the issue puts them (what they do needs the GPU: tests/test_review_stages_gpu.py)."""
    import inspect
    from swiftwatcher_amd import _lib, data_structures, pipeline
    assert inspect.signature(data_structures.segment_windows).parameters["stages"].default == ()
    assert inspect.signature(data_structures.segment_window_groups).parameters["stages"].default == ()
    assert inspect.signature(_lib.Context.batch_run_groups).parameters["device_stages"].default is False
    for fn in (pipeline.swift_counting_algorithm, pipeline.count_swifts, pipeline.count_swifts_videos):
        assert inspect.signature(fn).parameters["review_stages"].default == ()
    assert data_structures.Frame(None, 3).stage_planes is None
    w = SimpleNamespace(stages=("rpca", "labels", "rpca"))
    assert pipeline._review_stages([None, w, SimpleNamespace(stages=("thresh", "labels")), object()]) == ("rpca", "labels", "thresh")


# ------------------------------------------------------------------------------------------ the command line
def test_command_line(capsys):
    from swiftwatcher_amd.__main__ import plan
    base = ["clip.y4m", "--corners", "1,2,3,4"]
    args, _ = plan(base + ["--review", "r.y4m", "--review-stages", "rpca,thresh,labels"])
    assert args.review_stages == ("rpca", "thresh", "labels") and not args.review_text
    args, _ = plan(base + ["--review", "r.y4m", "--review-text", "--review-stages", "RPCA,cc_labeling"])          # the two combine
    assert args.review_stages == ("rpca", "labels") and args.review_text
    assert plan(base + ["--review", "r.y4m"])[0].review_stages == ()
    for bad in (["--review-stages", "rpca"], ["--review", "r.y4m", "--review-stages", "rpca,canny"]):
        with pytest.raises(SystemExit) as exc:
            plan(base + bad)
        assert exc.value.code == 2
    err = capsys.readouterr().err
    assert "--review-stages needs --review" in err and "unknown stage 'canny'" in err
