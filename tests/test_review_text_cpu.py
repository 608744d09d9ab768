"""The review video's text without a GPU: the declarations, the record's layout, the font table, and what ReviewWriter plans with
text=True (status line, scale, positions, event ordinals across windows, clamping) with the render call stubbed."""
import datetime
import os
import re
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import review_text_ref as tref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------ declarations and layout
def test_header_declares_the_struct_and_both_functions():
    from swiftwatcher_amd import _lib
    header = open(os.path.join(ROOT, "include", "swk.h")).read()
    assert re.search(r"}\s*swk_review_label\s*;", header)
    assert re.search(r"int32_t\s+swk_render_review_labels\s*\(", header) and re.search(r"void\s+swk_review_font\s*\(", header)
    assert "swk_render_review_labels" in _lib.EXPORTS and "swk_review_font" in _lib.EXPORTS
    assert _lib.ABI_VERSION == 2 and "#define SWK_ABI_VERSION 2" in header


def test_label_dtype_matches_the_header(tmp_path):
    """REVIEW_LABEL_DTYPE against the C compiler's layout of swk_review_label: size and every field's offset."""
    from swiftwatcher_amd import _lib
    fields = ["frame", "r", "c", "style", "plate", "scale", "len", "reserved_", "text"]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "swk.h"\nint main(){printf("%zu", sizeof(swk_review_label));\n'
                   + "".join('printf(" %%zu", offsetof(swk_review_label, %s));\n' % f for f in fields) + "return 0;}")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "sz")])
    got = [int(v) for v in subprocess.check_output([str(tmp_path / "sz")]).split()]
    dt = _lib.REVIEW_LABEL_DTYPE
    assert got == [dt.itemsize] + [dt.fields[f][1] for f in fields] and dt.itemsize == 64
    assert dt.fields["text"][0].shape == (32,) and dt.fields["text"][0].base == np.uint8
    rec = _lib.label_records([(3, -4, 5, 1, 2, 8, "AB #1"), (4, 0, 0, 0, 0, 1, b"")])
    assert rec.dtype == dt and rec["len"].tolist() == [5, 0] and bytes(rec["text"][0][:5]) == b"AB #1" and rec["frame"].tolist() == [3, 4]
    assert (rec["r"][0], rec["c"][0], rec["style"][0], rec["plate"][0], rec["scale"][0]) == (-4, 5, 1, 2, 8)
    with pytest.raises(ValueError):
        _lib.label_records([(0, 0, 0, 1, 1, 1, "A" * 33)])


# ------------------------------------------------------------------------------------------ the font
def test_font_table():
    from swiftwatcher_amd import _lib
    font = _lib.review_font()
    assert font.shape == (128, 8) and font.dtype == np.uint8
    assert len(tref.CHARSET) == 45 == len(set(tref.CHARSET))
    assert [ch for ch in range(128) if font[ch, 7]] == sorted(tref.CHARSET) and set(font[:, 7].tolist()) == {0, 1}
    assert not font[[ch for ch in range(128) if ch not in tref.CHARSET]].any()          # rows of zeros outside the set
    assert not (font[:, :7] & 0xE0).any()                                               # no ink outside 5 columns (rows: 7 by layout)
    assert not font[ord(" "), :7].any()
    glyphs = {ch: bytes(font[ch, :7]) for ch in tref.CHARSET}
    assert all(any(g) for ch, g in glyphs.items() if ch != ord(" "))
    assert len(set(glyphs.values())) == 45                                              # pairwise distinct
    # a letter's shape, bit 4 = the leftmost column: T is a bar over a stem
    assert font[ord("T"), :7].tolist() == [0x1F] + [0x04] * 6 and font[ord("L"), :7].tolist() == [0x10] * 6 + [0x1F]


# ------------------------------------------------------------------------------------------ the status line
def test_status_line_text():
    from swiftwatcher_amd import review
    t = datetime.datetime(1900, 1, 1, 1, 2, 3, 456789)
    assert review.status_text(123, t, 3, 1, 7) == "F000123 01:02:03.456 S03 R01 E007"
    assert len(review.status_text(0, t, 0, 0, 0)) == review.STATUS_CELLS == 33
    assert review.status_text(1234567, t, 100, 123, 1000) == "F1234567 01:02:03.456 S100 R123 E1000"          # fields widen
    assert review.status_text(5, "00:00:00.167", 0, 0, 0) == "F000005 00:00:00.167 S00 R00 E000"
    assert review.status_text(5, "ts00005", 0, 0, 0) == "F000005 TS00005 S00 R00 E000"                         # no strftime: upper-cased
    assert review.stamp_text("a_b,c 12:30:00.123456") == "A B C 12:30:"                                        # cut to 12, others to spaces
    assert all(b in tref.CHARSET for b in review.stamp_text("éx(y)").encode("ascii"))


@pytest.mark.parametrize("size,scale", [((424, 212), 2), ((850, 425), 4), ((94, 47), 1)])
def test_default_scale(tmp_path, size, scale):
    from swiftwatcher_amd.review import ReviewWriter, text_scale_for
    W, H = size
    assert text_scale_for(W, H, ReviewWriter.BORDER) == scale
    with ReviewWriter(str(tmp_path / "s.y4m"), [(0, 0), (W, H)], np.zeros((H, W), np.uint8), 30, text=True) as w:
        assert w.text_scale == scale
    with ReviewWriter(str(tmp_path / "s.y4m"), [(0, 0), (W, H)], np.zeros((H, W), np.uint8), 30, text=True, text_scale=3) as w:
        assert w.text_scale == 3
    with pytest.raises(ValueError):
        ReviewWriter(str(tmp_path / "t.y4m"), [(0, 0), (W, H)], np.zeros((H, W), np.uint8), 30, text=True, text_scale=9)


def test_styles_of_four_rows_need_text_off(tmp_path):
    from swiftwatcher_amd import review
    four = review.DEFAULT_STYLES[:4]
    assert review.DEFAULT_STYLES[4] == (255, 255, 255, 0, 256) and review.DEFAULT_STYLES[5] == (0, 0, 0, 160, 0) and len(review.DEFAULT_STYLES) == 6
    review.ReviewWriter(str(tmp_path / "a.y4m"), [(0, 0), (8, 6)], np.zeros((6, 8), np.uint8), 30, styles=four).close()
    with pytest.raises(ValueError):
        review.ReviewWriter(str(tmp_path / "b.y4m"), [(0, 0), (8, 6)], np.zeros((6, 8), np.uint8), 30, styles=four, text=True)


# ------------------------------------------------------------------------------------------ what the writer plans
def _segment(number, centroid, bbox=(1, 2, 3, 4)):
    return SimpleNamespace(parent_frame_number=number, centroid=centroid, bbox=bbox)


def _window(first, count, nulls=0, segments=None):
    frames = [SimpleNamespace(frame_number=first + k, frame=None, timestamp="00:00:%02d.000" % (first + k), segments=(segments or {}).get(first + k, []))
              for k in range(count)]
    return frames + [SimpleNamespace(frame_number=-1, frame=None, timestamp="", segments=[]) for _ in range(nulls)]


W, H, HOLD = 300, 120, 4


def _writer(tmp_path, **kw):
    from swiftwatcher_amd.review import ReviewWriter
    w = ReviewWriter(str(tmp_path / "review.y4m"), [(10, 20), (10 + W, 20 + H)], np.zeros((H, W), np.uint8), 30, event_hold=HOLD, **kw)
    w.calls = []

    def render(frames, boxes, marks, frame_style, **more):
        w.calls.append((tuple(f.frame_number for f in frames), list(boxes), list(marks), list(frame_style), more))
        out = np.full((len(frames), w._frame_bytes), 128, np.uint8)
        out[:, :6] = np.frombuffer(b"FRAME\n", np.uint8)
        return out.ravel()
    w._render = render
    return w


def _split(labels, k):
    """(status labels, event labels) of written frame k."""
    mine = [lab for lab in labels if lab[0] == k]
    return [lab for lab in mine if lab[3] == 5], [lab for lab in mine if lab[3] != 5]


def _line(labels, k):
    """The status line of written frame k, its labels joined."""
    return "".join(lab[6] for lab in _split(labels, k)[0])


def test_status_line_position_and_split(tmp_path):
    from swiftwatcher_amd.review import ReviewWriter
    w = _writer(tmp_path, text=True)
    s, B = w.text_scale, ReviewWriter.BORDER
    assert s == 1 and B == 3
    seg = _segment(2, (5.0, 5.0))
    w.write_window(_window(0, 3, nulls=1, segments={2: [seg, seg]}), [None, [(0, 0, 2, 2), (1, 1, 3, 3)], None, None], [])
    numbers, boxes, marks, style, more = w.calls[-1]
    assert numbers == (0, 1, 2) and set(more) == {"labels"}
    labels = more["labels"]
    for k, text in enumerate(["F000000 00:00:00.000 S00 R00 E000", "F000001 00:00:01.000 S00 R02 E000", "F000002 00:00:02.000 S02 R00 E000"]):
        status, events = _split(labels, k)
        assert not events
        # 33 bytes: a label of 32 and one of 1, on one row, 6 * scale * 32 pixels apart; style 5 on plate 6
        assert status == [(k, H - B - 8 * s, B + s, 5, 6, s, text[:32]), (k, H - B - 8 * s, B + s + 6 * s * 32, 5, 6, s, text[32:])]
    # the rectangle's bottom row is the last row above the border, its left column the first right of it
    r, c = labels[0][1], labels[0][2]
    assert r + 8 * s == H - B and c - s == B
    assert [lab[0] for lab in labels] == sorted(lab[0] for lab in labels)          # ascending frame
    w.close()
    w3 = _writer(tmp_path, text=True, text_scale=3)
    w3.write_window(_window(7, 1), None, [])
    assert w3.calls[-1][4]["labels"][0][:3] == (0, H - B - 24, B + 3) and w3.calls[-1][4]["labels"][1][2] == B + 3 + 6 * 3 * 32
    w3.close()


def test_event_ordinals_and_counts_over_three_windows(tmp_path):
    """event_hold = 4, as test_review_cpu.test_event_scheduling: ordinals follow the order the writer received the events and travel
    with the hold into the next window; E counts the events whose first shown frame is at or before the frame."""
    w = _writer(tmp_path, text=True)
    s, arm = w.text_scale, w.MARK_ARM
    # window 1, frames 0..4: event 1 (last segment on frame 2) shows on frames 3, 4 (5, 6)
    ev1 = [_segment(1, (10.4, 20.6)), _segment(2, (30.5, 40.0))]
    w.write_window(_window(0, 5), None, [ev1])
    labels = w.calls[-1][4]["labels"]
    assert [_line(labels, k)[-4:] for k in range(5)] == ["E000", "E000", "E000", "E001", "E001"]
    assert [_split(labels, k)[1] for k in range(3)] == [[], [], []]
    want1 = (31 + arm + 2 * s, 40 + arm + 2 * s, 3, 6, s, "#1")          # from the event's last centroid, rounded half up
    assert [_split(labels, k)[1] for k in (3, 4)] == [[(3,) + want1], [(4,) + want1]]
    # window 2, frames 5..9: the hold crosses the window's end (5, 6); events 2 and 3 arrive together, 2 (last segment on frame 6)
    # shows on 7..10, 3 (last segment on frame 9) from frame 10: not in this window, and not counted by E before frame 10
    ev2, ev3 = [_segment(6, (50.0, 60.0))], [_segment(8, (1.0, 1.0)), _segment(9, (70.0, 80.0))]
    w.write_window(_window(5, 5), None, [ev2, ev3])
    labels = w.calls[-1][4]["labels"]
    assert [_line(labels, k)[-4:] for k in range(5)] == ["E001", "E001", "E002", "E002", "E002"]
    want2 = (50 + arm + 2 * s, 60 + arm + 2 * s, 3, 6, s, "#2")
    assert [[lab[1:] for lab in _split(labels, k)[1]] for k in range(5)] == [[want1], [want1], [want2], [want2], [want2]]
    # window 3, frames 10..12 and null frames: event 2's hold ends on frame 10, event 3 shows on 10..13: both on frame 10, in the
    # order received; event 4 (last segment on frame 12) points at frame 13: not shown and not counted in this window
    ev4 = [_segment(12, (2.0, 2.0))]
    w.write_window(_window(10, 3, nulls=2), None, [ev4])
    numbers, _, marks, style, more = w.calls[-1]
    labels = more["labels"]
    want3 = (70 + arm + 2 * s, 80 + arm + 2 * s, 3, 6, s, "#3")
    assert numbers == (10, 11, 12)
    assert [_line(labels, k)[-4:] for k in range(3)] == ["E003", "E003", "E003"]
    assert [[lab[1:] for lab in _split(labels, k)[1]] for k in range(3)] == [[want2, want3], [want3], [want3]]
    # a later event keeps counting from where the writer is: ordinal 5
    w.write_window(_window(13, 2), None, [[_segment(12, (5.0, 5.0))]])
    labels = w.calls[-1][4]["labels"]
    assert [lab[6] for lab in _split(labels, 0)[1]] == ["#3", "#4", "#5"] and _line(labels, 0)[-4:] == "E005"
    w.close()


def test_event_numbers_are_clamped_inside_the_border(tmp_path):
    from swiftwatcher_amd.review import ReviewWriter
    w = _writer(tmp_path, text=True, text_scale=2)
    s, B, arm = 2, ReviewWriter.BORDER, ReviewWriter.MARK_ARM
    points = {"middle": (50, 100), "top-left": (-30, -30), "top": (-20, 100), "left": (50, -20), "bottom": (H - 1, 100), "right": (50, W - 1),
              "bottom-right": (H + 40, W + 40)}
    events = [[_segment(0, (float(r), float(c)))] for r, c in points.values()]
    w.write_window(_window(1, 1), None, events)
    got = {name: lab for name, lab in zip(points, _split(w.calls[-1][4]["labels"], 0)[1])}
    lo_r, hi_r, lo_c, hi_c = B + s, H - B - 8 * s, B + s, W - B - 6 * s * 2
    assert got["middle"][1:3] == (50 + arm + 2 * s, 100 + arm + 2 * s)
    assert got["top-left"][1:3] == (lo_r, lo_c)
    assert got["top"][1:3] == (lo_r, 100 + arm + 2 * s) and got["left"][1:3] == (50 + arm + 2 * s, lo_c)
    assert got["bottom"][1:3] == (hi_r, 100 + arm + 2 * s)
    assert got["right"][1:3] == (50 + arm + 2 * s, hi_c)
    assert got["bottom-right"][1:3] == (hi_r, hi_c)
    for lab in got.values():                      # the rectangle inside the border
        r, c, n = lab[1], lab[2], len(lab[6])
        assert r - s >= B and r + 8 * s <= H - B and c - s >= B and c + 6 * s * n <= W - B
    w.close()
    # ten events: "#10" is three cells wide
    w = _writer(tmp_path, text=True, text_scale=2)
    w.write_window(_window(1, 1), None, [[_segment(0, (50.0, float(W)))] for _ in range(10)])
    last = _split(w.calls[-1][4]["labels"], 0)[1][-1]
    assert last[6] == "#10" and last[2] == W - B - 6 * s * 3
    w.close()
    # a frame too small for the label: its top-left side stays inside
    from swiftwatcher_amd.review import ReviewWriter as RW
    small = RW(str(tmp_path / "small.y4m"), [(0, 0), (12, 10)], np.zeros((10, 12), np.uint8), 30, text=True)
    small.plan_window(_window(1, 1), None, [[_segment(0, (9.0, 11.0))]])
    plan = small.plan_window(_window(2, 1), None, [])
    assert [lab[1:3] for lab in small.plan_labels(plan) if lab[3] == 3] == [(B + 1, B + 1)]
    small.close()


def test_text_off_plans_no_labels_and_calls_as_before(tmp_path, monkeypatch):
    """A writer without text hands _render its four positional arguments and nothing else, and the library gets swk_render_review's
    call (no labels keyword); with text the same plan comes with labels."""
    from swiftwatcher_amd import _lib, review
    w = _writer(tmp_path)
    assert w.text is False
    ev = [_segment(1, (10.0, 20.0))]
    w.write_window(_window(0, 4), None, [ev])
    plain = w.calls[-1]
    assert plain[4] == {}
    w.close()
    t = _writer(tmp_path, text=True)
    t.write_window(_window(0, 4), None, [ev])
    assert t.calls[-1][:4] == plain[:4] and len(t.calls[-1][4]["labels"]) == 4 * 2 + 2
    t.close()
    # the library call: render_review's keywords with text off are exactly the earlier ones
    seen = []

    class Ctx:
        staging = None

        def device_alloc(self, n):
            return 4096

        def device_free(self, p):
            pass

        def render_review(self, stack, **kw):
            seen.append(sorted(kw))

        def _check(self, rc):
            pass
        _lib = SimpleNamespace(swk_device_read=lambda *a: 0)
        _h = None

    import swiftwatcher_amd.data_structures as ds
    monkeypatch.setattr(_lib, "default_context", lambda device=0: Ctx())
    monkeypatch.setattr(_lib, "pinned_empty", lambda shape, dtype, device=0: np.zeros(shape, dtype))
    monkeypatch.setattr(ds, "stack_frames", lambda frames, crop, origin, staging, device: (np.zeros((len(frames), 6, 8, 3), np.uint8), (0, 0), (6, 8), False))
    for text in (False, True):
        rw = review.ReviewWriter(str(tmp_path / "kw.y4m"), [(0, 0), (8, 6)], np.zeros((6, 8), np.uint8), 30, text=text)
        rw.write_window(_window(0, 2), None, [])
        rw._dev = 0
        rw.close()
    before = ["border", "boxes", "dst", "frame_style", "mark_arm", "marks", "mask", "mask_style", "rect", "styles"]
    assert seen == [before, sorted(before + ["labels"])]


# ------------------------------------------------------------------------------------------ the command line
def test_cli_review_text_needs_review(capsys):
    from swiftwatcher_amd.__main__ import build_parser, plan
    args = build_parser().parse_args(["night.y4m", "--corners", "1,2,3,4", "--review", "r.y4m", "--review-text"])
    assert args.review_text is True and build_parser().parse_args(["night.y4m"]).review_text is False
    with pytest.raises(SystemExit) as exc:
        plan(["night.y4m", "--corners", "1,2,3,4", "--review-text"])
    assert exc.value.code == 2
    assert "--review-text" in capsys.readouterr().err
    args, jobs = plan(["night.y4m", "--corners", "1,2,3,4", "--review", "r.y4m", "--review-text"])
    assert args.review_text and jobs == [("night.y4m", ((1, 2), (3, 4)))]


def test_pipeline_entry_points_take_review_text():
    import inspect
    from swiftwatcher_amd import pipeline
    for fn in (pipeline.swift_counting_algorithm, pipeline.count_swifts, pipeline.count_swifts_videos):
        assert inspect.signature(fn).parameters["review_text"].default is False


# ------------------------------------------------------------------------------------------ the restatement itself
def test_restatement_draws_a_glyph_by_the_definition():
    """One 'T' at scale 2 on a gray frame: ink where the definition says, the plate on the rest of the rectangle, nothing outside."""
    from swiftwatcher_amd import _lib
    font = _lib.review_font()
    frame = np.full((1, 24, 20, 3), 100, np.uint8)
    styles = [(255, 255, 255, 0, 256), (0, 0, 0, 128, 0)]
    out = tref.compose(frame, labels=[(0, 4, 3, 1, 2, 2, "T")], font=font, styles=styles)[0, :, :, 0]
    want = np.full((24, 20), 100, np.int64)
    want[2:20, 1:15] = 50                          # rows [r - s, r + 8 s) = [2, 20), columns [c - s, c + 6 s) = [1, 15): the plate
    want[4:6, 3:13] = 255                          # the bar: glyph row 0, columns 0..4, doubled
    want[6:18, 7:9] = 255                          # the stem: glyph rows 1..6, column 2
    assert np.array_equal(out, want)
    assert np.array_equal(tref.compose(frame, labels=[(0, 4, 3, 1, 2, 2, "")], font=font, styles=styles)[0, :, :, 0], np.full((24, 20), 100))
