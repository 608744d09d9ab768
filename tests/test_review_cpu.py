"""The review video without a GPU: the test-side restatement (tests/review_ref.py) against hand vectors and against the library's own
inverse conversion, the declarations, the command line, and ReviewWriter's event scheduling with the render call stubbed."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import review_ref as ref
import yuv_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------ the restatement
def test_hand_vectors():
    assert len(ref.HAND_VECTORS) == 8
    for (b, g, r), want in ref.HAND_VECTORS:
        assert tuple(int(x) for x in ref.yuv_pixels(b, g, r)) == want


def test_round_trip_through_the_inverse_conversion():
    """A strided sample of colours (every 5th value of each channel, and the extremes): Y in 16..235, U and V in 16..240, and back
    through yuv_ref.pixels (swk_yuv420_to_bgr's formula) within 2 in B and R and 1 in G."""
    axis = np.unique(np.concatenate([np.arange(0, 256, 5), [1, 254, 255]]))
    B, G, R = (a.ravel() for a in np.meshgrid(axis, axis, axis, indexing="ij"))
    Y, U, V = ref.yuv_pixels(B, G, R)
    assert Y.min() >= 16 and Y.max() <= 235 and U.min() >= 16 and U.max() <= 240 and V.min() >= 16 and V.max() <= 240
    b, g, r = yuv_ref.pixels(Y, U, V)
    assert np.abs(b - B).max() <= 2 and np.abs(r - R).max() <= 2 and np.abs(g - G).max() <= 1


def test_blend_ends():
    p, col = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    assert np.array_equal(ref.blend(p, col, 0), p)
    assert np.array_equal(ref.blend(p, col, 256), col)
    assert int(ref.blend(10, 250, 128)) == 130 and int(ref.blend(0, 255, 1)) == 1 and int(ref.blend(255, 0, 255)) == 1


def test_layers_apply_in_order():
    """Mask, boxes in array order, marks, border: a pixel under all four takes the four blends in that order."""
    frame = np.full((1, 6, 8, 3), 100, np.uint8)
    styles = [(0, 0, 0, 128, 64), (200, 200, 200, 128, 32)]
    got = ref.compose(frame, boxes=[(0, 0, 0, 3, 3, 1), (0, 0, 0, 6, 8, 2)], marks=[(0, 0, 0, 1)], frame_style=[2], mask=np.ones((6, 8)),
                      styles=styles, mask_style=1, mark_arm=0, border=1)
    want = 100
    for col, a in ((0, 128), (0, 64), (200, 32), (0, 64), (200, 32)):          # mask fill, box 1 edge, box 2 edge, mark line, border line
        want = (want * (256 - a) + col * a + 128) >> 8
    assert got[0, 0, 0].tolist() == [want] * 3
    assert got[0, 1, 1, 0] == ref.blend(ref.blend(ref.blend(100, 0, 128), 0, 128), 200, 128)          # mask, box 1 fill, box 2 fill


# ------------------------------------------------------------------------------------------ declarations
def test_header_and_binding_declare_both_symbols():
    from swiftwatcher_amd import _lib
    header = open(os.path.join(ROOT, "include", "swk.h")).read()
    for name in ("swk_bgr_to_yuv420", "swk_render_review"):
        assert re.search(r"int32_t\s+%s\s*\(" % name, header)
        assert name in _lib.EXPORTS
    for struct in ("swk_yuv420_dst", "swk_review_style", "swk_review_box", "swk_review_mark", "swk_review"):
        assert re.search(r"}\s*%s\s*;" % struct, header)
    assert "PARITY UNPINNED" in header[header.index("review video"):]
    assert _lib.ABI_VERSION == 2
    assert "review.hip" in open(os.path.join(ROOT, "swiftwatcher_amd", "csrc", "build.py")).read()


def test_cli_takes_review_and_refuses_standard_output(capsys):
    from swiftwatcher_amd.__main__ import build_parser
    args = build_parser().parse_args(["night.y4m", "--corners", "1,2,3,4", "--review", "night_review.y4m"])
    assert args.review == "night_review.y4m"
    assert build_parser().parse_args(["night.y4m"]).review is None
    with pytest.raises(SystemExit) as exc:
        build_parser().parse_args(["night.y4m", "--corners", "1,2,3,4", "--review", "-"])
    assert exc.value.code == 2
    assert "--review" in capsys.readouterr().err


# ------------------------------------------------------------------------------------------ ReviewWriter's scheduling
def _segment(number, centroid, bbox=(1, 2, 3, 4)):
    return SimpleNamespace(parent_frame_number=number, centroid=centroid, bbox=bbox)


def _window(first, count, nulls=0, segments=None):
    frames = [SimpleNamespace(frame_number=first + k, frame=None, segments=(segments or {}).get(first + k, [])) for k in range(count)]
    return frames + [SimpleNamespace(frame_number=-1, frame=None, segments=[]) for _ in range(nulls)]


@pytest.fixture
def writer(tmp_path):
    from swiftwatcher_amd.review import ReviewWriter
    calls = []
    w = ReviewWriter(str(tmp_path / "review.y4m"), [(10, 20), (18, 26)], np.zeros((6, 8), np.uint8), 30, event_hold=4)

    def render(frames, boxes, marks, frame_style):
        calls.append((tuple(f.frame_number for f in frames), list(boxes), list(marks), list(frame_style)))
        out = np.full((len(frames), w._frame_bytes), 128, np.uint8)          # (gray frames, each behind its FRAME mark like the real render's)
        out[:, :6] = np.frombuffer(b"FRAME\n", np.uint8)
        return out.ravel()
    w._render = render
    w.calls = calls
    yield w
    w.close()


def test_event_scheduling(writer):
    """event_hold = 4.  An event whose segment vanished on the last frame of a window shows on the next window's first four frames; a
    hold that crosses a window's end carries over; one that points past the last written frame is dropped."""
    from swiftwatcher_amd.review import STYLE_EVENT, STYLE_REJECTED, STYLE_SEGMENT
    seg = _segment(3, (2.5, 4.49), bbox=(0, 1, 5, 6))
    # window 1: frames 0..4; the tracker found an event on frame 3 (its last segment is on frame 2): frames 3, 4 (and 5, 6)
    ev_a = [_segment(1, (0.4, 0.6)), _segment(2, (1.5, 7.0))]
    writer.write_window(_window(0, 5, segments={3: [seg]}), [None, [(0, 0, 2, 2)], None, [], None], [ev_a])
    numbers, boxes, marks, style = writer.calls[-1]
    assert numbers == (0, 1, 2, 3, 4)
    assert boxes == [(1, 0, 0, 2, 2, STYLE_REJECTED), (3, 0, 1, 5, 6, STYLE_SEGMENT)]
    assert style == [0, 0, 0, STYLE_EVENT, STYLE_EVENT]
    assert marks == [(3, 0, 1, STYLE_EVENT), (3, 2, 7, STYLE_EVENT), (4, 0, 1, STYLE_EVENT), (4, 2, 7, STYLE_EVENT)]          # rounded half up
    # window 2: frames 5..9; event A's hold crosses into it (5, 6); event B vanished on frame 9, the window's last: nothing yet
    writer.write_window(_window(5, 5), None, [])
    numbers, boxes, marks, style = writer.calls[-1]
    assert numbers == (5, 6, 7, 8, 9) and boxes == [] and style == [STYLE_EVENT, STYLE_EVENT, 0, 0, 0]
    assert marks == [(0, 0, 1, STYLE_EVENT), (0, 2, 7, STYLE_EVENT), (1, 0, 1, STYLE_EVENT), (1, 2, 7, STYLE_EVENT)]
    # window 3: frames 10..12 and two null frames; event B (last segment on frame 9) is found on frame 10: frames 10..13, 13 is never
    # written; event C (last segment on frame 12) points at frame 13 and later: dropped
    ev_b, ev_c = [_segment(8, (3.0, 3.0)), _segment(9, (4.0, 4.0))], [_segment(11, (1.0, 1.0)), _segment(12, (2.0, 2.0))]
    writer.write_window(_window(10, 3, nulls=2), None, [ev_b, ev_c])
    numbers, boxes, marks, style = writer.calls[-1]
    assert numbers == (10, 11, 12) and style == [STYLE_EVENT] * 3
    assert marks == [(k, r, r, STYLE_EVENT) for k in range(3) for r in (3, 4)]
    # a window of null frames alone writes nothing
    count = len(writer.calls)
    writer.write_window(_window(0, 0, nulls=3), None, [])
    assert len(writer.calls) == count and writer.frames == 13
    # two events on one frame: marks in the order the tracker found them
    writer._pending = []
    writer.write_window(_window(20, 2), None, [[_segment(18, (1.0, 1.0)), _segment(19, (2.0, 2.0))], [_segment(19, (5.0, 6.0)), _segment(19, (0.0, 0.0))]])
    assert writer.calls[-1][2] == [(0, 1, 1, STYLE_EVENT), (0, 2, 2, STYLE_EVENT), (0, 5, 6, STYLE_EVENT), (0, 0, 0, STYLE_EVENT),
                                   (1, 1, 1, STYLE_EVENT), (1, 2, 2, STYLE_EVENT), (1, 5, 6, STYLE_EVENT), (1, 0, 0, STYLE_EVENT)]


def test_written_file_is_a_y4m_of_the_crop_region(writer, tmp_path):
    from swiftwatcher_amd.io_y4m import open_y4m
    writer.write_window(_window(0, 3, nulls=1), None, [])
    writer.close()
    reader = open_y4m(str(tmp_path / "review.y4m"))
    assert reader.total_frames == 3 and tuple(reader.frame_shape[:2]) == (6, 8)
    reader.close() if hasattr(reader, "close") else None


def test_writer_refuses_a_mask_of_another_size(tmp_path):
    from swiftwatcher_amd.review import ReviewWriter
    with pytest.raises(ValueError):
        ReviewWriter(str(tmp_path / "x.y4m"), [(0, 0), (8, 6)], np.zeros((8, 6), np.uint8), 30)
    assert not os.path.exists(str(tmp_path / "x.y4m"))


def test_struct_layouts_match_the_header(tmp_path):
    """The ctypes mirrors against the C compiler's layout of include/swk.h: sizes and the offsets of the last fields."""
    import ctypes
    import subprocess
    from swiftwatcher_amd import _lib
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "swk.h"\nint main(){printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu", '
                   'sizeof(swk_yuv420_dst), sizeof(swk_review_style), sizeof(swk_review_box), sizeof(swk_review_mark), sizeof(swk_review), '
                   'offsetof(swk_yuv420_dst, c_frame_stride), offsetof(swk_review, mark_arm), offsetof(swk_review, border), '
                   'offsetof(swk_review, nstyles));}')
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "sz")])
    got = [int(v) for v in subprocess.check_output([str(tmp_path / "sz")]).split()]
    assert got == [ctypes.sizeof(_lib.Yuv420Dst), ctypes.sizeof(_lib.ReviewStyle), _lib.REVIEW_BOX_DTYPE.itemsize, _lib.REVIEW_MARK_DTYPE.itemsize,
                   ctypes.sizeof(_lib.Review), _lib.Yuv420Dst.c_frame_stride.offset, _lib.Review.mark_arm.offset, _lib.Review.border.offset,
                   _lib.Review.nstyles.offset]
    assert _lib.REVIEW_STYLE_DTYPE.itemsize == ctypes.sizeof(_lib.ReviewStyle) == 12
