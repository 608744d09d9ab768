"""python -m swiftwatcher_amd --shape-props: the flag is planned like the others, and with --out DIR a count over a tiny .y4m writes
DIR/segments_shape.csv -- one row per segment of every event, values equal to the segments' attributes."""
import csv
import json
import os

import numpy as np
import pytest

CROP = [(30, 20), (30 + 96, 20 + 64)]
CORNERS = ((40, 71), (116, 71))          # the top edge of the clip's chimney (tests/test_y4m_stream_gpu.py)


def test_plan_accepts_the_flag():
    from swiftwatcher_amd.__main__ import plan
    args, jobs = plan(["clip.y4m", "--corners", "40,71,116,71", "--shape-props", "--out", "tables"])
    assert args.shape_props is True and args.out == "tables" and jobs == [("clip.y4m", CORNERS)]
    args, _ = plan(["clip.y4m", "--corners", "40,71,116,71"])
    assert args.shape_props is False
    args, _ = plan(["-", "--corners", "40,71,116,71", "--shape-props", "--windows-per-call", "4"])
    assert args.shape_props is True and args.windows_per_call == 4


def test_shape_rows_read_the_segments_attributes():
    """(no GPU: hand-made segments)"""
    import shape_props_ref as ref
    from swiftwatcher_amd import image_filtering as img
    from swiftwatcher_amd.__main__ import SHAPE_CSV_COLUMNS, shape_rows
    from swiftwatcher_amd.data_structures import Segment
    mask = np.zeros((9, 14), bool)
    mask[2:7, 3:12] = True
    mask[4, 6] = False
    bbox, rec = ref.measures_input(mask, (10, 20))
    seg = Segment(img.RegionProps(4, bbox, (14.0, 27.5), int(mask.sum())), 17, "00:00:00.567", None)
    seg._shape = rec
    rows = shape_rows([[seg], [seg, seg]])
    assert [r[0] for r in rows] == [0, 1, 1] and len(rows[0]) == len(SHAPE_CSV_COLUMNS)
    m = img.ShapeMeasures(bbox, rec)
    assert rows[0] == (0, 17, 4, int(mask.sum()), 14.0, 27.5, m.orientation, m.eccentricity, m.major_axis_length, m.minor_axis_length,
                       m.perimeter, m.extent, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("wpc", [1, 3])
def test_segments_shape_csv(tmp_path, capsys, wpc):
    import yuv_ref
    from swiftwatcher_amd import pipeline, synthetic
    from swiftwatcher_amd.__main__ import SHAPE_CSV_COLUMNS, main
    from swiftwatcher_amd.io_y4m import Y4MWriter
    bgr = synthetic.full_frames(500, 52, CROP, frame_hw=(110, 160), birds=4, bird_len=(8, 12), bird_wid=(3, 5))[::-1].copy()
    y, u, v = yuv_ref.bgr_to_yuv420(bgr)
    path = str(tmp_path / "tiny.y4m")
    with Y4MWriter(path, 160, 110, 30) as w:
        for k in range(44):
            w.append(y[k], u[k], v[k])
    out = str(tmp_path / "tables")
    assert main([path, "--corners", "40,71,116,71", "--out", out, "--shape-props", "--windows-per-call", str(wpc)]) == 0
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    count, events = pipeline.count_swifts(path, corners=CORNERS, windows_per_call=wpc, shape_props=True)
    assert line["events"] == len(events) > 0 and line["count"] == count
    with open(os.path.join(out, "segments_shape.csv"), newline="") as fh:
        rows = list(csv.reader(fh))
    assert tuple(rows[0]) == SHAPE_CSV_COLUMNS
    segments = [(k, s) for k, ev in enumerate(events) for s in ev]
    assert len(rows) - 1 == len(segments)
    for row, (k, s) in zip(rows[1:], segments):
        assert [int(row[0]), int(row[1]), int(row[2]), int(row[3])] == [k, s.parent_frame_number, s.label, s.area]
        assert [float(x) for x in row[4:12]] == [s.centroid[0], s.centroid[1], s.orientation, s.eccentricity, s.major_axis_length,
                                                 s.minor_axis_length, s.perimeter, s.extent]
        assert int(row[12]) == s.euler_number
    # without the flag the folder holds the result tables alone
    plain = str(tmp_path / "plain")
    assert main([path, "--corners", "40,71,116,71", "--out", plain, "--windows-per-call", str(wpc)]) == 0
    assert "segments_shape.csv" not in os.listdir(plain) and sorted(os.listdir(plain)) == sorted(set(os.listdir(out)) - {"segments_shape.csv"})
