"""tests/pipeline_options.py without a GPU: the covering array holds every pair of option levels, the clips are what the GPU tests take
them for, and every comparison helper fails on an observation that was doctored in the one way it is there to catch."""
import copy

import numpy as np
import pytest

import pipeline_options as po
import stabilize_ref as ref


# ---- the covering array -----------------------------------------------------------------------------------------------------------
def test_every_pair_of_levels_occurs_in_some_run():
    assert len(po.RUNS) <= 16 and len({c["name"] for c in po.RUNS}) == len(po.RUNS)
    assert len(po.all_pairs()) == sum(len(a) * len(b) for i, (_, a) in enumerate(po.AXES) for _, b in po.AXES[i + 1:]) == 157
    assert po.uncovered_pairs(po.RUNS) == []


def test_the_pair_check_notices_a_missing_pair():
    """a single run holds 28 pairs; the pairs that go with a run that is left out are pairs of that run's levels, and for some run
    there are such pairs; a level that is none of its axis is refused"""
    assert len(po.all_pairs()) - len(po.uncovered_pairs(po.RUNS[:1])) == 28
    for drop in range(len(po.RUNS)):
        rest = po.RUNS[:drop] + po.RUNS[drop + 1:]
        gone = po.uncovered_pairs(rest)
        assert all(all(po.RUNS[drop][axis] == level for axis, level in pair) for pair in gone)
    assert any(po.uncovered_pairs(po.RUNS[:k] + po.RUNS[k + 1:]) for k in range(len(po.RUNS)))
    with pytest.raises(ValueError):
        po.uncovered_pairs([dict(po.RUNS[0], source="mp4")])


def test_the_listed_combinations_are_in_the_array():
    on = dict(stabilize=po.SEARCH, shape_props=True, review="full", track_by_window=True)
    for name, wpc, entry in (("all_on_serial", 1, "single"), ("all_on_producer", 2, "single"), ("all_on_videos", 2, "videos")):
        case = po.case_named(name)
        assert all(case[k] == v for k, v in on.items()) and case["classifier"] != "none" and case["source"] != "array"
        assert (case["windows_per_call"], case["entry"]) == (wpc, entry)
    pre = po.case_named("presegmenting")
    assert pre["reader"] == "presegmenting" and pre["shape_props"] and pre["classifier"] != "none" and pre["stabilize"]
    assert all(c["reader"] is None for c in po.RUNS if c is not pre)
    # the baselines and reference runs are what the issue says they are
    base = po.baseline_case("eval", 2, "videos")
    assert (base["source"], base["stabilize"], base["shape_props"], base["review"]) == ("array", 0, False, "none")
    rv = po.review_reference_case(po.case_named("all_on_videos"))
    assert (rv["source"], rv["stabilize"], rv["shape_props"], rv["review"], rv["classifier"]) == ("array", 0, False, "full", "eval")
    sh = po.shape_reference_case()
    assert (sh["source"], sh["stabilize"], sh["classifier"], sh["shape_props"], sh["review"]) == ("array", 0, "none", True, "none")


# ---- the clips --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [0, 1])
def test_clip_properties(k):
    c = po.clip(k)
    H, W = c["frame_hw"]
    (x0, y0), (x1, y1) = c["crop_region"]
    total = c["total"]
    assert 47 <= total <= 58 and po.windows_of(total) == 3 and total % po.N                    # three windows, the last one padded
    assert x1 - x0 <= 96 and y1 - y0 <= 64
    assert c["shaken"].shape == c["still"].shape == (total, H, W, 3) and c["y_shaken"].shape == (total, H, W)
    jitter = c["jitter"]
    assert tuple(jitter[0]) == (0, 0) and 4 <= np.abs(jitter).max() <= ref.JITTER and jitter.min() < 0 < jitter.max()
    assert np.array_equal(c["shaken"][0], c["still"][0])
    inside = (slice(None), slice(y0, y1), slice(x0, x1))
    differs = [not np.array_equal(a, b) for a, b in zip(c["shaken"][inside], c["still"][inside])]
    assert sum(differs) > total // 2
    # a pipe's reader holds the crop region plus its margin plus the search range: inside the picture on every side
    my, mx = po.MIN_SEG[1] // 2 + po.SEARCH, po.MIN_SEG[0] // 2 + po.SEARCH
    assert y0 - my >= 0 and x0 - mx >= 0 and y1 + my <= H and x1 + mx <= W
    from swiftwatcher_amd.stabilize import search_rect
    (ya, yb, xa, xb), grown = search_rect((H, W, 3), c["crop_region"], po.SEARCH, po.MIN_SEG)
    assert grown == (ya - po.SEARCH, yb + po.SEARCH, xa - po.SEARCH, xb + po.SEARCH)          # nothing was clipped


def test_the_geometries_differ_and_one_is_odd():
    a, b = po.clip(0), po.clip(1)
    assert a["frame_hw"] != b["frame_hw"] and a["total"] != b["total"]
    size = lambda c: (c["crop_region"][1][0] - c["crop_region"][0][0], c["crop_region"][1][1] - c["crop_region"][0][1])          # noqa: E731
    assert size(a) != size(b)
    (x0, y0), _ = b["crop_region"]
    assert size(b)[0] % 2 == 1 and x0 % 2 == 1 and y0 % 2 == 1 and b["frame_hw"][1] % 2 == 1


@pytest.mark.parametrize("k", [0, 1])
def test_every_source_holds_the_same_pictures(k):
    """the host statements of the conversions: the 4:2:0 and the 4:4:4 file of a clip decode to its BGR array, shaken and still"""
    from swiftwatcher_amd.io_y4m import yuv420_rect_to_bgr, yuv_rect_to_bgr
    c = po.clip(k)
    H, W = c["frame_hw"]
    (u420, v420), (u444, v444) = po.flat_chroma((H, W), "420"), po.flat_chroma((H, W), "444")
    for twin in ("shaken", "still"):
        for f in (0, 1, c["total"] - 1):
            y = c["y_" + twin][f]
            assert np.array_equal(yuv420_rect_to_bgr(y, u420, v420, 0, H, 0, W), c[twin][f])
            assert np.array_equal(yuv_rect_to_bgr(y, u444, v444, 0, H, 0, W, sx=0, sy=0), c[twin][f])
    assert np.array_equal(po.luma(c["still"][:1])[0] >= 16, np.ones((H, W), bool))


def test_clip_one_has_given_regions():
    crop_region, mask = po.regions(1)
    assert crop_region == po.clip(1)["crop_region"] and mask.shape == (56, 83) and mask[:22].max() == 0 and mask[22:].min() == 255


# ---- the comparison helpers reject doctored observations ---------------------------------------------------------------------------
def observation():
    """what run_case returns for one video, made by hand: three frames, two events, a classifier, shapes, a review, shifts"""
    seg = lambda label, r, c: (label, (r, c, r + 4, c + 6), (r + 1.5, c + 2.5), 19)          # noqa: E731
    segments = {0: [seg(1, 3, 4)], 1: [seg(1, 4, 6), seg(2, 20, 30)], 2: []}
    events = [[(0,) + seg(1, 3, 4), (1,) + seg(1, 4, 6)], [(1,) + seg(2, 20, 30)]]
    shape = lambda x: (("orientation", np.float64(x).tobytes()), ("moments", np.arange(16, dtype=np.float64).tobytes()))          # noqa: E731
    return dict(segments=segments, count=2, events=events, shapes=[[shape(0.25), shape(0.5)], [shape(-1.0)]],
                removed={0: [], 1: [(7, 8, 12, 14)], 2: [(1, 1, 5, 5), (9, 9, 12, 12)]},
                review=b"YUV4MPEG2 W96 H64\n" + b"FRAME\n" + bytes(range(200)) + b"FRAME\n" + bytes(200), shifts={0: (0, 0, 11, 11), 1: (-2, 3, 9, 400), 2: (5, -5, 8, 900), 3: (5, -5, 8, 900)})


JITTER = np.array([(0, 0), (2, -3), (-5, 5)])


def all_checks(got, want):
    po.check_tracking(got, want)
    po.check_removed(got, want)
    po.check_shapes(got, want)
    po.check_review(got, want)
    po.check_shifts(got, JITTER)


def test_the_helpers_accept_an_equal_observation():
    all_checks(copy.deepcopy(observation()), observation())
    rows = [np.array([[0.5, -1.25], [3.0, 2.0]], np.float32), np.array([[7.0, 8.0]], np.float32)]
    po.check_scores(rows, [np.concatenate(rows)])
    po.check_scores(rows[::-1], rows, ordered=False)
    po.check_unbound(dict(shapes=[[None, None], [None]]))


def dropped_event(o):
    del o["events"][1]


def moved_bbox(o):
    label, (r0, c0, r1, c1), centroid, area = o["segments"][1][1]
    o["segments"][1][1] = (label, (r0, c0 + 1, r1, c1 + 1), centroid, area)


def moved_event_bbox(o):
    n, label, (r0, c0, r1, c1), centroid, area = o["events"][0][1]
    o["events"][0][1] = (n, label, (r0 + 1, c0, r1 + 1, c1), centroid, area)


def other_count(o):
    o["count"] += 1


def missing_frame(o):
    del o["segments"][2]


DOCTORED_TRACKING = [dropped_event, moved_bbox, moved_event_bbox, other_count, missing_frame]


@pytest.mark.parametrize("doctor", DOCTORED_TRACKING, ids=lambda f: f.__name__)
def test_check_tracking_rejects(doctor):
    got = observation()
    doctor(got)
    with pytest.raises(AssertionError):
        po.check_tracking(got, observation())
    with pytest.raises(AssertionError):
        po.check_tracking(observation(), got)


def test_check_review_rejects_one_flipped_byte():
    got = observation()
    raw = bytearray(got["review"])
    raw[100] ^= 1
    got["review"] = bytes(raw)
    with pytest.raises(AssertionError, match="1 bytes of the review file differ, first at offset 100"):
        po.check_review(got, observation())
    got["review"] = observation()["review"][:-1]
    with pytest.raises(AssertionError):
        po.check_review(got, observation())
    got["review"] = None
    with pytest.raises(AssertionError):
        po.check_review(got, observation())


def test_check_shapes_rejects_one_changed_attribute():
    got = observation()
    name, raw = got["shapes"][0][1][0]
    got["shapes"][0][1] = ((name, np.nextafter(np.float64(0.5), 1.0).tobytes()),) + got["shapes"][0][1][1:]
    with pytest.raises(AssertionError, match="event 0 segment 1: orientation"):
        po.check_shapes(got, observation())
    got = observation()
    got["shapes"][1][0] = None
    with pytest.raises(AssertionError):
        po.check_shapes(got, observation())
    with pytest.raises(AssertionError):
        po.check_unbound(observation())


def test_check_shifts_rejects_one_frame_off_by_one():
    for frame, change in ((1, (0, 1)), (2, (-1, 0)), (3, (0, -1))):
        got = observation()
        dy, dx, sad, sad0 = got["shifts"][frame]
        got["shifts"][frame] = (dy + change[0], dx + change[1], sad, sad0)
        with pytest.raises(AssertionError, match="frame %d" % frame):
            po.check_shifts(got, JITTER)
    got = observation()
    del got["shifts"][1]
    with pytest.raises(AssertionError):
        po.check_shifts(got, JITTER)
    with pytest.raises(AssertionError):
        po.check_shifts(dict(shifts=None), JITTER)


def test_check_removed_rejects_one_missing_box():
    got = observation()
    del got["removed"][2][1]
    with pytest.raises(AssertionError, match="frame 2"):
        po.check_removed(got, observation())
    got = observation()
    got["removed"] = None
    with pytest.raises(AssertionError):
        po.check_removed(got, observation())


def test_check_scores_rejects_one_bit():
    want = [np.array([[0.5, -1.25], [3.0, 2.0], [0.0, 1.0]], np.float32)]
    got = [want[0].copy()]
    got[0][1, 1] = np.nextafter(np.float32(2.0), np.float32(3.0))
    with pytest.raises(AssertionError, match="1 of 3 score rows differ, first at 1"):
        po.check_scores(got, want)
    with pytest.raises(AssertionError):
        po.check_scores(got, want, ordered=False)
    with pytest.raises(AssertionError):
        po.check_scores([want[0][:2]], want)
    got = [want[0].copy()]
    got[0][2, 0] = -0.0                                    # equal as numbers, another bit pattern
    with pytest.raises(AssertionError):
        po.check_scores(got, want)


def shape_table(o):
    return {(seg[0], seg[2]): values for row, event in zip(o["shapes"], o["events"]) for values, seg in zip(row, event)}


def test_check_shapes_in_rejects_a_changed_attribute_and_an_unknown_box():
    table = shape_table(observation())
    po.check_shapes_in(observation(), table)
    got = observation()
    got["shapes"][1][0] = (got["shapes"][1][0][0], ("moments", (np.arange(16, dtype=np.float64) + np.eye(1, 16, 5)[0]).tobytes()))
    with pytest.raises(AssertionError, match="event 1 segment 0: moments"):
        po.check_shapes_in(got, table)
    got = observation()
    moved_event_bbox(got)
    with pytest.raises(AssertionError, match="no segment of frame 1 has the box"):
        po.check_shapes_in(got, table)
    got = observation()
    got["shapes"][0][0] = None
    with pytest.raises(AssertionError, match="no shape record"):
        po.check_shapes_in(got, table)
