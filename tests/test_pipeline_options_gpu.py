"""The counting loop with its options in combination: every run of the covering array of tests/pipeline_options.py (source x stabilize
x classifier x shape_props x review x windows_per_call x track_by_window x entry point, every pair of levels in some run) against
baselines that are computed once per module.

  baseline          the still twin as a BGR array, every option off but the classifier level, per (classifier level, windows_per_call,
                    entry point): equal segments per frame number, count and events; with a classifier equal removed boxes and
                    bit-equal scores (the baseline's own scores are bit-equal from run to run: asserted here)
  stabilize         every frame's shift is (-jy, -jx), Context.stabilize runs once per window, no StabilizingReader without it
  shape_props       every event segment's attributes equal those of the run with shape_props alone, which are held once to
                    tests/shape_props_ref.py on that clip's own label planes; without it the documented AttributeError
  review            the file equals, byte for byte, that of the run with nothing but this review level and classifier level on the still
                    twin: the same pixels, boxes, removed boxes, event marks and text
  again             one case twice on one context and once more after a refused call
  command line      python -m swiftwatcher_amd with every flag on writes what the library calls gave

The clips' seeds were chosen so that the baselines make events: asserted below with the thresholds of tests/test_track_window_gpu.py."""
import csv
import filecmp
import json
import os

import numpy as np
import pytest

import pipeline_options as po
import shape_props_ref

pytestmark = pytest.mark.gpu


class Lab:
    def __init__(self, workdir, golden_dir):
        self.workdir = str(workdir)
        self.classifiers, self.model_path = po.make_classifiers(golden_dir, workdir)
        self.cache = {}

    def run(self, case, fresh=False, **kw):
        """the case's observation, computed once (fresh=True: again, and not kept)"""
        if fresh:
            return po.run_case(case, self.workdir, self.classifiers, **kw)
        key = (case["name"],) + tuple(sorted(kw.items()))
        if key not in self.cache:
            self.cache[key] = po.run_case(case, self.workdir, self.classifiers, **kw)
        return self.cache[key]

    def baseline(self, case):
        return self.run(po.baseline_case(*po.baseline_key(case)))


@pytest.fixture(scope="module")
def lab(tmp_path_factory, golden_dir):
    return Lab(tmp_path_factory.mktemp("pipeline_options"), golden_dir)


def test_clip_zero_takes_its_regions_from_its_corners():
    crop_region, mask = po.regions(0)          # (asserts that the corners give the crop region the scene was built around)
    (x0, y0), (x1, y1) = crop_region
    assert mask.shape == (y1 - y0, x1 - x0) and 0 < int((mask != 0).sum()) < mask.size


# ---- 1. the baselines ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", ["none", "eval", "dropout"])
def test_baselines(lab, level):
    runs = {(wpc, entry): lab.run(po.baseline_case(level, wpc, entry)) for wpc in (1, 2) for entry in ("single", "videos")}
    first = runs[(1, "single")]
    for key, obs in runs.items():
        assert obs["readers_made"] == 0 and obs["stabilize_calls"] == 0
        for k, video in enumerate(obs["videos"]):
            assert sorted(video["segments"]) == list(range(po.clip(k)["total"] + 1))
            po.check_unbound(video)
            assert video["review"] is None and video["shifts"] is None
            if level != "dropout":          # (a dropout realisation may depend on how the windows are batched: each key stands alone)
                po.check_tracking(video, first["videos"][k], "baseline %s %s clip %d" % (level, key, k))
                if level == "eval":
                    po.check_removed(video, first["videos"][k], "baseline %s %s clip %d" % (level, key, k))
    events = sum(len(v["events"]) for v in first["videos"])
    print("baseline %s: events per clip %s, counts %s, segments seen %s, scores %d" % (
        level, [len(v["events"]) for v in first["videos"]], [v["count"] for v in first["videos"]],
        [sum(len(s) for s in v["segments"].values()) for v in first["videos"]], len(po.score_rows(first["scores"]))))
    # conditions on the baseline (the clips were chosen for them), not measurements of anything new
    if level == "none":
        assert events >= po.MIN_EVENTS_PLAIN
        assert first["scores"] == [] and all(v["removed"] is None for v in first["videos"])
    if level == "eval":
        assert events >= po.MIN_EVENTS_CLASSIFIED
        assert len(first["videos"][0]["events"]) >= 1, "the command-line test needs an event in clip 0"
    if level != "none":
        assert len(po.score_rows(first["scores"])) > 30
        assert sum(len(b) for v in first["videos"] for b in v["removed"].values()) > 0, "the classifier removes something"


@pytest.mark.parametrize("level", ["eval", "dropout"])
@pytest.mark.parametrize("wpc,entry", [(1, "single"), (2, "videos")])
def test_baseline_scores_are_bit_equal_from_run_to_run(lab, level, wpc, entry):
    """what lets test_run ask for bit equality of the scores"""
    case = po.baseline_case(level, wpc, entry)
    po.check_scores(lab.run(case, fresh=True)["scores"], lab.run(case)["scores"], label="the baseline again")


# ---- 4. the shape reference ---------------------------------------------------------------------------------------------------------
def label_planes(k):
    """frame number -> label plane of the still twin of clip k, from the serial window loop with the stage images kept"""
    from swiftwatcher_amd.data_structures import FrameQueue
    from swiftwatcher_amd.io_frames import ArrayReader
    crop_region, _ = po.regions(k)
    reader = ArrayReader(list(po.clip(k)["still"]), fps=30.0)
    queue = FrameQueue(po.N, keep_stages=True)
    out = {}
    while queue.frames_processed < reader.total_frames:
        queue.push_list_of_frames(*reader.get_n_frames(n=po.N))
        queue.preprocess_queue(crop_region, None)
        queue.segment_queue(po.MIN_SEG, crop_region)
        while not queue.is_empty():
            frame = queue.pop_frame()
            if frame.frame_number >= 0:
                out[frame.frame_number] = np.asarray(frame.processed_frames["cc_labeling"])
    return out


def test_shape_reference_run_against_numpy(lab):
    """the attributes of the run with shape_props alone, for every segment of every event and of every fifth frame, against
    image_filtering.ShapeMeasures of the record that tests/shape_props_ref.py makes of the segment's own label plane"""
    from swiftwatcher_amd import image_filtering as img
    obs = lab.run(po.shape_reference_case(), all_shapes=True)
    base = lab.run(po.baseline_case("none", 1, "single"))
    checked = 0
    for k, video in enumerate(obs["videos"]):
        po.check_tracking(video, base["videos"][k], "shape_props alone, clip %d" % k)
        po.check_shapes_in(video, video["shape_table"], "clip %d" % k)
        planes = label_planes(k)
        wanted = {(seg[0], seg[2]) for ev in video["events"] for seg in ev} | {key for key in video["shape_table"] if key[0] % 5 == 0}
        labels = {(n, s[1]): s[0] for n, segs in video["segments"].items() for s in segs}
        for key in sorted(wanted):
            number, bbox = key
            mask = planes[number] == labels[key]
            want_bbox, record = shape_props_ref.measures_input(mask)
            assert tuple(want_bbox) == tuple(bbox), key
            assert video["shape_table"][key] == po.shape_values(img.ShapeMeasures(want_bbox, record)), key
            checked += 1
    assert checked > 30


# ---- the array ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", po.RUNS, ids=[c["name"] for c in po.RUNS])
def test_run(lab, case):
    obs = lab.run(case)
    base = lab.baseline(case)
    assert len(obs["videos"]) == len(base["videos"]) == 2
    classified, stabilized = case["classifier"] != "none", bool(case["stabilize"])
    for k, (video, want) in enumerate(zip(obs["videos"], base["videos"])):
        label = "%s, clip %d" % (case["name"], k)
        po.check_tracking(video, want, label)                                                 # 1
        if classified:                                                                        # 2
            po.check_removed(video, want, label)
        else:
            assert video["removed"] is None
        if stabilized:                                                                        # 3
            po.check_shifts(video, po.clip(k)["jitter"], label)
        else:
            assert video["shifts"] is None
        if case["shape_props"]:                                                               # 4
            po.check_shapes_in(video, lab.run(po.shape_reference_case(), all_shapes=True)["videos"][k]["shape_table"], label)
        else:
            po.check_unbound(video, label)
        if case["review"] != "none":                                                          # 5
            po.check_review(video, lab.run(po.review_reference_case(case))["videos"][k], label)
        else:
            assert video["review"] is None
    if classified:
        # the crops handed to the network are byte-identical and the baseline's scores repeat bit for bit: bit equality.  A reader
        # that segments ahead scores in batches of its own: the same rows in another order
        po.check_scores(obs["scores"], base["scores"], ordered=case["reader"] is None, label=case["name"])
    else:
        assert obs["scores"] == []
    windows = sum(po.windows_of(po.clip(k)["total"]) for k in (0, 1))
    assert (obs["readers_made"], obs["stabilize_calls"]) == ((2, windows) if stabilized else (0, 0))


def test_review_references_differ_where_they_should(lab):
    """what makes the byte comparison of the reviews say something: the review of the still twin differs from the review of the
    shaken clip counted without stabilization, and the classifier's removed boxes and the text change the file"""
    reference = po.review_reference_case(po.case_named("videos_plain_review"))
    plain = lab.run(reference)["videos"]
    raw = lab.run(dict(reference, name="review_plain_shaken_as_it_is", twin="shaken"))["videos"]
    eval_plain = lab.run(po.review_reference_case(po.case_named("eval_plain_review")))["videos"]
    full = lab.run(po.review_reference_case(po.case_named("stab_full_review")))["videos"]
    for k in (0, 1):
        assert plain[k]["review"] != eval_plain[k]["review"] and len(plain[k]["review"]) == len(eval_plain[k]["review"])
        assert plain[k]["review"] != raw[k]["review"] and len(plain[k]["review"]) == len(raw[k]["review"])
        assert len(full[k]["review"]) > len(plain[k]["review"])


# ---- 6. again, and after a refusal ----------------------------------------------------------------------------------------------------
def same_observation(got, want, label):
    for k, (a, b) in enumerate(zip(got["videos"], want["videos"])):
        po.check_tracking(a, b, label)
        po.check_removed(a, b, label)
        po.check_shapes(a, b, label)
        po.check_review(a, b, label)
        assert a["shifts"] == b["shifts"], label
    po.check_scores(got["scores"], want["scores"], label=label)
    assert (got["readers_made"], got["stabilize_calls"]) == (want["readers_made"], want["stabilize_calls"])


def test_twice_on_one_context_and_after_a_refusal(lab):
    from swiftwatcher_amd import pipeline
    case = po.case_named("all_on_producer")
    first = lab.run(case)
    same_observation(lab.run(case, fresh=True), first, "the second run")
    crop_region, mask = po.regions(0)
    with pytest.raises(ValueError, match="stabilize"):
        pipeline.count_swifts(list(po.clip(0)["shaken"]), crop_region, mask, stabilize=17, shape_props=True,
                              classifier=lab.classifiers["eval"], windows_per_call=2)
    same_observation(lab.run(case, fresh=True), first, "the run after the refusal")


# ---- 7. the command line ------------------------------------------------------------------------------------------------------------
def test_command_line_with_every_flag(lab, tmp_path, capsys):
    """python -m swiftwatcher_amd on the 4:2:0 file of the shaken clip 0 (in this process: main(argv)) against count_swifts on the same
    clip from a pipe with the same options"""
    from swiftwatcher_amd import __main__ as cli
    from swiftwatcher_amd import event_classification as ec
    from swiftwatcher_amd import stabilize
    from swiftwatcher_amd.io_data import export_results
    c = po.clip(0)
    twin = dict(po.case_named("all_on_serial"), name="command_line_twin", classifier="eval")
    want = lab.run(twin, clips=(0,))
    video = want["videos"][0]
    po.check_tracking(video, lab.run(po.baseline_case("eval", 1, "single"))["videos"][0], "the library twin")
    assert len(video["events"]) >= 1

    path = po.y4m_path(lab.workdir, 0, "shaken", "420")
    out, review = tmp_path / "tables", tmp_path / "review.y4m"
    corners = "%d,%d,%d,%d" % (c["corners"][0] + c["corners"][1])
    argv = [path, "--corners", corners, "--stabilize", "--shape-props", "--review", str(review), "--review-text", "--review-stages", "rpca,labels",
            "--classify", lab.model_path, "--out", str(out)]
    capsys.readouterr()
    with po.spies() as spy:
        assert cli.main(argv) == 0
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line == {"source": path, "frames": c["total"], "events": len(video["events"]), "count": video["count"],
                    "stabilize": stabilize.summary(video["shifts"], po.SEARCH)}
    assert line["stabilize"]["moved_frames"] > c["total"] // 2 and line["stabilize"]["max_shift"] == int(np.abs(c["jitter"]).max())
    # what the loop saw
    tracker, = spy.trackers
    assert tracker.seen == video["segments"] and tracker.removed == video["removed"]
    po.check_scores(spy.cls.scores, want["scores"], label="command line")
    assert len(spy.made) == 1 and dict(spy.made[0].shifts) == video["shifts"] and len(spy.calls) == po.windows_of(c["total"])
    # what it wrote
    with open(review, "rb") as fh:
        po.check_review(dict(review=fh.read()), video, "command line")
    expected = tmp_path / "expected"
    export_results(str(expected), ec.classify_events(video["raw_events"]), 30.0, 0, c["total"])
    capsys.readouterr()
    cli.write_shape_csv(str(expected / "segments_shape.csv"), video["raw_events"])
    stabilize.write_csv(str(expected / "stabilization.csv"), video["shifts"])
    names = sorted(os.listdir(expected))
    assert sorted(os.listdir(out)) == names and {"segments_shape.csv", "stabilization.csv"} < set(names) and len(names) >= 4
    match, mismatch, errors = filecmp.cmpfiles(str(out), str(expected), names, shallow=False)
    assert (mismatch, errors) == ([], []), "files that differ: %s %s" % (mismatch, errors)
    with open(out / "stabilization.csv", newline="") as fh:
        rows = list(csv.reader(fh))
    assert [[int(x) for x in r[:3]] for r in rows[1:c["total"] + 1]] == [[n, -jy, -jx] for n, (jy, jx) in enumerate(c["jitter"])]
    with open(out / "segments_shape.csv", newline="") as fh:
        rows = list(csv.reader(fh))
    assert len(rows) == 1 + sum(len(ev) for ev in video["events"]) and rows[0] == list(cli.SHAPE_CSV_COLUMNS)
