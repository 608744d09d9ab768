"""The launch sequence of the cropped classifier's forward, route by route: every swk_nhwc_* call of an eager forward (entry point,
stream, shapes, offsets, and which tensor every address points into) against tests/golden/cnn_launch_trace.json, which was recorded
with this file before the forward was split into one function per route.  A refactor of the host code must leave it as it is; a
change that adds, drops or re-aims a launch shows here as the first differing call.  The operand tensors the classifier makes for its
kernels (conv1's weights, the 3x3 expands' in each kernel's layout, the head's ring) are recorded as "ptr" only: that the right one
reaches each kernel is what tests/test_cnn_accuracy.py and tests/test_wino_bf16s.py check, route by route, on the values.

    python tests/test_cnn_launch_trace.py [output.json]      # records the golden file (on the GPU)
"""
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "cnn_launch_trace.json")

SWITCHES = {"default": {}, "wino_f32": {"wino_split_bf16": False}, "direct3x3": {"winograd": False},
            "unfused_pool": {"fuse_pool": False}, "miopen": {"own_kernels": False}}
ROWS = ((3, 0), (5, 64))                    # (rows, row0)
CASES = ["%s-%d@%d" % (route, k, row0) for route in SWITCHES for k, row0 in ROWS] + ["dropout-3@0", "two_chains-1100"]


class RecordingLib:
    """The library with every swk_nhwc_* call noted down (tools/bench_convs.py substitutes _lib.load the same way)."""

    def __init__(self, lib):
        self._lib = lib
        self.calls = []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("swk_nhwc_"):
            return fn

        def call(*a):
            self.calls.append((name, a))
            return fn(*a)
        return call


def _registry(clf, x):
    """(name, first byte, bytes) of the input, the model's parameters and the cropped network's persistent buffers."""
    named = [("x", x)] + [("model." + n, p) for n, p in clf.model.named_parameters()]
    bufs, live = clf.cropped._buf
    named += [("bufs[%d]" % j, t) for j, t in enumerate(bufs)]
    named += [("live[%d]" % j, t) for j, t in enumerate(live) if t is not None]
    aux = clf.cropped._aux
    named += [("aux.conv1", aux["conv1"]), ("aux.pool_in", aux["pool_in"])]
    named += [("aux.pool_out[%d]" % i, t) for i, t in enumerate(aux["pool_out"])]
    return [(name, t.data_ptr(), t.numel() * t.element_size()) for name, t in named]


def _normalise(calls, registry, streams):
    out = []
    for name, args in calls:
        row = [name, streams[getattr(args[0], "value", args[0]) or 0]]
        for a in args[1:]:
            a = getattr(a, "value", a)                       # ctypes scalars (the dropout seed)
            if isinstance(a, int) and a >= 1 << 32:
                hit = [(n, a - base) for n, base, size in registry if base <= a < base + size]
                a = "%s+%d" % hit[0] if hit else "ptr"
            assert a is None or isinstance(a, (int, float, str)), (name, a)
            row.append(a)
        out.append(row)
    return out


def _input(rows, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn((rows, 3, 40, 40), generator=g).cuda().contiguous(memory_format=torch.channels_last)


def record():
    """{case: [[entry point, stream, argument, ...], ...]} for every case of CASES."""
    from oracle import classifier_ref as ref
    from swiftwatcher_amd import _lib
    from swiftwatcher_amd.segment_classification import SegmentClassifier
    clf = SegmentClassifier.from_state_dict(ref.random_state_dict(17), batch_size=2048)
    net = clf.cropped
    assert clf._split_rows == 1024 and net.own_kernels and net.winograd and net.wino_split_bf16 and net.fuse_pool
    lib = RecordingLib(_lib.load())
    load, _lib.load = _lib.load, lambda: lib
    traces = {}

    def trace(case, x, forward):
        lib.calls = []
        forward()
        torch.cuda.synchronize()
        streams = {torch.cuda.current_stream(clf.device).cuda_stream: "main"}
        if clf._side_stream is not None:
            streams[clf._side_stream.cuda_stream] = "side"
        traces[case] = _normalise(lib.calls, _registry(clf, x), streams)

    try:
        for route, switches in SWITCHES.items():
            for name, value in switches.items():
                setattr(net, name, value)
            for k, row0 in ROWS:
                x = _input(k, 100 + k)
                trace("%s-%d@%d" % (route, k, row0), x, lambda: net(x, row0=row0))
            for name, value in switches.items():
                setattr(net, name, not value)
        x = _input(3, 103)
        keys = torch.arange(1, 4, dtype=torch.int64, device=clf.device)
        trace("dropout-3@0", x, lambda: net(x, dropout=(keys, 7, 2)))
        x = _input(1100, 1100)
        trace("two_chains-1100", x, lambda: clf._forward(x))
    finally:
        _lib.load = load
    assert sorted(traces) == sorted(CASES)
    return traces


@pytest.fixture(scope="module")
def traces():
    return json.loads(json.dumps(record()))


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_launch_sequence_matches_recording(case, traces):
    with open(GOLDEN) as f:
        want = json.load(f)[case]
    got = traces[case]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, "%s: call %d differs\n  got  %r\n  want %r" % (case, i, g, w)
    assert len(got) == len(want), "%s: %d calls, the recording has %d" % (case, len(got), len(want))


@pytest.mark.gpu
def test_two_chain_trace_is_two_forwards_on_disjoint_rows(traces):
    """What the recording of the 1,100-row forward must look like whatever else changes: 76 rows on the side stream, then 1,024 on
    the main one, the same entry points in the same order."""
    calls = traces["two_chains-1100"]
    side = [c for c in calls if c[1] == "side"]
    main = [c for c in calls if c[1] == "main"]
    assert calls == side + main and [c[0] for c in side] == [c[0] for c in main] and len(side) > 20
    assert {c[3] for c in side} == {76} and {c[3] for c in main} == {1024}


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    path = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    got = record()
    with open(path, "w") as f:                                # one call per line
        f.write("{\n" + ",\n".join("%s: [\n%s\n]" % (json.dumps(c), ",\n".join(json.dumps(call) for call in got[c])) for c in CASES) + "\n}\n")
    print("wrote %s" % path)
