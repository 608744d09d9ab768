"""The argument checks of the six placement entry points of the classifier's kernels (csrc/cnn_*.hip, cnn_common.h: Place, place_ok):
every clause, violated alone from a call that passes the check, is refused with SWK_ERR_ARG.  The checks come before any HIP call, so
no GPU is needed; the calls are made in a child process that sees no GPU, so that a call which passes the check (the base call of every
entry, or a clause that stopped refusing) fails in the runtime with SWK_ERR_HIP instead of launching a kernel on host memory."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWK_ERR_ARG = -1

# arguments of an entry point in order; p_* are pointers (16-byte aligned host buffers; "+4" misaligns, None is a null pointer)
PLACE = ["dH", "dW", "dC", "off_y", "off_x", "c_off"]
CONV3 = ["p_stream", "p_src", "n", "t", "cin", "p_weight", "p_bias", "cout", "p_dst"] + PLACE
ENTRIES = {
    "swk_nhwc_conv1x1_bias_relu_place": (
        ["p_stream", "p_src", "n", "sh", "sw", "cin", "crop_y", "crop_x", "h", "w", "p_weight", "p_bias", "cout", "p_dst"] + PLACE,
        dict(n=2, sh=8, sw=9, cin=32, crop_y=1, crop_x=2, h=6, w=5, cout=64, dH=8, dW=7, dC=128, off_y=2, off_x=1, c_off=64)),
    "swk_nhwc_conv3x3_bias_relu_place": (CONV3, dict(n=2, t=8, cin=32, cout=128, dH=8, dW=7, dC=256, off_y=2, off_x=1, c_off=128)),
    "swk_nhwc_conv3x3_winograd_bias_relu_place": (CONV3, dict(n=2, t=8, cin=32, cout=128, dH=8, dW=7, dC=256, off_y=2, off_x=1, c_off=128)),
    "swk_nhwc_conv3x3_winograd_bf16s_bias_relu_place": (CONV3, dict(n=2, t=8, cin=32, cout=128, dH=8, dW=7, dC=256, off_y=2, off_x=1, c_off=128)),
    "swk_nhwc_maxpool3s2_conv1x1_bias_relu_place": (
        ["p_stream", "p_src", "n", "t", "cin", "p_weight", "p_bias", "cout", "p_dst", "dH", "dW", "dC", "off_y", "off_x", "p_ring", "live_lo", "live_n"],
        dict(n=2, t=17, cin=64, cout=32, dH=10, dW=9, dC=32, off_y=2, off_x=1, live_lo=2, live_n=13)),          # P = 8
    "swk_nhwc_bias_relu_place": (
        ["p_stream", "p_src", "n", "sh", "sw", "c", "crop_y", "crop_x", "h", "w", "p_bias", "p_dst"] + PLACE,
        dict(n=2, sh=8, sw=9, c=64, crop_y=1, crop_x=2, h=6, w=5, dH=8, dW=7, dC=128, off_y=2, off_x=1, c_off=64)),
}
NULLS = {"p_src": None, "p_weight": None, "p_bias": None, "p_dst": None}
SQUARE = {"n < 1": dict(n=0), "t < 3": dict(t=2), "off_y < 0": dict(off_y=-1), "off_x < 0": dict(off_x=-1), "c_off < 0": dict(c_off=-4),
          "rows past dH": dict(off_y=3), "columns past dW": dict(off_x=2), "c_off + cout > dC": dict(c_off=132, dC=256)}
QUADS = {"cout & 3": dict(cout=126), "cout < 4": dict(cout=0), "dC & 3": dict(dC=258), "c_off & 3": dict(c_off=126)}
CROP = {"h < 1": dict(h=0), "w < 1": dict(w=0), "crop_y < 0": dict(crop_y=-1), "crop_x < 0": dict(crop_x=-1), "crop past sh": dict(crop_y=3),
        "crop past sw": dict(crop_x=5), "rows past dH": dict(off_y=3), "columns past dW": dict(off_x=3), "n < 1": dict(n=0),
        "off_y < 0": dict(off_y=-1), "off_x < 0": dict(off_x=-1), "c_off < 0": dict(c_off=-4), "dC & 3": dict(dC=130), "c_off & 3": dict(c_off=62)}
WINO = dict(SQUARE, **QUADS, **{"src misaligned": dict(p_src="+4"), "dst misaligned": dict(p_dst="+4"), "weight misaligned": dict(p_weight="+4"),
                                "unsupported (cin, cout)": dict(cin=32, cout=64), "unsupported cin": dict(cin=24, cout=96)})
VIOLATIONS = {
    "swk_nhwc_conv1x1_bias_relu_place": dict(CROP, **{
        "cin < 16": dict(cin=0), "cin & 15": dict(cin=24), "cin > 1024": dict(cin=1040), "cout < 4": dict(cout=0), "cout > 256": dict(cout=260, dC=512),
        "cout & 3": dict(cout=62), "c_off + cout > dC": dict(c_off=68), "src misaligned": dict(p_src="+4"), "dst misaligned": dict(p_dst="+4"),
        "weight misaligned": dict(p_weight="+4"), "unsupported column blocks": dict(cout=160, dC=256)}),
    # the direct kernel stores scalars: it does not ask for multiples of four or an aligned dst (not exercised here: such a call is accepted)
    "swk_nhwc_conv3x3_bias_relu_place": dict(SQUARE, **{
        "cin < 16": dict(cin=0), "cin & 15": dict(cin=24), "cin > 1024": dict(cin=1040), "cout < 1": dict(cout=0), "cout > 256": dict(cout=260, dC=512),
        "src misaligned": dict(p_src="+4"), "unsupported column blocks": dict(cout=160, c_off=0)}),
    "swk_nhwc_conv3x3_winograd_bias_relu_place": WINO,
    "swk_nhwc_conv3x3_winograd_bf16s_bias_relu_place": WINO,
    "swk_nhwc_maxpool3s2_conv1x1_bias_relu_place": {
        "n < 1": dict(n=0), "t < 3": dict(t=2), "cin < 32": dict(cin=0), "cin & 31": dict(cin=48), "cout < 4": dict(cout=0), "cout & 3": dict(cout=30),
        "cout > 64": dict(cout=68, dC=128), "dC & 3": dict(dC=34), "off_y < 0": dict(off_y=-1), "off_x < 0": dict(off_x=-1),
        "src misaligned": dict(p_src="+4"), "dst misaligned": dict(p_dst="+4"), "weight misaligned": dict(p_weight="+4"),
        "bias misaligned": dict(p_bias="+4"), "ring misaligned": dict(p_ring="+4"), "live_lo < 0": dict(live_lo=-1), "live_n < 0": dict(live_n=-1),
        "live square past the tile": dict(live_lo=5), "rows past dH": dict(off_y=3), "columns past dW": dict(off_x=2), "cout > dC": dict(dC=28),
        "P * P > 96": dict(t=21, dH=12, dW=11)},
    "swk_nhwc_bias_relu_place": dict(CROP, **{
        "c < 4": dict(c=0), "c & 3": dict(c=62), "c_off + c > dC": dict(c_off=68), "src misaligned": dict(p_src="+4"),
        "bias misaligned": dict(p_bias="+4"), "dst misaligned": dict(p_dst="+4")}),
}
for _name, (_args, _base) in ENTRIES.items():
    for _p in NULLS:
        if _p in _args:
            VIOLATIONS[_name]["null " + _p[2:]] = {_p: None}

CHILD = r"""
import ctypes, json, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from swiftwatcher_amd import _lib
lib = _lib.load()
spec = json.load(sys.stdin)
raw = np.zeros(1 << 20, np.uint8)
aligned = raw.ctypes.data + (-raw.ctypes.data) % 16          # never read here: every call is refused, or fails for want of a GPU
out = {}
for name, (args, base) in spec["entries"].items():
    def call(change):
        v = dict(base, **change)
        a = []
        for k in args:
            if k == "p_stream": a.append(None)
            elif k.startswith("p_"):
                p = v.get(k, "")
                a.append(None if p is None else ctypes.c_void_p(aligned + (4 if p == "+4" else 0)))
            else: a.append(v[k])
        return getattr(lib, name)(*a)
    out[name] = {"base": call({}), "refused": {what: call(change) for what, change in spec["violations"][name].items()}}
print("RESULT " + json.dumps(out))
"""


def test_every_clause_of_the_placement_checks_refuses():
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT], input=json.dumps({"entries": ENTRIES, "violations": VIOLATIONS}), env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(next(l for l in r.stdout.splitlines() if l.startswith("RESULT "))[7:])
    assert set(got) == set(ENTRIES) and len(got) == 6
    for name, res in got.items():
        # the base call passes the check (and then fails in the runtime: there is no GPU to launch on)
        assert res["base"] not in (0, SWK_ERR_ARG), (name, res["base"])
        wrong = {what: rc for what, rc in res["refused"].items() if rc != SWK_ERR_ARG}
        assert not wrong, (name, wrong)
        assert len(res["refused"]) >= 15, name
