"""The host-only plan of a review call (csrc/review_plan.{h,cpp}: plan_review, review_font, review_label_palette) on the CPU:
tests/review_plan_check.cpp holds it to the header's words -- every refusal's code, message and precedence with the plan left alone and
no source, panel or destination byte read; the destination's geometry and the staging sizes on every listed size; the kernels' table
(records with styles resolved, prefix tables, border words, mask bytes, captions, palette, packed text, block order) on designed
overlays and 3000 seeded random ones; the font against its character set.  The checker is a program of its own, built with the
address and undefined-behaviour sanitizers; nothing is loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_review_plan_invariants(tmp_path):
    exe = str(tmp_path / "review_plan_check")
    csrc = os.path.join(ROOT, "swiftwatcher_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "include"), "-I", csrc, os.path.join(ROOT, "tests", "review_plan_check.cpp"),
                           os.path.join(csrc, "review_plan.cpp"), "-o", exe])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0, run.stdout
