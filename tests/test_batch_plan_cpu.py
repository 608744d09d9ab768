"""The host-only plan of a batch call (csrc/batch_plan.{h,cpp}: plan_batch, fill_batch_tables) on the CPU: tests/batch_plan_check.cpp
holds it to its invariants -- sub-batch membership and offsets, disjoint plane spans, window order, the labeller's word width, staging
offsets, record flags, the descriptor tables, every refusal's code and message -- on designed group mixes and 3000 seeded random ones.
The checker is a program of its own, built with the address and undefined-behaviour sanitizers; nothing is loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_batch_plan_invariants(tmp_path):
    exe = str(tmp_path / "batch_plan_check")
    csrc = os.path.join(ROOT, "swiftwatcher_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "include"), "-I", csrc, os.path.join(ROOT, "tests", "batch_plan_check.cpp"),
                           os.path.join(csrc, "batch_plan.cpp"), "-o", exe])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0, run.stdout
