"""The film-major accumulation's launch rules without a GPU: tests/cpp/test_accumulate_plan.cpp runs statmc::plan_accumulate over
a fixed list of launches, and every line must be the one in tests/golden/accumulate_plan.json.  The grid, fused and loader
columns there were recorded from launch_accumulate as it was before plan_accumulate existed, so the rules have not moved."""
import json
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "accumulate_plan.json")


def test_every_planned_launch_is_the_recorded_one():
    from statmc_amd import build
    build.build_tools()
    out = subprocess.run([build.ACC_PLAN_BIN], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    got = out.stdout.splitlines()
    want = json.load(open(GOLDEN))["cases"]
    assert len(want) >= 300 and os.path.getsize(GOLDEN) < 64 * 1024
    names = [line.split(" : ")[0] for line in got]
    assert len(set(names)) == len(names)
    assert names == [line.split(" : ")[0] for line in want], "the case list and the golden file's differ"
    wrong = [(g, w) for g, w in zip(got, want) if g != w]
    assert not wrong, "%d of %d cases, the first (planned, recorded): %s" % (len(wrong), len(want), wrong[0])


def test_the_plan_calls_no_hip_function_and_keeps_no_state():
    """plan_accumulate is pure: its text in statmc_pointwise.hip names no HIP call and none of the launch's thread-local records."""
    src = open(os.path.join(ROOT, "statmc_amd", "csrc", "statmc_pointwise.hip")).read()
    start = src.index("AccumulatePlan plan_accumulate(")
    body = src[start:src.index("\n}\n", start)]
    assert "hip" not in body and "g_last_acc" not in body and "static" not in body
