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


def test_every_fused_instantiation_is_planned_by_the_closed_form():
    """The 24 lines `256x4 s4 k<K>m<M> <fmt> fused1` of the golden file (the program's output equals the file: the test above)
    against the ring written out here from the layout comment above acc_fused_slot_dwords, not from the program.  One workgroup
    of four waves, D sample rows in flight per wave, a slot per row:
      fp32    D = 3, slot = 768 dwords per RGB type (the radiance type and K more) + 256 per 1-channel type;
      half    the radiance row stays fp32 (768 dwords) where only the features are half; every half RGB row has its first KiB
              (256 dwords) as a transfer of its own and its last 512 B as a unit, every half 1-channel row is one unit; two
              units share a 256-dword transfer and an odd last one has a transfer to itself.  D = 5 (features half), 6 (all half)."""
    want = {}
    for line in json.load(open(GOLDEN))["cases"]:
        name, _, cols = line.partition(" : ")
        if name.startswith("256x4 s4 k") and name.endswith(" fused1"):
            want[name] = dict(zip("grid fused loader kernel vec dma umul grid_mode resident_blocks K M fmt lds".split(), map(int, cols.split())))
    assert len(want) == 24
    PER_TYPE, PER_TYPE_HALF, FUSED, FUSED_HALF = range(4)          # statmc_device.h: kAccPerType ...
    for K in range(3):
        for M in range(3):
            if K + M == 0:
                continue
            for fmt, fmt_name in enumerate(("f32", "feat16", "all16")):
                if fmt == 0:
                    depth, slot = 3, 768 * (1 + K) + 256 * M
                else:
                    half_rgb = K + (1 if fmt == 2 else 0)
                    u0 = (768 if fmt == 1 else 0) + 256 * half_rgb
                    n_units = half_rgb + M
                    depth, slot = (5 if fmt == 1 else 6), u0 + 256 * ((n_units + 1) // 2)
                got = want.pop("256x4 s4 k%dm%d %s fused1" % (K, M, fmt_name))
                what = (K, M, fmt_name, got)
                assert got["fused"] == 1 and got["kernel"] == (FUSED if fmt == 0 else FUSED_HALF), what
                assert (got["K"], got["M"], got["fmt"]) == (K, M, fmt), what
                assert got["grid"] == 1 and got["resident_blocks"] == 0, what
                assert got["vec"] == 1 and got["loader"] == (0 if fmt == 0 else 1), what
                assert got["lds"] == 4 * depth * slot * 4, what
                assert got["lds"] <= 160 * 1024, what
    assert not want


def test_the_plan_calls_no_hip_function_and_keeps_no_state():
    """plan_accumulate is pure: its text in statmc_pointwise.hip names no HIP call and none of the launch's thread-local records."""
    src = open(os.path.join(ROOT, "statmc_amd", "csrc", "statmc_pointwise.hip")).read()
    start = src.index("AccumulatePlan plan_accumulate(")
    body = src[start:src.index("\n}\n", start)]
    assert "hip" not in body and "g_last_acc" not in body and "static" not in body
