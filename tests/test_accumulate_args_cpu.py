"""What the accumulation entries check and fill, without a GPU and without the library: tests/cpp/test_accumulate_args.cpp runs
every check and fill of statmc_amd/csrc/statmc_accumulate_args.h over a fixed case list, and every line must be the one in
tests/golden/accumulate_args.json; once more under AddressSanitizer and UBSan.  The film there is 12 x 5, so row 3 starts at
pixel 36: 144 bytes into an int32 or 1-channel fp32 plane, 432 into an RGB fp32 plane, 216 into an RGB half arena."""
import json
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "accumulate_args.json")
SRC = os.path.join(ROOT, "tests", "cpp", "test_accumulate_args.cpp")
HEADER = os.path.join(ROOT, "statmc_amd", "csrc", "statmc_accumulate_args.h")


def _run(binary):
    out = subprocess.run([binary], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stderr == "", out.stdout + out.stderr
    return out.stdout.splitlines()


@pytest.fixture(scope="module")
def lines():
    from statmc_amd import build
    build.build_tools()
    return _run(build.ACC_ARGS_BIN)


def test_every_case_is_the_recorded_line(lines):
    want = json.load(open(GOLDEN))["cases"]
    assert len(want) >= 130 and os.path.getsize(GOLDEN) < 64 * 1024
    names = [line.split(" : ")[0] for line in lines]
    assert len(set(names)) == len(names)
    assert names == [line.split(" : ")[0] for line in want], "the case list and the golden file's differ"
    wrong = [(g, w) for g, w in zip(lines, want) if g != w]
    assert not wrong, "%d of %d cases, the first (got, recorded): %s" % (len(wrong), len(want), wrong[0])


def test_the_recorded_lines_are_what_the_rules_say(lines):
    """The golden file against the rules of include/statmc.h written out here, not against the program."""
    got = dict(line.split(" : ", 1) for line in json.load(open(GOLDEN))["cases"])
    # every refusal of one descriptor names types[i]; moments, planes, the epilogue pair
    for ch in (1, 3):
        for name, word in (("max_moment 0", "max_moment"), ("max_moment 4", "max_moment"), ("no m2", "m2"), ("no m3", "m3"),
                           ("transform without film_mean", "film_mean"), ("transform without film_m2", "film_m2"),
                           ("mean_corr alone", "discriminator"), ("discriminator alone", "mean_corr"),
                           ("epilogue with max_moment 2", "max_moment 3"), ("negative n_samples", "n_samples"), ("no n", "null")):
            line = got["type %s c%d" % (name, ch)]
            assert line.startswith("types[7]: ") and word in line, (name, ch, line)
        assert got["type epilogue c%d" % ch].startswith("ok ") and " pre4/3 " in got["type epilogue c%d" % ch]
        assert " pre0/0 " in got["type three moments, transform c%d" % ch]
    # n_types x n_ranges <= 16, named
    assert "n_types" in got["limit n_types 2 x n_ranges 9"] and "n_ranges" in got["limit n_types 2 x n_ranges 9"]
    assert got["limit n_types 2 x n_ranges 8"] == "ok" and got["limit n_types 17 x n_ranges 0"] == "ok"
    assert "n_types" in got["limit n_types 17"] and "n_ranges" not in got["limit n_types 17"]
    assert "n_tiles" in got["limit n_tiles -1"]
    # ranges: outside, reversed, overlapping in either order refused; touching and empty ones valid
    for name in ("rows [0,6)", "rows [-1,2)", "rows [3,2) reversed"):
        assert "outside" in got["film " + name]
    for name in ("rows [0,3) [2,5) overlap", "rows [2,5) [0,3) overlap"):
        assert "overlap" in got["film " + name]
    assert got["film rows [0,2) [2,5) touch"].startswith("ok entries4 ")
    assert got["film rows [2,2) empty"].startswith("ok entries0 ")
    assert "n_ranges" in got["ranges default NULL, 2"] and got["ranges default NULL, 0"] == "ok n_ranges1 [0,5) whole"
    # the pointer advance of rows [3,5): samples, n, mean, m2, m3, film_mean, film_m2, mean_corr, discriminator
    px0 = 3 * 12
    tail = " ".join([str(px0 * 4)] + [str(px0 * 3 * 4)] * 7)
    assert got["film advance f32 rows [3,5) entry 0"].endswith("elems72 stride180 | %d %s" % (px0 * 3 * 4, tail))
    assert got["film advance half rows [3,5) entry 0"].endswith("elems72 stride180 | %d %s" % (px0 * 3 * 2, tail))
    assert got["film advance counted rows [3,5) entry 0"].endswith("| %d %s counts%d" % (px0 * 3 * 4, tail, px0 * 4))
    # the half mask: bit (range x n_types + type) over the non-empty ranges
    assert got["film half mask, 2 ranges x (f32, half, half)"] == "ok entries6 half_mask0x%x" % 0b110110
    assert got["film half mask, 3 ranges x (half, f32, half), one empty"] == "ok entries6 half_mask0x%x" % 0b101101
    # the counted entry drops the middle type, the last one's half bit moves down with it; the uncounted entry keeps all three
    assert got["film counted, middle n_samples 0, last half"] == "ok entries2 half_mask0x2"
    assert got["film counted, middle n_samples 0, last half entry 1"].startswith("type2 ch1 ")
    assert got["film uncounted, the same"] == "ok entries3 half_mask0x4"
    assert got["film counted, middle n_samples 0 without mean"].startswith("types[1]: ")
    # formats, arenas, counts
    assert "sample_formats[0]" in got["formats bad first"] and "sample_formats[1]" in got["formats bad last"]
    assert "odd address" in got["arenas odd half arena"] and got["arenas odd fp32 arena (the kernels' scalar path)"] == "ok"
    for k in (1, 2, 3):
        assert "sample_counts" in got["arenas counts + %d" % k]
    assert got["arenas counts + 4"] == "ok"


def test_the_program_is_clean_under_sanitizers(lines, tmp_path):
    """The same source built with -fsanitize=address,undefined (the header under test is compiled into it) and run on its own:
    no report, the same lines."""
    from statmc_amd import build
    rocm_inc = os.path.join(os.path.dirname(os.path.dirname(build._hipcc())), "include")
    binary = str(tmp_path / "args_sanitized")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-D__HIP_PLATFORM_AMD__", "-I", rocm_inc, "-I", os.path.join(ROOT, "include"), SRC, "-o", binary])
    assert _run(binary) == lines


def test_the_header_is_pure():
    """statmc_accumulate_args.h names no HIP call and keeps no state; beside the C headers it includes the argument blocks only."""
    code = re.sub(r"//.*", "", open(HEADER).read())
    assert "hip" not in code.lower() and not re.search(r"\bstatic\b", code) and "thread_local" not in code
    assert re.findall(r"#include\s+(\S+)", code) == ["<stdarg.h>", "<stdint.h>", "<stdio.h>", '"statmc_device.h"']
