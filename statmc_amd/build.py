"""Builds libstatmc_hip.so for gfx950 with hipcc, in-tree (statmc_amd/libstatmc_hip.so)."""
import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
SO = os.path.join(HERE, "libstatmc_hip.so")
DEFAULT_SO = SO
SOURCES = ["statmc_pointwise.hip", "statmc_filter.hip", "statmc_filter_sym.hip", "statmc_placement.hip", "statmc_abi.hip", "statmc_rccl.hip",
           "statmc_records.hip", "statmc_counted.hip", "statmc_pool.hip", "statmc_plan.hip", "statmc_error.hip", "statmc_upsample.hip", "statmc_select.hip", "statmc_score_window.hip", "statmc_score_sum.hip", "statmc_score_tiles.hip", "statmc_tile_select.hip", "statmc_compact.hip", "statmc_state_records.hip"]
HEADERS = ["statmc_device.h", "statmc_scan.h", "statmc_state_records_args.h", "statmc_compact_args.h", "statmc_compact_interleaved_args.h", "statmc_record_field.h", "statmc_accumulate_fold.h", "statmc_accumulate_args.h", "statmc_records_plan.h", "statmc_pool_args.h", "statmc_plan_args.h", "statmc_error_args.h", "statmc_upsample_args.h", "statmc_select_args.h", "statmc_score_window_args.h", "statmc_score_sum_args.h", "statmc_score_tiles_args.h", "statmc_tile_select_args.h", "statmc_filter_common.h", "t_quantiles.h", os.path.join("..", "..", "include", "statmc.h"),
           os.path.join("..", "..", "include", "statmc_pinned_spec.h"), os.path.join("..", "..", "include", "statmc_device_api.hpp")]
# -ffp-contract=off: every fp32 op rounds once, in source order, like the CPU oracle build.
FLAGS = ["-O3", "--offload-arch=gfx950", "-std=c++17", "-fPIC", "-ffp-contract=off",
         "-fno-fast-math", "-fno-slp-vectorize", "-Wall", "-Wno-unused-function"]
# The hot loops are written in the order they should issue (stage by stage across a lane's pixels,
# loads ahead of the folds); the pre-RA machine scheduler only loses against that order: window filter
# 2.44 -> 2.40 ms, radiance accumulation 1.40 -> 1.30 ms in A/B builds on one box.
KERNEL_FLAGS = ["-mllvm", "-enable-misched=0"]


def _hipcc():
    for c in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if c and os.path.exists(c):
            return c
    raise RuntimeError("hipcc not found: libstatmc_hip.so cannot be built")


STAMP = DEFAULT_SO + ".src"   # hash of the sources + flags the library was built from (git-ignored, ships with the .so)


def source_hash():
    import hashlib
    h = hashlib.sha256()
    for name in SOURCES + HEADERS:
        with open(os.path.join(CSRC, name), "rb") as f:
            h.update(name.encode() + b"\0" + f.read())
    h.update(" ".join(FLAGS + KERNEL_FLAGS).encode())
    return h.hexdigest()


def stale():
    """True when libstatmc_hip.so exists but was built from other sources than the ones in csrc/ (mtimes do not
    survive a snapshot copy of the tree, a content hash does)."""
    if not os.path.exists(SO):
        return False
    try:
        return open(STAMP).read().strip() != source_hash()
    except OSError:
        return True


def needs_build():
    """A missing library or one built from other sources.  The rebuild goes to a temporary file and is renamed into
    place, so a process that has the old library mapped keeps a consistent image."""
    return not os.path.exists(SO) or stale()


def build(force=False, verbose=False):
    if not force and not needs_build():
        return SO
    hipcc = _hipcc()
    objs = []
    procs = []
    for src in SOURCES:
        obj = os.path.join(CSRC, src.replace(".hip", ".o"))
        objs.append(obj)
        extra = KERNEL_FLAGS if src not in ("statmc_abi.hip", "statmc_placement.hip", "statmc_rccl.hip") else []
        cmd = [hipcc] + FLAGS + extra + ["-c", os.path.join(CSRC, src), "-o", obj]
        if verbose:
            print(" ".join(cmd), file=sys.stderr)
        procs.append((cmd, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)))
    for cmd, p in procs:
        out, _ = p.communicate()
        if p.returncode != 0:
            raise RuntimeError("hipcc failed: %s\n%s" % (" ".join(cmd), out.decode()))
        if verbose and out:
            print(out.decode(), file=sys.stderr)
    tmp = SO + ".tmp.%d" % os.getpid()
    cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", tmp] + objs
    subprocess.check_call(cmd)
    os.replace(tmp, SO)
    with open(STAMP, "w") as f:
        f.write(source_hash() + "\n")
    return SO


ROOT = os.path.dirname(HERE)
DENOISE_BIN = os.path.join(ROOT, "tools", "bin", "statmc_denoise")
RENDER_SIM_BIN = os.path.join(ROOT, "tools", "bin", "statmc_render_sim")
CV_ADAPTOR_BIN = os.path.join(ROOT, "tools", "bin", "test_cv_adaptor")   # tests/cpp/test_cv_adaptor.cpp: include/statmc_cv.hpp in use
DEVICE_ACC_BIN = os.path.join(ROOT, "tools", "bin", "test_device_accumulate")   # tests/cpp/test_device_accumulate.cpp: Estimator::DeviceStatistics
ACC_RECORDS_BIN = os.path.join(ROOT, "tools", "bin", "test_accumulate_records")   # tests/cpp/test_accumulate_records.cpp: Estimator::AccumulateRecords
ACC_FILM_BIN = os.path.join(ROOT, "tools", "bin", "test_accumulate_film")   # tests/cpp/test_accumulate_film.cpp: Estimator::AccumulateFilm
ACC_PLAN_BIN = os.path.join(ROOT, "tools", "bin", "test_accumulate_plan")   # tests/cpp/test_accumulate_plan.cpp: statmc::plan_accumulate, no device
REC_ILV_PLAN_BIN = os.path.join(ROOT, "tools", "bin", "test_records_interleaved_plan")   # tests/cpp/test_records_interleaved_plan.cpp: statmc_records_plan.h, no device, no library
REC_ILV_BIN = os.path.join(ROOT, "tools", "bin", "test_accumulate_records_interleaved")   # tests/cpp/test_accumulate_records_interleaved.cpp: Estimator::AccumulateRecordsInterleaved
REC_SPLIT_PLAN_BIN = os.path.join(ROOT, "tools", "bin", "test_records_split_plan")   # tests/cpp/test_records_split_plan.cpp: the split entries' chunk rule, no device, no library
REC_SPLIT_BIN = os.path.join(ROOT, "tools", "bin", "test_accumulate_records_split")   # tests/cpp/test_accumulate_records_split.cpp: Estimator::AccumulateRecords(..., splitAbove)
ACC_ARGS_BIN = os.path.join(ROOT, "tools", "bin", "test_accumulate_args")   # tests/cpp/test_accumulate_args.cpp: statmc_accumulate_args.h, no device, no library
ACC_COUNTED_BIN = os.path.join(ROOT, "tools", "bin", "test_accumulate_counted")   # tests/cpp/test_accumulate_counted.cpp: ragged StatTiles, Estimator::AccumulateFilm(..., d_counts)
POOL_ARGS_BIN = os.path.join(ROOT, "tools", "bin", "test_pool_args")   # tests/cpp/test_pool_args.cpp: statmc_pool_args.h, no device, no library
POOL_BIN = os.path.join(ROOT, "tools", "bin", "test_pool_statistics")   # tests/cpp/test_pool_statistics.cpp: Estimator::PoolStatistics
PLAN_ARGS_BIN = os.path.join(ROOT, "tools", "bin", "test_plan_args")   # tests/cpp/test_plan_args.cpp: statmc_plan_args.h, no device, no library
PLAN_BIN = os.path.join(ROOT, "tools", "bin", "test_plan_samples")   # tests/cpp/test_plan_samples.cpp: Estimator::PlanSamples
SELECT_ARGS_BIN = os.path.join(ROOT, "tools", "bin", "test_select_args")   # tests/cpp/test_select_args.cpp: statmc_select_args.h, no device, no library
SELECT_BIN = os.path.join(ROOT, "tools", "bin", "test_score_select")   # tests/cpp/test_score_select.cpp: Estimator::ScoreSelect / ScoreCountAbove
WINDOW_ARGS_BIN = os.path.join(ROOT, "tools", "bin", "test_score_window_args")   # tests/cpp/test_score_window_args.cpp: statmc_score_window_args.h, no device, no library
SUM_ARGS_BIN = os.path.join(ROOT, "tools", "bin", "test_score_sum_args")   # tests/cpp/test_score_sum_args.cpp: statmc_score_sum_args.h, no device, no library
TILES_ARGS_BIN = os.path.join(ROOT, "tools", "bin", "test_score_tiles_args")   # tests/cpp/test_score_tiles_args.cpp: statmc_score_tiles_args.h, no device, no library
TILE_SELECT_ARGS_BIN = os.path.join(ROOT, "tools", "bin", "test_tile_select_args")   # tests/cpp/test_tile_select_args.cpp: statmc_tile_select_args.h, no device, no library
WINDOW_BIN = os.path.join(ROOT, "tools", "bin", "test_score_window")   # tests/cpp/test_score_window.cpp: Estimator::PlanSamples(..., scoreDilate) / ScoreWindow
COMPACT_ARGS_BIN = os.path.join(ROOT, "tools", "bin", "test_compact_args")   # tests/cpp/test_compact_args.cpp: statmc_compact_args.h, no device, no library
COMPACT_ILV_ARGS_BIN = os.path.join(ROOT, "tools", "bin", "test_compact_interleaved_args")   # tests/cpp/test_compact_interleaved_args.cpp: statmc_compact_interleaved_args.h, no device, no library
COMPACT_ILV_BIN = os.path.join(ROOT, "tools", "bin", "test_compact_accumulate_interleaved")   # tests/cpp/test_compact_accumulate_interleaved.cpp: Estimator::AccumulateCompactInterleaved
COMPACT_BIN = os.path.join(ROOT, "tools", "bin", "test_compact_accumulate")   # tests/cpp/test_compact_accumulate.cpp: Estimator::CompactOffsets / AccumulateCompact
STATE_ARGS_BIN = os.path.join(ROOT, "tools", "bin", "test_state_records_args")   # tests/cpp/test_state_records_args.cpp: statmc_state_records_args.h, no device, no library
STATE_BIN = os.path.join(ROOT, "tools", "bin", "test_state_records")   # tests/cpp/test_state_records.cpp: Estimator::GatherStates / CombineRecords
ERROR_ARGS_BIN = os.path.join(ROOT, "tools", "bin", "test_error_args")   # tests/cpp/test_error_args.cpp: statmc_error_args.h, no device, no library
TARGET_BIN = os.path.join(ROOT, "tools", "bin", "test_plan_to_target")   # tests/cpp/test_plan_to_target.cpp: Estimator::PlanToTarget / scoreOf
UPSAMPLE_ARGS_BIN = os.path.join(ROOT, "tools", "bin", "test_upsample_args")   # tests/cpp/test_upsample_args.cpp: statmc_upsample_args.h, no device, no library
TOOLS = {DENOISE_BIN: "statmc_denoise.cpp", RENDER_SIM_BIN: "statmc_render_sim.cpp",
         UPSAMPLE_ARGS_BIN: os.path.join("..", "tests", "cpp", "test_upsample_args.cpp"),
         ERROR_ARGS_BIN: os.path.join("..", "tests", "cpp", "test_error_args.cpp"),
         TARGET_BIN: os.path.join("..", "tests", "cpp", "test_plan_to_target.cpp"),
         CV_ADAPTOR_BIN: os.path.join("..", "tests", "cpp", "test_cv_adaptor.cpp"),
         DEVICE_ACC_BIN: os.path.join("..", "tests", "cpp", "test_device_accumulate.cpp"),
         ACC_RECORDS_BIN: os.path.join("..", "tests", "cpp", "test_accumulate_records.cpp"),
         ACC_FILM_BIN: os.path.join("..", "tests", "cpp", "test_accumulate_film.cpp"),
         ACC_PLAN_BIN: os.path.join("..", "tests", "cpp", "test_accumulate_plan.cpp"),
         ACC_ARGS_BIN: os.path.join("..", "tests", "cpp", "test_accumulate_args.cpp"),
         REC_ILV_PLAN_BIN: os.path.join("..", "tests", "cpp", "test_records_interleaved_plan.cpp"),
         REC_ILV_BIN: os.path.join("..", "tests", "cpp", "test_accumulate_records_interleaved.cpp"),
         REC_SPLIT_PLAN_BIN: os.path.join("..", "tests", "cpp", "test_records_split_plan.cpp"),
         REC_SPLIT_BIN: os.path.join("..", "tests", "cpp", "test_accumulate_records_split.cpp"),
         ACC_COUNTED_BIN: os.path.join("..", "tests", "cpp", "test_accumulate_counted.cpp"),
         POOL_ARGS_BIN: os.path.join("..", "tests", "cpp", "test_pool_args.cpp"),
         POOL_BIN: os.path.join("..", "tests", "cpp", "test_pool_statistics.cpp"),
         PLAN_ARGS_BIN: os.path.join("..", "tests", "cpp", "test_plan_args.cpp"),
         PLAN_BIN: os.path.join("..", "tests", "cpp", "test_plan_samples.cpp"),
         SELECT_ARGS_BIN: os.path.join("..", "tests", "cpp", "test_select_args.cpp"),
         SELECT_BIN: os.path.join("..", "tests", "cpp", "test_score_select.cpp"),
         WINDOW_ARGS_BIN: os.path.join("..", "tests", "cpp", "test_score_window_args.cpp"),
         WINDOW_BIN: os.path.join("..", "tests", "cpp", "test_score_window.cpp"),
         SUM_ARGS_BIN: os.path.join("..", "tests", "cpp", "test_score_sum_args.cpp"),
         TILES_ARGS_BIN: os.path.join("..", "tests", "cpp", "test_score_tiles_args.cpp"),
         TILE_SELECT_ARGS_BIN: os.path.join("..", "tests", "cpp", "test_tile_select_args.cpp"),
         COMPACT_ARGS_BIN: os.path.join("..", "tests", "cpp", "test_compact_args.cpp"),
         COMPACT_ILV_ARGS_BIN: os.path.join("..", "tests", "cpp", "test_compact_interleaved_args.cpp"),
         COMPACT_ILV_BIN: os.path.join("..", "tests", "cpp", "test_compact_accumulate_interleaved.cpp"),
         COMPACT_BIN: os.path.join("..", "tests", "cpp", "test_compact_accumulate.cpp"),
         STATE_ARGS_BIN: os.path.join("..", "tests", "cpp", "test_state_records_args.cpp"),
         STATE_BIN: os.path.join("..", "tests", "cpp", "test_state_records.cpp")}
# A renderer's own kernel accumulating through include/statmc_device_api.hpp (tools/device_accumulate_example.hip), built with
# hipcc's DEFAULT floating-point flags -- not the library's -ffp-contract=off: the header's bits must not depend on them.
DEVICE_EXAMPLE_SO = os.path.join(ROOT, "tools", "bin", "libstatmc_device_example.so")
DEVICE_EXAMPLE_SRC = "device_accumulate_example.hip"
DEVICE_EXAMPLE_FLAGS = ["-O3", "--offload-arch=gfx950", "-std=c++17", "-fPIC", "-shared"]


TOOLS_STAMP = os.path.join(os.path.dirname(DENOISE_BIN), ".src")


def tools_hash():
    """Content hash of what the host tools are compiled from: their sources and every header under include/."""
    import hashlib
    h = hashlib.sha256()
    inc = os.path.join(ROOT, "include")
    files = [os.path.join(ROOT, "tools", src) for src in list(TOOLS.values()) + [DEVICE_EXAMPLE_SRC]]
    files += [os.path.join(inc, f) for f in sorted(os.listdir(inc))]
    files.append(os.path.join(CSRC, "statmc_device.h"))    # test_accumulate_plan.cpp reads the library's own argument blocks
    files.append(os.path.join(CSRC, "statmc_accumulate_args.h"))    # ... test_accumulate_args.cpp the accumulation entries' checks and fills
    files.append(os.path.join(CSRC, "statmc_records_plan.h"))    # ... test_records_interleaved_plan.cpp the records entries' host decisions
    files.append(os.path.join(CSRC, "statmc_pool_args.h"))    # ... test_pool_args.cpp the pooling entry's checks
    files.append(os.path.join(CSRC, "statmc_plan_args.h"))    # ... test_plan_args.cpp the planning entries' checks
    files.append(os.path.join(CSRC, "statmc_error_args.h"))    # ... test_error_args.cpp the error entries' checks
    files.append(os.path.join(CSRC, "statmc_upsample_args.h"))    # ... test_upsample_args.cpp the upsampling entry's checks
    files.append(os.path.join(CSRC, "statmc_select_args.h"))  # ... test_select_args.cpp the order-statistics entries' checks
    files.append(os.path.join(CSRC, "statmc_score_window_args.h"))    # ... test_score_window_args.cpp the window entry's checks
    files.append(os.path.join(CSRC, "statmc_score_sum_args.h"))    # ... test_score_sum_args.cpp the sum entry's checks and finalisation
    files.append(os.path.join(CSRC, "statmc_score_tiles_args.h"))    # ... test_score_tiles_args.cpp the tile entry's checks and finalisation
    files.append(os.path.join(CSRC, "statmc_tile_select_args.h"))    # ... test_tile_select_args.cpp the tile select's and the gate's checks and host evaluation
    files.append(os.path.join(CSRC, "statmc_compact_args.h"))    # ... test_compact_args.cpp the compact entries' checks
    files.append(os.path.join(CSRC, "statmc_compact_interleaved_args.h"))    # ... and test_compact_interleaved_args.cpp the interleaved compact entry's
    files.append(os.path.join(CSRC, "statmc_state_records_args.h"))    # ... and test_state_records_args.cpp the state-record entries'
    for path in files:
        with open(path, "rb") as f:
            h.update(os.path.basename(path).encode() + b"\0" + f.read())
    return h.hexdigest()


def tools_stale():
    try:
        return open(TOOLS_STAMP).read().strip() != tools_hash()
    except OSError:
        return True


def build_tools(force=False):
    """g++ build of the C++ host side (include/statmc_denoiser.hpp + tools/*.cpp: the offline
    denoise driver and the render-loop harness), linked against libstatmc_hip.so, and the hipcc build of the
    device-side accumulation example (tools/bin/libstatmc_device_example.so)."""
    # Binaries built from other sources than the ones in the tree are rebuilt (content hash: mtimes do not survive a
    # snapshot copy of the tree); each goes to a temporary file and is renamed into place.
    if not force and all(os.path.exists(b) for b in list(TOOLS) + [DEVICE_EXAMPLE_SO]) and not tools_stale():
        return DENOISE_BIN
    if not os.path.exists(SO):
        build()
    os.makedirs(os.path.dirname(DENOISE_BIN), exist_ok=True)
    rocm_lib = os.path.join(os.path.dirname(os.path.dirname(_hipcc())), "lib")
    rocm_inc = os.path.join(os.path.dirname(rocm_lib), "include")
    tmp = DEVICE_EXAMPLE_SO + ".tmp%d" % os.getpid()
    subprocess.check_call([_hipcc()] + DEVICE_EXAMPLE_FLAGS + ["-I", os.path.join(ROOT, "include"),
                                                             os.path.join(ROOT, "tools", DEVICE_EXAMPLE_SRC), "-o", tmp])
    os.replace(tmp, DEVICE_EXAMPLE_SO)
    for binary, src in TOOLS.items():
        tmp = binary + ".tmp%d" % os.getpid()
        extra = ["-L", os.path.dirname(DEVICE_EXAMPLE_SO), "-lstatmc_device_example", "-Wl,-rpath,$ORIGIN"] if binary == DEVICE_ACC_BIN else []
        if binary in (ACC_PLAN_BIN, ACC_ARGS_BIN, COMPACT_ARGS_BIN, COMPACT_ILV_ARGS_BIN, STATE_ARGS_BIN):      # statmc_device.h includes the HIP runtime's header
            extra = ["-D__HIP_PLATFORM_AMD__", "-I", rocm_inc]
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-ffp-contract=off", "-pthread",
                               "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", src), "-o", tmp,
                               "-L", HERE, "-lstatmc_hip"] + extra + ["-L", rocm_lib, "-Wl,-rpath,$ORIGIN/../../statmc_amd",
                               "-Wl,-rpath," + rocm_lib])
        os.replace(tmp, binary)
    with open(TOOLS_STAMP, "w") as f:
        f.write(tools_hash() + "\n")
    return DENOISE_BIN


if __name__ == "__main__":
    print(build(force=True, verbose="-v" in sys.argv))
    print(build_tools(force=True))
