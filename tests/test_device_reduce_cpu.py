"""statmc::device::merge_lanes / merge_waves (include/statmc_device_api.hpp) without a GPU: every instantiation compiles for
gfx950 under hipcc's default flags and is refused under fast math, the example library exports the launchers that use them,
and their kernels' code objects use no scratch."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
# tests/test_combine_many_gpu.py's VARIANTS (channels, max_moment, transform); that module needs torch and a device to import
# (tests/test_device_reduce_gpu.py asserts that the two lists agree)
VARIANTS = [(3, 3, True), (3, 3, False), (3, 2, True), (3, 1, False), (1, 3, True),
            (1, 2, False), (1, 1, True), (1, 1, False), (3, 2, False), (3, 1, True)]
LANES = (2, 4, 8, 16, 32, 64)
WAVES = (2, 4, 8, 16)
NEW_LAUNCHERS = ("fold_arena_lanes", "fold_arena_waves", "gen_fold_lanes")
NEW_KERNELS = ("fold_lanes_kernel", "fold_waves_kernel", "gen_fold_lanes_kernel")

KERNELS = """
#include "statmc_device_api.hpp"
using namespace statmc::device;
template <int G, int C, int M, bool T>
__global__ void lanes(statmc_stat_type t, long long n_px) {
    const long long i = blockIdx.x * 256ll + threadIdx.x, p = i / G;
    PixelStats<C, M, T> ps;
    ps.clear();
    if (p < n_px) ps.load(t, p);
    merge_lanes<G>(ps);
    if (p < n_px && i % G == 0) ps.store(t, p);
}
template <int NW, int C, int M, bool T>
__global__ void waves(statmc_stat_type t, long long n_px) {
    __shared__ float scratch[merge_waves_lds_bytes<NW, C, M, T>() / 4];
    static_assert(merge_waves_lds_bytes<NW, C, M, T>() == 256 * (NW - 1) * (1 + C * (M + (T ? 2 : 0))), "one plane per field and staging wave");
    const long long p = blockIdx.x * 64ll + threadIdx.x % 64;
    PixelStats<C, M, T> ps;
    ps.clear();
    if (p < n_px) ps.load(t, p);
    merge_waves<NW>(ps, scratch);
    if (p < n_px && threadIdx.x < 64) ps.store(t, p);
}
"""


def source():
    src = [KERNELS]
    for c, m, t in VARIANTS:
        targs = "%d, %d, %s" % (c, m, "true" if t else "false")
        for g in LANES:
            src.append("template __global__ void lanes<%d, %s>(statmc_stat_type, long long);" % (g, targs))
        for nw in WAVES:
            src.append("template __global__ void waves<%d, %s>(statmc_stat_type, long long);" % (nw, targs))
    return "\n".join(src) + "\n"


def _hipcc(tmp_path, *flags):
    from statmc_amd import build
    src = tmp_path / "k.hip"
    src.write_text(source())
    return subprocess.run([build._hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-c", *flags, "-I", INCLUDE, str(src),
                           "-o", str(tmp_path / "k.o")], capture_output=True, text=True, timeout=900)


def test_every_instantiation_compiles_for_gfx950_under_hipcc_defaults(tmp_path):
    out = _hipcc(tmp_path)
    assert out.returncode == 0, out.stdout + out.stderr


def test_reductions_are_refused_under_fast_math(tmp_path):
    for flag in ("-ffast-math", "-ffinite-math-only"):
        out = _hipcc(tmp_path, flag)
        assert out.returncode != 0, flag
        assert "statmc_device_api.hpp needs IEEE fp32 semantics" in out.stderr + out.stdout, flag


def test_example_library_exports_the_launchers():
    from statmc_amd import build
    build.build_tools()
    syms = subprocess.check_output(["nm", "-D", "--defined-only", build.DEVICE_EXAMPLE_SO], text=True).split()
    for name in NEW_LAUNCHERS + ("fold_arena_lanes_waves",):
        assert name in syms, name


def kernel_metadata(so, tmp_path):
    """[(kernel name, private segment bytes, LDS bytes, VGPRs)] of the gfx950 code object bundled in a HIP shared library"""
    from statmc_amd import build
    llvm = os.path.join(os.path.dirname(os.path.dirname(build._hipcc())), "llvm", "bin")
    fat, co = str(tmp_path / "fatbin"), str(tmp_path / "co.hsaco")
    subprocess.check_call(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", so, fat])
    subprocess.check_call([os.path.join(llvm, "clang-offload-bundler"), "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                           "--input=" + fat, "--output=" + co, "--unbundle"])
    notes = subprocess.check_output([os.path.join(llvm, "llvm-readelf"), "--notes", co], text=True)
    out = []
    for block in re.split(r"\n\s+- \.agpr_count:", notes)[1:]:
        f = {k: re.search(r"\.%s:\s+(\S+)" % k, block) for k in ("name", "private_segment_fixed_size", "group_segment_fixed_size",
                                                                  "vgpr_count")}
        assert all(f.values()), block[:400]
        out.append((f["name"].group(1), int(f["private_segment_fixed_size"].group(1)), int(f["group_segment_fixed_size"].group(1)),
                    int(f["vgpr_count"].group(1))))
    return out


def test_the_new_kernels_use_no_scratch(tmp_path):
    from statmc_amd import build
    build.build_tools()
    meta = kernel_metadata(build.DEVICE_EXAMPLE_SO, tmp_path)
    for kernel, count in zip(NEW_KERNELS, (72, 48, 6)):   # (6 G | 4 NW) x 12 stat-type shapes; 6 G
        mine = [m for m in meta if re.search(r"\d%sI" % kernel, m[0])]
        assert len(mine) == count, (kernel, len(mine))
        for name, private, lds, vgprs in mine:
            assert private == 0, (name, private)
            assert (lds > 0) == (kernel == "fold_waves_kernel"), (name, lds)
        print("%s: VGPRs %d..%d, LDS %d..%d B" % (kernel, min(m[3] for m in mine), max(m[3] for m in mine),
                                                    min(m[2] for m in mine), max(m[2] for m in mine)))
    rad = [m for m in meta if "fold_waves_kernelILi16ELi3ELi3ELb1E" in m[0]]
    assert len(rad) == 1 and rad[0][2] == 16 * 15 * 256      # [16 fields][15 staging waves][64 lanes] dwords
