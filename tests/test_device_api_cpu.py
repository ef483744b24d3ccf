"""include/statmc_device_api.hpp and statmc_get_prepass_context without a GPU: the C entry point and its struct, the header
under hipcc's default flags (and refused under fast math), and the example library build_tools() makes."""
import ctypes as C
import os
import subprocess
import sys
import textwrap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")


def test_prepass_context_is_exported_and_needs_setup():
    from statmc_amd import api, build
    build.build()
    assert "statmc_get_prepass_context" in api.EXPORTS
    # a fresh process that never called statmc_setup (no device visible either way)
    code = textwrap.dedent("""
        import ctypes as C
        from statmc_amd import api
        lib = api.load()
        ctx = api.PrepassContext()
        print(lib.statmc_get_prepass_context(C.byref(ctx)), lib.statmc_get_prepass_context(None))
    """)
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, env=env, timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split() == [str(api.ERR_NO_DEVICE), str(api.ERR_INVALID)]


def test_prepass_context_layout_matches_gcc(tmp_path):
    from statmc_amd import api
    src = tmp_path / "t.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "statmc.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu\\n", sizeof(statmc_prepass_context), offsetof(statmc_prepass_context, t_table),\n'
                   '                        offsetof(statmc_prepass_context, flags), offsetof(statmc_prepass_context, reserved)); return 0; }\n')
    subprocess.check_call(["gcc", "-I", INCLUDE, str(src), "-o", str(tmp_path / "t")])
    got = [int(v) for v in subprocess.check_output([str(tmp_path / "t")], text=True).split()]
    P = api.PrepassContext
    assert got == [C.sizeof(P), P.t_table.offset, P.flags.offset, P.reserved.offset] == [16, 0, 8, 12]


KERNEL = """
#include "statmc_device_api.hpp"
template <int C, int M, bool T>
__global__ void k(statmc_stat_type t, const float *smp, int S, statmc_prepass_context ctx) {
    statmc::device::PixelStats<C, M, T> ps;
    const long long p = blockIdx.x * 64 + threadIdx.x;
    ps.load(t, p);
    for (int s = 0; s < S; s++) ps.add(smp + (s * 4096 + p) * C);
    if constexpr (M == 3) ps.store(t, p, ctx); else ps.store(t, p);
}
template __global__ void k<3, 3, true>(statmc_stat_type, const float *, int, statmc_prepass_context);
template __global__ void k<1, 2, false>(statmc_stat_type, const float *, int, statmc_prepass_context);
template __global__ void k<3, 1, false>(statmc_stat_type, const float *, int, statmc_prepass_context);
"""


def _hipcc(tmp_path, *flags):
    from statmc_amd import build
    src = tmp_path / "k.hip"
    src.write_text(KERNEL)
    return subprocess.run([build._hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-c", *flags, "-I", INCLUDE, str(src),
                           "-o", str(tmp_path / "k.o")], capture_output=True, text=True, timeout=600)


def test_header_compiles_for_gfx950_under_hipcc_defaults(tmp_path):
    out = _hipcc(tmp_path)
    assert out.returncode == 0, out.stdout + out.stderr


def test_header_refuses_fast_math(tmp_path):
    for flag in ("-ffast-math", "-ffinite-math-only"):
        out = _hipcc(tmp_path, flag)
        assert out.returncode != 0, flag
        assert "statmc_device_api.hpp needs IEEE fp32 semantics" in out.stderr + out.stdout, flag


def test_example_library_is_built():
    from statmc_amd import build
    build.build_tools()
    assert os.path.exists(build.DEVICE_EXAMPLE_SO) and os.path.exists(build.DEVICE_ACC_BIN)
    syms = subprocess.check_output(["nm", "-D", "--defined-only", build.DEVICE_EXAMPLE_SO], text=True).split()
    for name in ("fold_arena", "gen_arena", "gen_fold"):
        assert name in syms, name
