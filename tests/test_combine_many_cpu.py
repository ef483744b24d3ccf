"""No-GPU checks of statmc_combine_many (include/statmc.h) and statmc::device::PixelStats::merge
(include/statmc_device_api.hpp): exported, laid out as the ctypes mirror says, refused without a device, the device header
with merge under hipcc's default flags (and refused under fast math), and the example library's slot-merging launcher."""
import ctypes as C
import os
import subprocess
import sys
import textwrap

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")


@pytest.fixture(scope="module")
def lib():
    from statmc_amd import api, build
    build.build()
    return api.load()


def test_combine_many_is_exported(lib):
    from statmc_amd import api
    assert hasattr(lib, "statmc_combine_many")
    assert "statmc_combine_many" in api.EXPORTS
    assert lib.statmc_version() == 101
    syms = subprocess.check_output(["nm", "-D", "--defined-only", api.load()._name], text=True).split()
    assert "statmc_combine_many" in syms


def test_combine_many_entry_layout_matches_header(lib, tmp_path):
    from statmc_amd import api
    src = tmp_path / "t.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "statmc.h"\n'
                   'int main(void) {\n'
                   '  printf("%zu %zu %zu %zu %d\\n", sizeof(statmc_combine_many_entry), offsetof(statmc_combine_many_entry, dst),\n'
                   '         offsetof(statmc_combine_many_entry, srcs), offsetof(statmc_combine_many_entry, count_of),\n'
                   '         STATMC_MAX_COMBINE_SOURCES);\n'
                   '  return 0;\n}\n')
    subprocess.check_call(["gcc", "-I", INCLUDE, str(src), "-o", str(tmp_path / "t")])
    got = [int(x) for x in subprocess.check_output([str(tmp_path / "t")]).split()]
    ce = api.CombineManyEntry
    assert got == [C.sizeof(ce), ce.dst.offset, ce.srcs.offset, ce.count_of.offset, api.MAX_COMBINE_SOURCES]
    assert api.MAX_COMBINE_SOURCES == 15


def test_make_combine_many_entry_keeps_its_sources():
    import torch
    from statmc_amd import api
    st = lambda: {"n": torch.zeros(2, 4, dtype=torch.int32), "mean": torch.zeros(2, 4, 3)}
    dst, srcs = st(), [st(), st(), st()]
    e = api.make_combine_many_entry(dst, srcs, 3, 1)
    assert e.count_of == -1 and e.dst.n == dst["n"].data_ptr() and e._n_sources == 3
    for k, s in enumerate(srcs):
        assert e.srcs[k].mean == s["mean"].data_ptr() and e.srcs[k].n == s["n"].data_ptr()
        assert e.srcs[k].channels == 3 and e.srcs[k].max_moment == 1
    b = api.make_combine_many_entry({"mean": dst["mean"]}, [{"mean": s["mean"]} for s in srcs], 3, 1, count_of=0)
    assert b.count_of == 0 and not b.dst.n and not b.srcs[2].n


def test_combine_many_without_a_device_is_an_error():
    """A fresh process that never called statmc_setup (no device visible either way)."""
    from statmc_amd import api, build
    build.build()
    code = textwrap.dedent("""
        from statmc_amd import api
        lib = api.load()
        e = (api.CombineManyEntry * 1)()
        print(lib.statmc_combine_many(8, 8, e, 1, 1, None), lib.statmc_combine_many(8, 8, None, 0, 0, None))
        print(lib.statmc_last_error().decode())
    """)
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, env=env, timeout=120)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    assert lines[0].split() == [str(api.ERR_NO_DEVICE)] * 2
    assert "setup" in lines[1]


KERNEL = """
#include "statmc_device_api.hpp"
template <int C, int M, bool T>
__global__ void k(statmc_stat_type t, statmc_stat_type o, const float *smp, int S, int slots) {
    using PS = statmc::device::PixelStats<C, M, T>;
    const long long p = blockIdx.x * 64 + threadIdx.x;
    PS ps, other;
    ps.load(t, p);
    other.load(o, p);
    ps.merge(other);
    for (int k = 0; k < slots; k++) {
        PS slot;
        slot.clear();
        for (int s = k; s < S; s += slots) slot.add(smp + (s * 4096 + p) * C);
        ps.merge(slot);
    }
    ps.store(t, p);
}
#define K(C, M, T) template __global__ void k<C, M, T>(statmc_stat_type, statmc_stat_type, const float *, int, int);
K(1, 1, false) K(1, 2, false) K(1, 3, false) K(1, 1, true) K(1, 2, true) K(1, 3, true)
K(3, 1, false) K(3, 2, false) K(3, 3, false) K(3, 1, true) K(3, 2, true) K(3, 3, true)
"""


def _hipcc(tmp_path, *flags):
    from statmc_amd import build
    src = tmp_path / "k.hip"
    src.write_text(KERNEL)
    return subprocess.run([build._hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-c", *flags, "-I", INCLUDE, str(src),
                           "-o", str(tmp_path / "k.o")], capture_output=True, text=True, timeout=900)


def test_merge_compiles_for_gfx950_under_hipcc_defaults(tmp_path):
    """merge for C in {1, 3}, max_moment in {1, 2, 3} and both transform values."""
    out = _hipcc(tmp_path)
    assert out.returncode == 0, out.stdout + out.stderr


def test_header_with_merge_refuses_fast_math(tmp_path):
    out = _hipcc(tmp_path, "-ffast-math")
    assert out.returncode != 0
    assert "statmc_device_api.hpp needs IEEE fp32 semantics" in out.stderr + out.stdout


def test_example_library_has_the_slot_launcher():
    from statmc_amd import build
    build.build_tools()
    syms = subprocess.check_output(["nm", "-D", "--defined-only", build.DEVICE_EXAMPLE_SO], text=True).split()
    assert "fold_arena_slots" in syms
