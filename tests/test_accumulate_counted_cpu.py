"""Per-pixel sample counts without a GPU: the declaration and binding of statmc_accumulate_counted / statmc_accumulate_tiles_counted,
their argument checks, which are reported before anything touches a device, and ragged tiles in the staging of a dry-run
statmc::Estimator (tests/cpp/test_accumulate_counted_host.cpp, a stand-alone program built by g++ with and without
AddressSanitizer + UBSan)."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from statmc_amd import api
    return api.load()


def stat_types(api, n, samples=0x1000, n_samples=4):
    """Descriptors that pass every host-side check (no call below gets as far as reading through them)."""
    types = (api.StatType * max(n, 1))()
    for t in types:
        t.channels, t.transform, t.max_moment, t.n_samples = 3, 0, 1, n_samples
        t.samples, t.n, t.mean = samples, 0x2000, 0x3000
    return types


def formats(*f):
    return (C.c_int32 * max(len(f), 1))(*f)


def ranges(*r):
    return (C.c_int32 * max(len(r), 1))(*r)


COUNTS = 0x7000          # a 16-byte aligned address nobody reads
FILM_DECL = ("uint16_t width, uint16_t height, const statmc_stat_type *types, const int32_t *sample_formats, int n_types, "
             "const int32_t *sample_counts, const int32_t *ranges, int n_ranges, void *stream")
TILES_DECL = ("uint16_t width, uint16_t height, const statmc_stat_type *types, const int32_t *sample_formats, int n_types, "
              "const int32_t *tile_bounds, const int64_t *tile_offsets, const int32_t *tile_samples, int n_tiles, "
              "const int32_t *sample_counts, void *stream")


def film_call(lib, types, fmts, n_types, counts=COUNTS, rng=None, n_ranges=0):
    return lib.statmc_accumulate_counted(8, 8, types, fmts, n_types, counts, rng, n_ranges, None)


def tiles_call(lib, types, fmts, n_types, counts=COUNTS, n_tiles=1):
    return lib.statmc_accumulate_tiles_counted(8, 8, types, fmts, n_types, 0x4000, 0x5000, 0x6000, n_tiles, counts, None)


def test_entries_are_exported_declared_and_bound(lib):
    import inspect
    from statmc_amd import api, film
    header = open(os.path.join(ROOT, "include", "statmc.h")).read()
    for name, want, n_args in (("statmc_accumulate_counted", FILM_DECL, 9), ("statmc_accumulate_tiles_counted", TILES_DECL, 11)):
        assert hasattr(lib, name)
        assert name in api.EXPORTS
        decl = re.search(r"int\s+%s\s*\(([^;]*)\)\s*;" % name, header)
        assert decl, "include/statmc.h does not declare %s" % name
        assert " ".join(decl.group(1).split()) == want
        assert len(getattr(lib, name).argtypes) == n_args
    assert "sample_counts" in inspect.signature(api.accumulate).parameters
    assert "sample_counts" in inspect.signature(api.accumulate_tiles).parameters
    assert "counts" in inspect.signature(film.FilmStats.accumulate).parameters
    debug = open(os.path.join(ROOT, "include", "statmc_debug.h")).read()
    assert re.search(r"int\s+statmc_debug_last_accumulate_counted\s*\(void\)\s*;", debug)
    assert hasattr(lib, "statmc_debug_last_accumulate_counted") and callable(api.last_accumulate_counted)
    hpp = open(os.path.join(ROOT, "include", "statmc_denoiser.hpp")).read()
    assert "const int32_t *d_counts)" in hpp and "size_t countedFlushes()" in hpp


@pytest.mark.parametrize("counts", [COUNTS + 1, COUNTS + 2, COUNTS + 3])
def test_misaligned_counts_are_refused_before_any_device_work(lib, counts):
    from statmc_amd import api
    types = stat_types(api, 2)
    for call in (film_call, tiles_call):
        for fmts in (None, formats(0, 1)):
            assert call(lib, types, fmts, 2, counts=counts) == api.ERR_INVALID
            assert b"sample_counts" in lib.statmc_last_error()


@pytest.mark.parametrize("bad", [2, -1])
def test_unknown_formats_are_refused_before_any_device_work(lib, bad):
    from statmc_amd import api
    types = stat_types(api, 2)
    for call in (film_call, tiles_call):
        for fmts in (formats(bad, 0), formats(1, bad)):
            assert call(lib, types, fmts, 2) == api.ERR_INVALID
            assert b"sample_formats" in lib.statmc_last_error()


def test_limits_and_odd_arenas_are_refused_before_any_device_work(lib):
    from statmc_amd import api
    types = stat_types(api, 17)
    for call in (film_call, tiles_call):
        assert call(lib, types, formats(*([1] * 17)), 17) == api.ERR_INVALID
        assert b"n_types" in lib.statmc_last_error()
        assert call(lib, types, None, -1) == api.ERR_INVALID
        assert b"n_types" in lib.statmc_last_error()
    # n_types x n_ranges <= 16, and a range count needs ranges
    nine = ranges(*[v for r in range(9) for v in (r % 8, r % 8)])
    assert film_call(lib, stat_types(api, 2), None, 2, rng=nine, n_ranges=9) == api.ERR_INVALID
    assert b"n_ranges" in lib.statmc_last_error()
    assert film_call(lib, stat_types(api, 2), None, 2, rng=None, n_ranges=2) == api.ERR_INVALID
    assert b"n_ranges" in lib.statmc_last_error()
    assert film_call(lib, stat_types(api, 2), None, 2, rng=ranges(0, 8), n_ranges=-1) == api.ERR_INVALID
    assert tiles_call(lib, stat_types(api, 2), None, 2, n_tiles=-1) == api.ERR_INVALID
    assert b"n_tiles" in lib.statmc_last_error()
    odd = stat_types(api, 2, samples=0x1001)
    for call in (film_call, tiles_call):
        assert call(lib, odd, formats(0, 1), 2) == api.ERR_INVALID
        assert b"odd address" in lib.statmc_last_error()
        assert call(lib, None, formats(0, 1), 2) == api.ERR_INVALID


def test_refuses_to_run_before_setup(lib):
    """Argument checks first, then the device: with counts and -- the uncounted entries' own order -- without."""
    import torch
    from statmc_amd import api
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    types = stat_types(api, 2)
    for call in (film_call, tiles_call):
        for fmts in (formats(1, 1), formats(0, 1), formats(0, 0), None):
            assert call(lib, types, fmts, 2) == api.ERR_NO_DEVICE
            assert call(lib, types, fmts, 2, counts=None) == api.ERR_NO_DEVICE
        assert call(lib, types, None, 0) == api.ERR_NO_DEVICE
        assert call(lib, types, formats(2, 0), 2) == api.ERR_INVALID           # ... never the other way round
    assert lib.statmc_debug_last_accumulate_counted() == 0


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_estimator_stages_ragged_tiles(sanitize, tmp_path):
    """Ragged StatTiles merge, the slot rectangle, S, the staged block and counts and stagedBytes() are what include/statmc_denoiser.hpp
    says, a uniform flush stages no counts, and types whose per-pixel counts disagree are refused."""
    from statmc_amd import build
    build.build()
    exe = str(tmp_path / "test_accumulate_counted_host")
    rocm_lib = os.path.join(os.path.dirname(os.path.dirname(build._hipcc())), "lib")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-pthread"] + flags +
                          ["-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_accumulate_counted_host.cpp"), "-o", exe,
                           "-L", os.path.dirname(build.SO), "-lstatmc_hip", "-L", rocm_lib,
                           "-Wl,-rpath," + os.path.dirname(build.SO), "-Wl,-rpath," + rocm_lib])
    # (no device is visible to the program, on a GPU box too: tests/test_host_cpu.py)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:protect_shadow_gap=0", ROCR_VISIBLE_DEVICES="-1", HIP_VISIBLE_DEVICES="-1")
    out = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "accumulate counted host ok" in out.stdout
