"""The IEEE-half tile feed without a GPU: statmc::floatToHalfBits against numpy bit for bit, the half staging of
statmc::Estimator in a dry run (tests/cpp/test_tile_half.cpp, a stand-alone program built by g++ with AddressSanitizer + UBSan),
the declaration and binding of statmc_accumulate_tiles_formats, and its argument checks, which are reported before anything
touches a device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    from statmc_amd import build
    build.build()
    exe = str(tmp_path_factory.mktemp("tile_half") / "test_tile_half")
    rocm_lib = os.path.join(os.path.dirname(os.path.dirname(build._hipcc())), "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-pthread", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_tile_half.cpp"), "-o", exe,
                           "-L", os.path.dirname(build.SO), "-lstatmc_hip", "-L", rocm_lib,
                           "-Wl,-rpath," + os.path.dirname(build.SO), "-Wl,-rpath," + rocm_lib])
    # (no device is visible to the sanitized program, on a GPU box too: tests/test_host_cpu.py)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:protect_shadow_gap=0", ROCR_VISIBLE_DEVICES="-1", HIP_VISIBLE_DEVICES="-1")
    return exe, env


def finite_halves():
    h = np.arange(65536, dtype=np.uint32).astype(np.uint16).view(np.float16)
    return h[np.isfinite(h)]


def converter_inputs():
    """fp32 values as bit patterns: what the issue lists."""
    f32 = np.float32
    halves = finite_halves().astype(f32)
    assert halves.size == 63488
    pos = np.sort(halves[halves >= 0])[1:]                       # +0 (once) .. 65504, ascending
    pos = np.concatenate([[f32(0)], pos, [f32(65536)]])          # ... and the half that would follow 65504
    mid = ((pos[:-1].astype(np.float64) + pos[1:].astype(np.float64)) / 2).astype(f32)
    assert np.array_equal(mid.astype(np.float64), (pos[:-1].astype(np.float64) + pos[1:].astype(np.float64)) / 2)   # exact in fp32
    assert mid[-1] == f32(65520)
    near = np.concatenate([mid, np.nextafter(mid, f32(np.inf)), np.nextafter(mid, f32(-np.inf))])
    special = np.array([65504, np.nextafter(f32(65520), f32(0)), 65520, np.nextafter(f32(65520), f32(np.inf)), 65536, 1e5, 1e30,
                        np.finfo(f32).max, 2.0 ** -14, np.nextafter(f32(2.0 ** -14), f32(0)), np.nextafter(f32(2.0 ** -14), f32(1)),
                        2.0 ** -24, 2.0 ** -25, np.nextafter(f32(2.0 ** -25), f32(1)), np.nextafter(f32(2.0 ** -25), f32(0)),
                        2.0 ** -26, 1e-40, np.finfo(f32).tiny, 0.0, np.inf, 2049, 2051, 1.0, 1.0 / 3], f32)
    values = np.concatenate([halves, near, -near, special, -special, np.array([np.nan], f32)])
    rng = np.random.default_rng(20240)
    return np.concatenate([values.view(np.uint32), np.array([0x7fc00001, 0xffc00000, 0x7f800001, 0xff812345], np.uint32),
                           rng.integers(0, 2 ** 32, 1_000_000, dtype=np.uint64).astype(np.uint32)])


def test_numpy_rounds_to_nearest_even():
    """The yardstick itself, on the cases where the rounding modes differ."""
    with np.errstate(over="ignore"):
        to_half = lambda v: float(np.float32(v).astype(np.float16))
        assert to_half(2049) == 2048 and to_half(2051) == 2052
        assert to_half(2.0 ** -25) == 0 and to_half(np.nextafter(np.float32(2.0 ** -25), np.float32(1))) == 2.0 ** -24
        assert to_half(65520) == np.inf and to_half(np.nextafter(np.float32(65520), np.float32(0))) == 65504


def test_converter_matches_numpy_bit_for_bit(program, tmp_path):
    exe, env = program
    bits = converter_inputs()
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    bits.tofile(fin)
    out = subprocess.run([exe, "convert", fin, fout], capture_output=True, text=True, env=env)
    assert out.returncode == 0, out.stdout + out.stderr
    got = np.fromfile(fout, np.uint16)
    assert got.size == bits.size
    with np.errstate(over="ignore", invalid="ignore"):
        want = bits.view(np.float32).astype(np.float16).view(np.uint16)
    nan = np.isnan(bits.view(np.float32))
    assert nan.sum() > 1000
    assert np.isnan(got[nan].view(np.float16)).all()             # NaN stays NaN; its payload is not promised
    bad = np.nonzero((got != want) & ~nan)[0]
    assert bad.size == 0, [(hex(bits[i]), hex(got[i]), hex(want[i])) for i in bad[:10]]
    # every finite half widened comes back as itself
    halves = finite_halves()
    assert np.array_equal(got[:halves.size], halves.view(np.uint16))


def test_estimator_stages_half(program):
    """SetSampleFormat before / after EnableDeviceAccumulation, capacity and stagedBytes() at 36 -> 24 bytes per pixel-sample of the
    9-channel set, and the staged words of merged tiles equal to the converter's output in block order."""
    exe, env = program
    out = subprocess.run([exe, "staging"], capture_output=True, text=True, env=env)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "tile half staging ok" in out.stdout


@pytest.fixture(scope="module")
def lib():
    from statmc_amd import api
    return api.load()


def stat_types(api, n, samples=0x1000):
    """Descriptors that pass every host-side check (no call below gets as far as reading through them)."""
    types = (api.StatType * max(n, 1))()
    for t in types:
        t.channels, t.transform, t.max_moment, t.n_samples = 3, 0, 1, 0
        t.samples, t.n, t.mean = samples, 0x2000, 0x3000
    return types


def formats(*f):
    return (C.c_int32 * max(len(f), 1))(*f)


def test_entry_is_exported_declared_and_bound(lib):
    import inspect
    from statmc_amd import api
    assert hasattr(lib, "statmc_accumulate_tiles_formats")
    assert "statmc_accumulate_tiles_formats" in api.EXPORTS
    header = open(os.path.join(ROOT, "include", "statmc.h")).read()
    decl = re.search(r"int\s+statmc_accumulate_tiles_formats\s*\(([^;]*)\)\s*;", header)
    assert decl, "include/statmc.h does not declare statmc_accumulate_tiles_formats"
    assert " ".join(decl.group(1).split()) == ("uint16_t width, uint16_t height, const statmc_stat_type *types, const int32_t *sample_formats, "
                                               "int n_types, const int32_t *tile_bounds, const int64_t *tile_offsets, "
                                               "const int32_t *tile_samples, int n_tiles, void *stream")
    assert len(lib.statmc_accumulate_tiles_formats.argtypes) == 10
    assert "sample_formats" in inspect.signature(api.accumulate_tiles).parameters
    hpp = open(os.path.join(ROOT, "include", "statmc_denoiser.hpp")).read()
    assert "uint16_t floatToHalfBits(float" in hpp and "void SetSampleFormat(" in hpp and "size_t stagedBytes()" in hpp


@pytest.mark.parametrize("bad", [2, -1])
def test_unknown_formats_are_refused_before_any_device_work(lib, bad):
    from statmc_amd import api
    types = stat_types(api, 2)
    for fmts in (formats(bad, 0), formats(1, bad)):
        assert lib.statmc_accumulate_tiles_formats(8, 8, types, fmts, 2, 0x4000, 0x5000, 0x6000, 1, None) == api.ERR_INVALID
        assert b"sample_formats" in lib.statmc_last_error()


def test_limits_and_odd_arenas_are_refused_before_any_device_work(lib):
    from statmc_amd import api
    types = stat_types(api, 17)
    assert lib.statmc_accumulate_tiles_formats(8, 8, types, formats(*([1] * 17)), 17, 0x4000, 0x5000, 0x6000, 1, None) == api.ERR_INVALID
    assert b"n_types" in lib.statmc_last_error()
    types = stat_types(api, 2, samples=0x1001)
    assert lib.statmc_accumulate_tiles_formats(8, 8, types, formats(0, 1), 2, 0x4000, 0x5000, 0x6000, 1, None) == api.ERR_INVALID
    assert b"odd address" in lib.statmc_last_error()


def test_refuses_to_run_before_setup(lib):
    """(Checked where no device can have been set up: tests/test_accumulate_half_cpu.py.)"""
    import torch
    from statmc_amd import api
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    types = stat_types(api, 2)
    for fmts in (formats(1, 1), formats(0, 1), formats(0, 0), None):
        assert lib.statmc_accumulate_tiles_formats(8, 8, types, fmts, 2, 0x4000, 0x5000, 0x6000, 1, None) == api.ERR_NO_DEVICE
