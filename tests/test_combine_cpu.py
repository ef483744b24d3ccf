"""No-GPU checks of statmc_combine_statistics (include/statmc.h): exported, laid out as the ctypes mirror says, refused
without a device, the offline tool's --combine argument errors, and the float64 restatement the GPU tests
(tests/test_combine_gpu.py) compare against."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from statmc_amd import api, build
    build.build()
    return api.load()


# ---------------------------------------------------------------- float64 restatement of the combine (include/statmc.h)
def combine64(nA, A, nB, B, max_moment):
    """A, B: dicts of float64 arrays mean / m2 / m3 ([H, W, C]); nA, nB: [H, W] counts.  Returns (n, dict) of the
    union's moments by the pairwise formulas, with nB == 0 -> A and nA == 0 -> B."""
    nA = np.asarray(nA, np.float64)[..., None]
    nB = np.asarray(nB, np.float64)[..., None]
    n = nA + nB
    with np.errstate(divide="ignore", invalid="ignore"):
        d = B["mean"] - A["mean"]
        out = {"mean": A["mean"] + d * nB / n}
        if max_moment >= 2:
            out["m2"] = A["m2"] + B["m2"] + d * d * nA * nB / n
        if max_moment >= 3:
            out["m3"] = (A["m3"] + B["m3"] + d ** 3 * nA * nB * (nA - nB) / (n * n)
                         + 3.0 * d * (nA * B["m2"] - nB * A["m2"]) / n)
    for k in out:
        out[k] = np.where(nB == 0, A[k], np.where(nA == 0, B[k], out[k]))
    return (nA + nB)[..., 0].astype(np.int64), out


def two_pass64(x):
    """x: [S, ...] samples -> (mean, m2, m3) about the mean, float64, two passes."""
    x = np.asarray(x, np.float64)
    mu = x.mean(axis=0)
    dev = x - mu
    return mu, (dev ** 2).sum(axis=0), (dev ** 3).sum(axis=0)


def test_float64_reference_restates_the_union():
    """The restatement itself: the moments of two halves, combined, are the two-pass moments of the union (to 1e-12) --
    uneven splits, empty halves and constant samples included."""
    rng = np.random.default_rng(3)
    S, H, W, Ch = 40, 3, 5, 3
    x = np.exp(rng.normal(0.0, 1.0, (S, H, W, Ch)))
    x[:, 2, 0] = 0.75                                    # constant samples
    split = rng.integers(0, S + 1, size=(H, W))
    split[0, 0], split[0, 1] = 0, S                      # one side empty
    nA = split.astype(np.int64)
    nB = S - nA
    A = {k: np.zeros((H, W, Ch)) for k in ("mean", "m2", "m3")}
    B = {k: np.zeros((H, W, Ch)) for k in ("mean", "m2", "m3")}
    for y in range(H):
        for xx in range(W):
            k = split[y, xx]
            if k:
                A["mean"][y, xx], A["m2"][y, xx], A["m3"][y, xx] = two_pass64(x[:k, y, xx])
            if k < S:
                B["mean"][y, xx], B["m2"][y, xx], B["m3"][y, xx] = two_pass64(x[k:, y, xx])
    n, got = combine64(nA, A, nB, B, 3)
    want = two_pass64(x)
    assert np.array_equal(n, np.full((H, W), S))
    for k, w in zip(("mean", "m2", "m3"), want):
        scale = max(np.abs(w).max(), 1.0)
        assert np.abs(got[k] - w).max() <= 1e-12 * scale, k
    assert np.all(got["m2"][2, 0] == 0.0) and np.all(got["m3"][2, 0] == 0.0)


# ---------------------------------------------------------------- the C ABI
def test_combine_entry_point_is_exported(lib):
    from statmc_amd import api
    assert hasattr(lib, "statmc_combine_statistics")
    assert "statmc_combine_statistics" in api.EXPORTS
    assert lib.statmc_version() == 101


def test_combine_entry_layout_matches_header(lib):
    from statmc_amd import api
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "statmc.h"
int main(void) {
  printf("%zu %zu %zu %zu\n", sizeof(statmc_combine_entry), offsetof(statmc_combine_entry, dst),
         offsetof(statmc_combine_entry, src), offsetof(statmc_combine_entry, count_of));
  return 0;
}'''
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")])
        got = [int(x) for x in subprocess.check_output([os.path.join(d, "t")]).split()]
    ce = api.CombineEntry
    assert got == [C.sizeof(ce), ce.dst.offset, ce.src.offset, ce.count_of.offset]


def test_combine_without_a_device_is_an_error(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from statmc_amd import api
    e = (api.CombineEntry * 1)()
    assert lib.statmc_combine_statistics(8, 8, e, 1, None) == api.ERR_NO_DEVICE
    assert lib.statmc_combine_statistics(8, 8, None, 0, None) == api.ERR_NO_DEVICE
    assert b"setup" in lib.statmc_last_error()


# ---------------------------------------------------------------- the offline tool
@pytest.fixture(scope="module")
def denoise_bin():
    from statmc_amd import build
    return build.build_tools()


def test_denoise_tool_combine_argument_errors(denoise_bin, tmp_path):
    r = subprocess.run([denoise_bin, "--stem", str(tmp_path / "a"), "--spp", "4", "--combine", str(tmp_path / "b")],
                       capture_output=True, text=True)
    assert r.returncode != 0 and "--output-stem" in r.stderr
    r = subprocess.run([denoise_bin, "--combine", "X"], capture_output=True, text=True)
    assert r.returncode != 0 and "--output-stem" in r.stderr
    r = subprocess.run([denoise_bin, "--stem", str(tmp_path / "a"), "--spp", "4", "--combine", str(tmp_path / "b"),
                        "--output-stem", str(tmp_path / "o"), "--grid", "2x1"], capture_output=True, text=True)
    assert r.returncode != 0 and "--grid" in r.stderr
    r = subprocess.run([denoise_bin, "--stem", str(tmp_path / "a"), "--spp", "4", "--combine", str(tmp_path / "b"),
                        "--output-stem", str(tmp_path / "o"), "--sweep", "quick"], capture_output=True, text=True)
    assert r.returncode != 0 and "--sweep" in r.stderr
