"""bench.py without a GPU: the --dump-outputs writer and the argument checks that come before any device call."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_outputs_that_fit_are_written_whole(tmp_path):
    import bench
    rng = np.random.default_rng(3)
    film = rng.standard_normal((6, 10, 3)).astype(np.float32)
    info = bench.write_outputs(str(tmp_path / "out"), {"film_f": film})
    got = np.load(tmp_path / "out" / "film_f.npy")
    assert got.dtype == np.float32 and np.array_equal(got, film)
    assert info["arrays"]["film_f"] == {"shape": [6, 10, 3], "dtype": "float32"}


def test_outputs_over_the_limit_are_a_fixed_sample_of_pixels(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 4096 + 64 * 12)      # room for 64 of the 200 RGB float32 pixels
    film = np.arange(20 * 10 * 3, dtype=np.float32).reshape(20, 10, 3)
    runs = []
    for k in range(2):
        d = tmp_path / str(k)
        info = bench.write_outputs(str(d), {"film_f": film})
        runs.append(np.load(d / "film_f.npy"))
        assert os.path.getsize(d / "film_f.npy") <= bench.DUMP_LIMIT_BYTES
    a = info["arrays"]["film_f"]
    assert a["shape"] == [20, 10, 3] and a["sampled_pixels"] == 64 and a["stored_shape"] == [64, 3]
    assert np.array_equal(runs[0], runs[1])                             # the same pixels on every run
    px = runs[0][:, 0] / 3                                              # pixel indices, ascending, each a whole RGB triple
    assert np.all(np.diff(px) > 0) and np.array_equal(runs[0], film.reshape(-1, 3)[px.astype(int)])


def test_steps_must_be_positive():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 2 and "--steps must be at least 1" in out.stderr


def test_full_is_off_by_default(monkeypatch):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "5", "--warmup", "2"])
    args = bench.parse()
    assert args.full is False and (args.steps, args.warmup) == (5, 2)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--no-cpu-baseline"])
    args = bench.parse()
    assert args.full is True and args.no_cpu_baseline
