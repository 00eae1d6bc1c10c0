"""bench.py --dump-outputs: the .npy files hold what the last timed MSM step returned, bit for bit (every 256-bit value as eight
32-bit words in float64); --steps below 1 is refused before anything touches a GPU."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_dump_outputs_hold_the_step_results_exactly(tmp_path):
    raw = np.random.default_rng(1).integers(0, 2 ** 64, size=(27, 32, 4), dtype=np.uint64)
    raw[0, 0] = np.iinfo(np.uint64).max
    result = (bench.P - 1, 0x0123456789ABCDEF << 190)
    d = str(tmp_path / "dump")
    bench.dump_outputs(d, result, raw)
    assert sorted(os.listdir(d)) == ["msm_result.npy", "window_points.npy"]
    xy, wp = np.load(os.path.join(d, "msm_result.npy")), np.load(os.path.join(d, "window_points.npy"))
    assert xy.dtype == np.float64 and wp.dtype == np.float64
    assert xy.shape == (2, 8) and wp.shape == (27, 32, 8)
    assert [sum(int(w) << (32 * i) for i, w in enumerate(row)) for row in xy] == list(result)
    words = wp.astype(np.uint64).reshape(27, 32, 4, 2)
    assert np.array_equal(words[..., 0] | (words[..., 1] << np.uint64(32)), raw)


def test_steps_below_one_are_refused():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "--steps must be at least 1" in r.stderr


def test_full_is_an_option_of_its_own():
    # --full is parsed like any other option (an unknown one would fail with argparse's own message before the --steps check)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--steps", "0"], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 2 and "--steps must be at least 1" in r.stderr
