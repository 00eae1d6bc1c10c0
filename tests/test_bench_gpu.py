"""A plain `bench.py` run (no --full) on the GPU: it prints the headline line and nothing of the legs --full adds, and what
--dump-outputs writes is the MSM of the bench's seeded inputs, bit-exact against the C oracle."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_ffi as O
from gkr_msm_amd import codec, ffi, harness

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

pytestmark = pytest.mark.gpu

FULL_ONLY = ("roofline", "roofline_levels_ge1", "stage_ms", "whole_msm", "sumcheck", "gen1", "g1", "full_gen2_prover", "cpu_baseline",
             "parity", "n1_same_run", "weak", "config_d")


def _words_to_ints(a):
    w = a.astype(np.uint64)
    return [sum(int(v) << (32 * i) for i, v in enumerate(row)) for row in w.reshape(-1, 8)]


def test_plain_run_prints_the_headline_and_dumps_the_msm(tmp_path):
    x_log, d_log, nbits = 12, 8, 256
    d = str(tmp_path / "dump")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--x-logsize", str(x_log), "--dump-outputs", d], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["metric"] == "msm_points_per_sec" and out["unit"] == "points/s" and out["higher_is_better"] is True
    assert out["steps"] == 3 and out["warmup"] == 1 and out["n_gpus"] == 1 and out["dtype"]
    assert out["value"] > 0 and out["ms_per_step"] > 0
    assert out["config"]["x_logsize"] == x_log
    assert [k for k in FULL_ONLY if k in out] == []

    # the same seeded inputs, made here, through the C oracle
    n, y_size = 1 << x_log, (nbits + d_log - 1) // d_log
    L = ffi.lib()
    d_pts = harness.dev_empty(n * 8)
    ffi.check(L.gm_gen_points(C.c_void_p(d_pts.data_ptr()), n, bench.SEED, harness.cur_stream()))
    pts = harness.to_host(d_pts).reshape(n, 8)
    ref = O.msm(pts, bench.make_scalars(n, nbits), x_log, d_log, y_size, threads=4, want_aux=False)
    wp = np.load(os.path.join(d, "window_points.npy"))
    assert wp.shape == (3 * (d_log + 1), y_size, 8)
    words = wp.astype(np.uint64).reshape(3 * (d_log + 1), y_size, 4, 2)
    assert np.array_equal(words[..., 0] | (words[..., 1] << np.uint64(32)), ref["window_cols"])
    exp = tuple(codec.from_mont_limbs(O.msm_combine(ref["window_cols"], d_log)))
    assert tuple(_words_to_ints(np.load(os.path.join(d, "msm_result.npy")))) == exp
    assert out["result_x"] == hex(exp[0])
