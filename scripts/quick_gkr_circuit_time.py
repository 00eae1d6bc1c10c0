"""Caller-defined GKR circuits, development aid (not part of bench.py).  Prints one JSON line per case:
  dense_evaluate   gm_dense_evaluate of 4 columns x 2^EVAL_LOG (the whole call: it returns with the results on the host), median of
                   `reps`, GB/s by algorithmic bytes (32 B per element read once) and the share of 8 TB/s
  bintree          the bintree circuit (bit check, VecVec input of 2^ROW x 2^COL cells, ADDS additions) built and proven three ways:
                   gm_bintree_witness_create + gm_gkr_prove, the same layer list with built-in ids through
                   gm_gkr_circuit_witness_create_vv, and with every function a program; build and prove wall times (median of
                   `reps`, the three alternated), rounds and the prover's time per sumcheck round
Usage: quick_gkr_circuit_time.py [EVAL_LOG=24] [ROW=10] [COL=10] [ADDS=6] [reps=5]"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
from gkr_msm_amd import codec, ffi, harness as H

EVAL_LOG = int(sys.argv[1]) if len(sys.argv) > 1 else 24
ROW = int(sys.argv[2]) if len(sys.argv) > 2 else 10
COL = int(sys.argv[3]) if len(sys.argv) > 3 else 10
ADDS = int(sys.argv[4]) if len(sys.argv) > 4 else 6
reps = int(sys.argv[5]) if len(sys.argv) > 5 else 5
P = codec.P
HBM_PEAK_GBS = 8000.0


def rand_limbs(rs, n):
    a = rs.integers(0, 2**63, size=(n, 4), dtype=np.uint64)
    a[:, 3] &= np.uint64(0x3FFFFFFFFFFFFFFF)
    return a


def median_ms(f):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), ts


def dense_evaluate_case(rs):
    k, n = 4, 1 << EVAL_LOG
    cols = [H.to_dev(rand_limbs(rs, n)) for _ in range(k)]
    pa = H.fr_arg([int(x) for x in rs.integers(1, 2**62, size=EVAL_LOG)])
    evs = np.zeros((k, 4), dtype=np.uint64)
    ptrs = H.ptr_array(cols)

    def run():
        ffi.check(ffi.lib().gm_dense_evaluate(ptrs, k, EVAL_LOG, pa.ctypes.data, evs.ctypes.data, H.cur_stream()))
    run()
    ms, ts = median_ms(run)
    gbs = k * n * 32 / 1e9 / (ms / 1e3)
    print(json.dumps(dict(case="dense_evaluate", cols=k, num_vars=EVAL_LOG, ms=round(ms, 3), runs=[round(t, 3) for t in ts],
                          GBps=round(gbs, 1), hbm_share=round(gbs / HBM_PEAK_GBS, 3))), flush=True)


def bintree_vv(rs):
    """6 full polynomials (x_e, y_e, x_o, y_o random; z_e, z_o Boolean) of 2^ROW x 2^COL cells, zero pads on z"""
    nrows, rl = 1 << COL, 1 << ROW
    cells = nrows * rl
    data = [rand_limbs(rs, cells) for _ in range(4)]
    one = codec.to_mont_limbs([1])[0]
    for _ in range(2):
        bits = rs.integers(0, 2, size=cells).astype(bool)
        z = np.zeros((cells, 4), dtype=np.uint64)
        z[bits] = one
        data.append(z)
    lens = np.full(nrows, rl, dtype=np.uint32)
    dptr = (C.c_void_p * 6)(*[d.ctypes.data for d in data])
    rp = H.fr_arg([5, 7, 11, 13, 0, 0])
    cp = H.fr_arg([17, 19, 23, 29, 0, 0])
    h = C.c_void_p()
    ffi.check(ffi.lib().gm_vv_from_host(6, nrows, lens.ctypes.data, dptr, rp.ctypes.data, cp.ctypes.data, ROW, COL, C.byref(h),
                                        H.cur_stream()))
    return H.VV(h)


def bintree_case(rs):
    from test_gkr_circuit_gpu import bintree_spec   # the layer lists the GPU tests check bit for bit
    vv = bintree_vv(rs)
    spec_b, spec_p = bintree_spec(ADDS, True), bintree_spec(ADDS, True, programs=True)
    makers = dict(builtin_witness=lambda: H.GkrWitness.bintree(vv, ADDS, True),
                  circuit_builtin_ids=lambda: H.GkrCircuit.vecvec(spec_b, vv),
                  circuit_programs=lambda: H.GkrCircuit.vecvec(spec_p, vv))
    w0 = makers["builtin_witness"]()
    out, nv = w0.output()
    rng = np.random.default_rng(3)
    point = [int(x) for x in rng.integers(1, 2**62, size=nv)]
    evs = H.gkr_witness_claims(w0, point)
    tape = [int(x) for x in rng.integers(1, 2**62, size=4 * (ROW + COL) * ADDS + 64)]
    ref = w0.prove(point, evs, tape)
    w0.close()
    build = {k: [] for k in makers}
    prove = {k: [] for k in makers}
    for it in range(reps + 1):   # the first round warms up every shape
        for k, mk in makers.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            w = mk()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            r = w.prove(point, evs, tape)
            t2 = time.perf_counter()
            assert r["msgs"] == ref["msgs"], k
            w.close()
            if it:
                build[k].append((t1 - t0) * 1e3)
                prove[k].append((t2 - t1) * 1e3)
    for k in makers:
        b, p = float(np.median(build[k])), float(np.median(prove[k]))
        print(json.dumps(dict(case="bintree", variant=k, row_logsize=ROW, col_logsize=COL, num_adds=ADDS, rounds=ref["rounds"],
                              build_ms=round(b, 2), prove_ms=round(p, 2), total_ms=round(b + p, 2),
                              us_per_round=round(p * 1e3 / ref["rounds"], 1), prove_runs=[round(t, 2) for t in prove[k]])), flush=True)


def main():
    torch.cuda.set_device(0)
    rs = np.random.default_rng(1)
    dense_evaluate_case(rs)
    bintree_case(rs)


if __name__ == "__main__":
    main()
