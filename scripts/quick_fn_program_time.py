"""Built-in layer functions against their program twins (gm_fn_program_create), development aid.  For PROJ_L1 and PROJ_L2:
gm_dense_map at 2^24 rows, and every round of a dense deg-2 sumcheck object at 2^22 elements (kernel, fold and host time per
round as the prover sees it).  Prints one JSON line per case: built-in ms, program ms and their ratio (median of `reps`)."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gkr_msm_amd import codec, ffi, harness as H

MAP_LOG = int(sys.argv[1]) if len(sys.argv) > 1 else 24
SC_LOG = int(sys.argv[2]) if len(sys.argv) > 2 else 22
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
P = codec.P
A5 = 5          # y1 y2 - a x1 x2 with a = -5
TERMS = {
    "PROJ_L1": (4, 6, 4, [(1, 0, (0, 4)), (1, 1, (3, 1)), (1, 2, (1, 4)), (A5, 2, (0, 3)), (1, 3, (2, 5))]),
    "PROJ_L2": (5, 4, 4, [(1, 0, (0, 3)), (1, 0, (1, 3)), (1, 1, (2, 3)), (1, 2, (3, 3)), (1, 3, (0, 1))]),
}


def rand_cols(rs, k, n):
    out = []
    for _ in range(k):
        a = rs.integers(0, 2**63, size=(n, 4), dtype=np.uint64)
        a[:, 3] &= np.uint64(0x3FFFFFFFFFFFFFFF)
        out.append(H.to_dev(a))
    return out


def timed(f):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def main():
    torch.cuda.set_device(0)
    rs = np.random.default_rng(1)
    for name, (bid, ni, no, terms) in TERMS.items():
        pid = H.make_program(ni, no, 2, terms)
        fb, fp = ffi.make_fn((bid, 1)), ffi.make_fn((pid, 1))
        cols = rand_cols(rs, ni, 1 << MAP_LOG)
        outs = [H.dev_empty((1 << MAP_LOG) * 4) for _ in range(no)]

        def run_map(fn):
            ffi.check(ffi.lib().gm_dense_map(H.C.byref(fn), H.ptr_array(cols), H.ptr_array(outs), 1 << MAP_LOG, H.cur_stream()))
        run_map(fb)
        run_map(fp)
        tb, tp = timed(lambda: run_map(fb)), timed(lambda: run_map(fp))
        hbm = (ni + no) * 32.0 * (1 << MAP_LOG) / 1e9
        print(json.dumps(dict(case="dense_map", fn=name, rows_log=MAP_LOG, builtin_ms=round(tb, 3), program_ms=round(tp, 3),
                              ratio=round(tp / tb, 2), builtin_GBps=round(hbm / tb * 1e3, 1), program_GBps=round(hbm / tp * 1e3, 1))))
        del cols, outs
        cols = rand_cols(rs, ni, 1 << SC_LOG)
        rng = np.random.default_rng(2)
        point = [int(x) % P for x in rng.integers(1, 2**62, size=SC_LOG)]
        chal = [int(x) for x in rng.integers(1, 2**62, size=SC_LOG)]
        claims = [int(x) for x in rng.integers(1, 2**62, size=no)]

        def run_sc(fn):
            so = H.Sumcheckable.dense_deg2(fn, SC_LOG, cols, point, 12345, claims)
            for t in chal:
                so.unipoly()
                so.bind(t)
            so.final_evals()
            so.close()
        run_sc(fb)
        run_sc(fp)
        tb, tp = timed(lambda: run_sc(fb)), timed(lambda: run_sc(fp))
        print(json.dumps(dict(case="dense_deg2_object", fn=name, num_vars=SC_LOG, rounds=SC_LOG, builtin_ms=round(tb, 3),
                              program_ms=round(tp, 3), ratio=round(tp / tb, 2))))
        del cols
        H.destroy_program(pid)


if __name__ == "__main__":
    main()
