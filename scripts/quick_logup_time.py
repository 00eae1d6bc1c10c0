"""Timings around the standalone GKR-logup (development aid).

  ab X_LOG D_LOG NBITS --other-lib PATH [--rounds R] [--runs N]
      gm_pushforward_prove with this tree's library and with another build (e.g. the parent commit's), alternately, each run in a
      fresh child process: whole-call time (no stage timer) and the `logup witness` / `logup prove` stages (GM_PROVE_TIMING=1).
      Prints one JSON line with the medians and the other build's min-to-max spread.  Extra environment for this tree's children
      (GM_LOGUP_NO_TAIL=1, GM_LOGUP_TAIL_LOG=8..11) is taken from --env K=V.
  standalone L0 L1 L2 ...   gm_logup_witness_create + gm_logup_prove on random columns of those logsizes
  helpers                   gm_logup_denominators and gm_logup_multiplicities: time and achieved bytes per second
"""
import argparse
import ctypes as C
import json
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def child_pushforward(x_log, d_log, nbits, runs):
    import numpy as np
    import torch
    from gkr_msm_amd import codec, ffi, harness as H
    raw = C.CDLL(ffi.LIB_PATH)   # the other build may be older than this tree's symbol table: bind what it has
    for name in [s for s in ffi._SIGS if not hasattr(raw, s)]:
        del ffi._SIGS[name]
    L = ffi.lib()
    n = 1 << x_log
    y_size = (nbits + d_log - 1) // d_log
    y_log = (y_size - 1).bit_length()
    d_pts = H.dev_empty(n * 8)
    ffi.check(L.gm_gen_points(C.c_void_p(d_pts.data_ptr()), n, 0x474b524d534d, H.cur_stream()))
    rng = np.random.default_rng(1)
    sc = rng.integers(0, 2**64, size=(n, 4), dtype=np.uint64)
    if nbits < 256:
        for limb in range(4):
            keep = min(max(nbits - 64 * limb, 0), 64)
            sc[:, limb] &= np.uint64((1 << keep) - 1)
    else:
        sc[:, 3] &= np.uint64((1 << 60) - 1)
    plan = H.MsmPlan(x_log, d_log, y_size)
    plan.run(d_pts, H.to_dev(sc))
    P = codec.P
    r = [int.from_bytes(rng.bytes(64), "little") % P for _ in range(y_log + d_log + x_log)]
    evs = [int.from_bytes(rng.bytes(64), "little") % P for _ in range(3)]
    tape = [int.from_bytes(rng.bytes(64), "little") % P for _ in range(4)] + [int.from_bytes(rng.bytes(16), "little") for _ in range(1500)]
    for it in range(2 + runs):   # two warm-ups
        torch.cuda.synchronize()
        t = time.perf_counter()
        H.pushforward_prove(plan, d_pts, y_log, r, evs, tape)
        ms = (time.perf_counter() - t) * 1e3
        print("[run] %s %.3f" % ("warm" if it < 2 else "timed", ms), file=sys.stderr, flush=True)


def parse_child(err, runs):
    whole = [float(m.group(1)) for m in re.finditer(r"^\[run\] timed ([0-9.]+)", err, re.M)]
    stages = {}
    for name in ("logup witness", "logup prove"):
        v = [float(m.group(1)) for m in re.finditer(r"^\[gm pushforward\] %s\s+([0-9.]+) ms" % name, err, re.M)]
        stages[name] = v[-runs:] if v else []
    return whole, stages


def ab(args):
    mine = os.path.join(ROOT, "gkr_msm_amd", "libgkrmsm_hip.so")
    extra = dict(kv.split("=", 1) for kv in args.env)
    res = {k: dict(whole=[], witness=[], prove=[]) for k in ("other", "this")}
    for rd in range(args.rounds):
        for timing in ("0", "1"):
            for who, lib in (("other", args.other_lib), ("this", mine)):
                env = dict(os.environ, GM_LIB_PATH=lib, GM_PROVE_TIMING=timing)
                if who == "this":
                    env.update(extra)
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "child", str(args.x_log), str(args.d_log), str(args.nbits),
                                    "--runs", str(args.runs)], env=env, capture_output=True, text=True, timeout=300)
                if p.returncode != 0:   # nothing more is started after a failure
                    print(p.stderr[-3000:], file=sys.stderr)
                    sys.exit("child (%s, timing %s) ended with %d" % (who, timing, p.returncode))
                whole, st = parse_child(p.stderr, args.runs)
                if timing == "0":
                    res[who]["whole"] += whole
                else:
                    res[who]["witness"] += st["logup witness"]
                    res[who]["prove"] += st["logup prove"]
    out = dict(shape=[args.x_log, args.d_log, args.nbits], env=extra)
    for who in res:
        for k, v in res[who].items():
            out["%s_%s_median_ms" % (who, k)] = round(statistics.median(v), 3)
            out["%s_%s_spread_ms" % (who, k)] = round(max(v) - min(v), 3)
            out["%s_%s_n" % (who, k)] = len(v)
    print(json.dumps(out))


def rand_cols(torch, n):
    """n field elements: 254 random bits each (below the modulus), read as Montgomery form"""
    t = torch.randint(-2**63, 2**63 - 1, (n, 4), dtype=torch.int64, device="cuda")
    t[:, 3] &= (1 << 62) - 1
    return t.reshape(-1)


def standalone(logsizes):
    import torch
    from gkr_msm_amd import codec, harness as H
    P = codec.P
    torch.manual_seed(3)
    nums = [rand_cols(torch, 1 << lg) for lg in logsizes]
    dens = [rand_cols(torch, 1 << lg) for lg in logsizes]
    tape = [int.from_bytes(os.urandom(16), "little") for _ in range(1500)]
    for it in range(4):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        w = H.LogupWitness(logsizes, nums, dens)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        n, d = w.total()
        claim = n * pow(d, P - 2, P) % P
        t2 = time.perf_counter()
        g = w.prove(claim, tape)
        t3 = time.perf_counter()
        w.close()
        print(json.dumps(dict(logsizes=logsizes, run=it, create_ms=round((t1 - t0) * 1e3, 3), prove_ms=round((t3 - t2) * 1e3, 3),
                              rounds=g["rounds"])), flush=True)


def helpers():
    import torch
    from gkr_msm_amd import harness as H
    torch.manual_seed(4)

    def timed(fn, reps=5):
        fn()
        v = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            v.append((time.perf_counter() - t) * 1e3)
        return statistics.median(v)
    ln, k = 1 << 24, 2
    cols = [rand_cols(torch, ln) for _ in range(k)]
    for ones in (False, True):
        ms = timed(lambda: H.logup_denominators(cols, 12345, 67890, ones=ones))
        b = 32 * (k + 1) * ln + (32 * ln if ones else 0)
        print(json.dumps(dict(kernel="k_logup_den", k=k, len=ln, ones=ones, ms=round(ms, 3), GBps=round(b / ms / 1e6, 1),
                              note="includes the allocation of the outputs")), flush=True)
    n = 1 << 24
    for tl_log in (8, 14, 20):
        idx = torch.randint(0, 1 << tl_log, (n,), dtype=torch.int32, device="cuda")
        ms = timed(lambda: H.logup_multiplicities(idx, n, 1 << tl_log))
        b = 4 * n + 32 * (1 << tl_log)
        print(json.dumps(dict(kernel="k_logup_hist", n=n, table_log=tl_log, ms=round(ms, 3), GBps=round(b / ms / 1e6, 1),
                              note="whole call: counters, conversion, flag copy")), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="mode", required=True)
    for name in ("ab", "child"):
        a = sub.add_parser(name)
        a.add_argument("x_log", type=int)
        a.add_argument("d_log", type=int)
        a.add_argument("nbits", type=int)
        a.add_argument("--runs", type=int, default=3)
        if name == "ab":
            a.add_argument("--other-lib", required=True)
            a.add_argument("--rounds", type=int, default=2)
            a.add_argument("--env", action="append", default=[])
    s = sub.add_parser("standalone")
    s.add_argument("logsizes", type=int, nargs="+")
    sub.add_parser("helpers")
    args = ap.parse_args()
    if args.mode == "child":
        child_pushforward(args.x_log, args.d_log, args.nbits, args.runs)
    elif args.mode == "ab":
        ab(args)
    elif args.mode == "standalone":
        standalone(args.logsizes)
    else:
        helpers()
