"""BASELINE.json's named configurations at their FULL sizes on one GPU, bit for bit against the C oracle (oracle/gkrmsm_oracle*.c,
OpenMP on the host cores):

  configs[1]  x_logsize=20, d_logsize=8, nbits=256 Pippenger MSM     -> digits, counter, row lengths, bucket sums, window
                                                                        points, final point AND every message of the image-part
                                                                        prover (1518 sumcheck rounds)
  configs[0]  x_logsize=16, d_logsize=8, nbits=128 (examples/pippenger.rs defaults of README.md:5)
                                                                     -> the same, plus the whole gen-2 proof through the
                                                                        library's verifier and the pairing check
  configs[2]  gen-1 gkr_msm_prove at the largest size of the reference's own bench grid (benches/gkr_msm_simple.rs:97-107:
              log_num_points 13..17 exclusive, 256-bit scalars) -> every transcript message

  configs[3]  x_logsize=24, nbits=256 MSM sharded by windows over 8 GPUs -> ONE rank's share at full size on one GPU (4 of the
              32 windows over all 2^24 points: ranks 0 and 5), bit-exact against the oracle run on the same digits
  configs[4]  x_logsize=24 prover sharded 8 ways -> DRY RUN of one rank's share at full size (memory and time of every kernel at
              that shape; the other ranks' partial sums are absent, so the transcript is not a real proof's)
  configs[1] sharded: the image-part prover of config B with its bucket rows split over 4 ranks (4 processes sharing the one GPU,
              gloo): every message equal to the unsharded proof, which the first test pins to the oracle

  configs[2]  gen-1 gkr_msm_prove at 2^20 points x 2^8 bits and the WHOLE gen-2 proof at x_logsize=20 (the oracle stops at 2^16:
              checked through the library verifier, the final claims against the committed columns, the pairing, tampering)

Nothing here shrinks silently: a host without the memory the oracle leg needs FAILS the test (the GPU boxes have terabytes), and
every test records the size it ran (conftest.record_at_size -> the session summary and gpurun_out/at_size_runs.json)."""
import ctypes as C
import os
import sys
import time

import numpy as np
import pytest
import torch

import oracle_ffi as O
from gkr_msm_amd import codec, ffi, harness as H

pytestmark = pytest.mark.gpu
P = codec.P


def host_threads():
    return max(1, min(os.cpu_count() or 1, 32))


def require_host_gib(need, what):
    """the named size or a failure -- never a smaller size"""
    import psutil   # a missing psutil is a failure too (it used to read as 0 GiB and shrink every test)
    have = psutil.virtual_memory().available / 2 ** 30
    if have < need:
        pytest.fail("%s needs %d GiB of host memory for the oracle leg, %.0f GiB available: not run at a smaller size" % (what, need, have))
    return have


def record(test, **fields):
    from conftest import record_at_size
    return record_at_size(test, **fields)


def device_inputs(x_log, nbits, seed):
    """points: gm_gen_points (k_i * G from SplitMix64 `seed`); scalars: uniform nbits-bit canonical bigints"""
    n = 1 << x_log
    d_pts = H.dev_empty(n * 8)
    ffi.check(ffi.lib().gm_gen_points(C.c_void_p(d_pts.data_ptr()), n, seed, H.cur_stream()))
    sc = np.random.default_rng(seed).integers(0, 2 ** 64, size=(n, 4), dtype=np.uint64)
    sc[:, 3] &= np.uint64((1 << 60) - 1)           # < 2^252 < the Bandersnatch group order
    for limb in range(4):
        lo = max(0, min(64, nbits - 64 * limb))
        if lo < 64:
            sc[:, limb] &= np.uint64((1 << lo) - 1)
    sc[1] = 0                                      # a zero scalar: bucket 0 of every window
    sc[3] = sc[2]                                  # a collision
    return d_pts, H.to_dev(sc), sc


def check_msm(x_log, d_log, nbits, seed, scalars=None):
    y_size = (nbits + d_log - 1) // d_log
    d_pts, d_sc, sc = device_inputs(x_log, nbits, seed)
    if scalars is not None:
        sc = np.ascontiguousarray(scalars, dtype=np.uint64)
        d_sc = H.to_dev(sc)
    pts_host = H.to_host(d_pts).reshape(-1, 8)
    plan = H.MsmPlan(x_log, d_log, y_size)
    plan.run(d_pts, d_sc)
    t0 = time.perf_counter()
    ref = O.msm(pts_host, sc, x_log, d_log, y_size, threads=host_threads(), want_aux=True)
    cpu_s = time.perf_counter() - t0
    dg, ct, rl = plan.digits_counter_rowlen()
    assert np.array_equal(dg, ref["digits"]), "digits"
    assert np.array_equal(ct, ref["counter"]), "counter"
    assert np.array_equal(rl, ref["row_len"]), "bucket populations"
    px, py, pz, nb = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_uint64()
    ffi.check(plan.L.gm_msm_bucket_sums(plan.h, C.byref(px), C.byref(py), C.byref(pz), C.byref(nb)))
    assert nb.value == y_size << d_log
    for p, k in ((px, "bx"), (py, "by"), (pz, "bz")):
        assert np.array_equal(H.read_dev(p, nb.value * 32).reshape(-1, 4), ref[k]), "bucket sums " + k
    raw = plan.window_points_raw()
    assert np.array_equal(raw, ref["window_cols"]), "window points"
    got = H.combine_host(raw, d_log)
    assert got == tuple(codec.from_mont_limbs(O.msm_combine(ref["window_cols"], d_log))), "final point"
    print("[at-size] MSM x=%d d=%d nbits=%d bit-exact vs the C oracle (%d threads, %.2f s on the CPU)" % (
        x_log, d_log, nbits, host_threads(), cpu_s))
    return plan, d_pts, d_sc, pts_host, sc


def check_image_part(plan, d_pts, pts_host, sc, x_log, d_log, nbits, seed):
    y_size = (nbits + d_log - 1) // d_log
    y_log = (y_size - 1).bit_length()
    w = H.PipWitness(plan, d_pts, y_log)
    outs, _ = w.outputs()
    pr = np.random.default_rng(seed)
    r_pt = [int.from_bytes(pr.bytes(64), "little") % P for _ in range(y_log)]

    def ev(poly):
        cur = list(poly)
        for f in reversed(r_pt):
            cur = [(cur[2 * i] + f * (cur[2 * i + 1] - cur[2 * i])) % P for i in range(len(cur) // 2)]
        return cur[0]
    r_evs = [ev(o) for o in outs]
    tape = [int.from_bytes(pr.bytes(16), "little") for _ in range(4000)]
    g = w.prove_image_part(r_pt, r_evs, tape)
    w.close()
    H.ffi.lib().gm_release_cached_memory()
    t0 = time.perf_counter()
    cw = O.PipWitness(pts_host, sc, x_log, d_log, y_size, y_log, host_threads())
    assert np.array_equal(np.array([codec.to_mont_limbs(o) for o in outs]).reshape(len(outs), -1, 4), cw.output()), "dense output"
    c = cw.prove_image_part(codec.to_mont_limbs(r_pt), codec.to_mont_limbs(r_evs), codec.ints_to_limbs(tape))
    cpu_s = time.perf_counter() - t0
    cw.close()
    assert g["tape_used"] == c["tape_used"] and g["rounds"] == c["rounds"]
    assert codec.from_mont_limbs(c["msgs"]) == g["msgs"], "prover messages"
    assert codec.from_mont_limbs(c["point"]) == g["point"] and codec.from_mont_limbs(c["evs"]) == g["evs"], "final claims"
    print("[at-size] image-part prover x=%d d=%d nbits=%d: %d rounds, %d messages bit-exact vs the C oracle (%.1f s on the CPU)" % (
        x_log, d_log, nbits, g["rounds"], len(g["msgs"]), cpu_s))
    return g


def test_config_b_msm_and_image_part_at_full_size():
    """BASELINE.json configs[1] (pippenger.rs:462-559 at x_logsize=20, d_logsize=8, nbits=256)"""
    x_log, d_log, nbits = 20, 8, 256
    require_host_gib(40, "config B's prover leg (x_logsize 20)")
    t0 = time.perf_counter()
    plan, d_pts, d_sc, pts_host, sc = check_msm(x_log, d_log, nbits, 0x474B524D534D)
    g = check_image_part(plan, d_pts, pts_host, sc, x_log, d_log, nbits, 7)
    assert g["rounds"] == 1518
    record("config_b_msm_and_image_part", x_logsize=x_log, d_logsize=d_log, nbits=nbits, rounds=g["rounds"], messages=len(g["msgs"]),
           seconds=round(time.perf_counter() - t0, 1), checked="every MSM stage + every prover message vs the C oracle")
    plan.close()
    ffi.lib().gm_release_cached_memory()
    torch.cuda.empty_cache()


def test_config_a_msm_image_part_and_whole_proof():
    """BASELINE.json configs[0]: --x-logsize 16 --d-logsize 8 --nbits 128 (examples/pippenger.rs:19-94, README.md:5); the whole
    gen-2 proof of that shape is made on the GPU under the built-in merlin transcript and accepted by the library's verifier and
    the pairing check (verify_pippenger, pippenger.rs:562-606)"""
    from test_verifier_gpu import _prove_merlin, _setup
    from gkr_msm_amd import verifier as VF
    from pyref import g1 as G
    from pyref import pairing as PR
    x_log, d_log, nbits = 16, 8, 128
    t0 = time.perf_counter()
    plan, d_pts, d_sc, pts_host, sc = check_msm(x_log, d_log, nbits, 0xA11CE)
    g = check_image_part(plan, d_pts, pts_host, sc, x_log, d_log, nbits, 8)
    y_size = nbits // d_log
    assert g["rounds"] > 1000
    plan.close()
    s = _setup(x_log, d_log, nbits, 0, 16, device_srs=True)
    proof, pair = _prove_merlin(s, b"config-a")
    got = VF.pippenger_verify_merlin(*s["shape"], s["claims"][0], s["claims"][1], G.GEN, 2, b"config-a", proof)
    assert got == pair
    assert VF.kzg_verify_pair(got, PR.G2_GEN, PR.g2_mul(PR.G2_GEN, s["tau"]))
    bad = bytearray(proof)
    bad[len(bad) // 3] ^= 4
    try:
        alt = VF.pippenger_verify_merlin(*s["shape"], s["claims"][0], s["claims"][1], G.GEN, 2, b"config-a", bytes(bad))
        assert not VF.kzg_verify_pair(alt, PR.G2_GEN, PR.g2_mul(PR.G2_GEN, s["tau"]))
    except VF.Rejected:
        pass
    print("[at-size] config A whole proof: %d bytes, verified (y_size %d)" % (len(proof), y_size))
    record("config_a_msm_image_part_and_whole_proof", x_logsize=x_log, d_logsize=d_log, nbits=nbits, rounds=g["rounds"],
           proof_bytes=len(proof), seconds=round(time.perf_counter() - t0, 1),
           checked="MSM + image-part prover vs the C oracle; whole gen-2 proof through verifier + pairing")
    del s
    ffi.lib().gm_release_cached_memory()
    torch.cuda.empty_cache()


def test_gen1_at_the_reference_bench_size():
    """gkr_msm_prove at log_num_points = 16, 2^8 scalar bits: the top of the reference's bench grid
    (benches/gkr_msm_simple.rs:97-107), every transcript message vs the C oracle"""
    lp, lb = 16, 8
    require_host_gib(24, "gen-1 at log_num_points 16")
    t_begin = time.perf_counter()
    n = 1 << lp
    d_pts = H.dev_empty(n * 8)
    ffi.check(ffi.lib().gm_gen_points(C.c_void_p(d_pts.data_ptr()), n, 0x6E31, H.cur_stream()))
    pts_host = H.to_host(d_pts).reshape(-1, 8)
    rng = np.random.default_rng(11)
    bits = rng.integers(0, 2, size=(n << lb), dtype=np.uint8)
    tape = [int.from_bytes(rng.bytes(64), "little") % P for _ in range(6000)]
    g = H.gkr_msm_prove(d_pts, torch.from_numpy(bits).cuda(), lp, lb, tape, msgs_cap=1 << 16)
    ffi.lib().gm_release_cached_memory()
    t0 = time.perf_counter()
    c = O.gkr_msm_prove(pts_host, bits, lp, lb, codec.ints_to_limbs(tape), threads=host_threads(), msgs_cap=1 << 16)
    cpu_s = time.perf_counter() - t0
    assert g["tape_used"] == c["tape_used"] and g["rounds"] == c["rounds"]
    assert codec.from_mont_limbs(c["msgs"]) == g["msgs"], "transcript messages"
    nout = 1 << lb
    assert [codec.from_mont_limbs(c["output"][k * nout:(k + 1) * nout]) for k in range(3)] == g["output"]
    assert codec.from_mont_limbs(c["point"]) == g["point"] and codec.from_mont_limbs(c["evs"]) == g["evs"]
    print("[at-size] gen-1 gkr_msm_prove 2^%d points x 2^%d bits: %d rounds, %d messages bit-exact vs the C oracle (%.1f s on the CPU)" % (
        lp, lb, g["rounds"], len(g["msgs"]), cpu_s))
    record("gen1_at_the_reference_bench_size", log_num_points=lp, log_num_scalar_bits=lb, rounds=g["rounds"], messages=len(g["msgs"]),
           seconds=round(time.perf_counter() - t_begin, 1), checked="every transcript message vs the C oracle")
    torch.cuda.empty_cache()


def test_config_d_one_ranks_share_of_the_window_sharded_msm():
    """BASELINE.json configs[3] (x_logsize=24, nbits=256, windows sharded 8 ways: pushforward.rs:401 is the unit of sharding):
    the share of rank 0 and of rank 5 -- 4 windows over all 2^24 points, twice the cells of config B -- at full size.  The
    oracle computes the same four windows from the scalars shifted down to them (digit k of `s >> 8 y0` is digit y0 + k of s)."""
    from gkr_msm_amd import dist as gdist
    x_log, d_log, nbits, world = 24, 8, 256, 8
    require_host_gib(24, "config D's share (x_logsize 24)")
    t_begin = time.perf_counter()
    y_size = nbits // d_log
    d_pts, d_sc, sc = device_inputs(x_log, nbits, 0xD0D0)
    pts_host = H.to_host(d_pts).reshape(-1, 8)
    for rank in (0, 5):
        y0, y1 = gdist.window_range(rank, world, y_size)
        assert y1 - y0 == 4
        plan = H.MsmPlan(x_log, d_log, y_size, y0, y1)
        plan.run(d_pts, d_sc)
        raw = plan.window_points_raw()
        # the scalars shifted right by 8 * y0 bits, cut to the 32 bits of this rank's windows
        bit0 = d_log * y0
        limb, sh = bit0 // 64, bit0 % 64
        assert sh + 32 <= 64
        sub = np.zeros_like(sc)
        sub[:, 0] = (sc[:, limb] >> np.uint64(sh)) & np.uint64(0xFFFFFFFF)
        t0 = time.perf_counter()
        ref = O.msm(pts_host, sub, x_log, d_log, y1 - y0, threads=host_threads(), want_aux=True)
        cpu_s = time.perf_counter() - t0
        px, py, pz, nb = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_uint64()
        ffi.check(plan.L.gm_msm_bucket_sums(plan.h, C.byref(px), C.byref(py), C.byref(pz), C.byref(nb)))
        assert nb.value == (y1 - y0) << d_log
        for p, k in ((px, "bx"), (py, "by"), (pz, "bz")):
            assert np.array_equal(H.read_dev(p, nb.value * 32).reshape(-1, 4), ref[k]), "bucket sums " + k
        assert np.array_equal(raw, ref["window_cols"]), "window points of rank %d" % rank
        print("[at-size] config D share of rank %d (windows %d..%d, x_logsize %d): bucket sums + window points bit-exact (%.1f s on the CPU)" % (
            rank, y0, y1 - 1, x_log, cpu_s))
        plan.close()
    record("config_d_one_ranks_share", x_logsize=x_log, d_logsize=d_log, nbits=nbits, ranks_checked=[0, 5], world=world,
           seconds=round(time.perf_counter() - t_begin, 1), checked="bucket sums + window points of 4 windows vs the C oracle")
    del d_pts, d_sc
    ffi.lib().gm_release_cached_memory()
    torch.cuda.empty_cache()


def _release_unless_rank_thread():
    """gm_release_cached_memory gives EVERY thread's idle blocks back to the driver and hipFree waits for the device: a rank thread must
    not do that while its sibling ranks have kernels in flight that wait for it"""
    import threading
    if threading.current_thread() is threading.main_thread():
        ffi.lib().gm_release_cached_memory()


def _hold_hardware_queues():
    """Four PROCESSES sharing one GPU are served by its scheduler per hardware queue: a process that holds one queue (one stream) gets its
    latency-bound launches dispatched markedly later than one that holds four -- the sharded image part over 4 ranks measured 75 ms
    with one stream per process and 55 ms with four (same library, same proof; bench.py's ranks hold four after their pipelined MSM
    leg, which is why its figure was the lower one).  The workers of the shared-GPU rehearsals therefore hold GM_TEST_EXTRA_STREAMS
    (default 3) more streams with a kernel run on each; with one process per GPU there is nobody to share the scheduler with."""
    streams = [torch.cuda.Stream() for _ in range(int(os.environ.get("GM_TEST_EXTRA_STREAMS", "3")))]
    for st_ in streams:
        with torch.cuda.stream(st_):
            torch.zeros(1024, device="cuda").add_(1)
    torch.cuda.synchronize()
    return streams


def _sharded_worker(rank, world, port, x_log, d_log, nbits, q):
    """one rank of the at-size sharded proof: operands from gm_gen_points / numpy (identical on every rank), the unsharded
    proof as the reference (pinned to the oracle by test_config_b_msm_and_image_part_at_full_size).  The ranks exchange through the
    library's shared-memory communicator (gm_comm_shm_*), as the ranks of one node do in production."""
    try:
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        for d in (root, os.path.join(root, "oracle"), os.path.join(root, "tests")):
            if d not in sys.path:
                sys.path.insert(0, d)
        import ctypes as C
        from gkr_msm_amd import dist as gd
        y_size = (nbits + d_log - 1) // d_log
        y_log = (y_size - 1).bit_length()
        d_pts, d_sc, sc = device_inputs(x_log, nbits, 0x474B524D534D)
        extra_streams = _hold_hardware_queues()
        pr = np.random.default_rng(7)
        r_pt = [int.from_bytes(pr.bytes(64), "little") % P for _ in range(y_log)]
        tape = [int.from_bytes(pr.bytes(16), "little") for _ in range(4000)]

        def ev(poly):
            cur = list(poly)
            for f in reversed(r_pt):
                cur = [(cur[2 * i] + f * (cur[2 * i + 1] - cur[2 * i])) % P for i in range(len(cur) // 2)]
            return cur[0]
        plan = H.MsmPlan(x_log, d_log, y_size)
        plan.run(d_pts, d_sc)
        w = H.PipWitness(plan, d_pts, y_log)
        outs, bs = w.outputs()
        evs = [ev(o) for o in outs]
        ref = w.prove_image_part(r_pt, evs, tape)
        w.close()
        plan.close()
        _release_unless_rank_thread()
        y0, y1 = gd.window_range(rank, world, y_size)
        comm = gd.ShmComm("/gm-at-size-%d" % port, rank, world)
        plan_s = H.MsmPlan(x_log, d_log, y_size, y0, y1)
        plan_s.run(d_pts, d_sc)
        ws = H.PipWitness(plan_s, d_pts, y_log, comm=comm)
        outs_s, bs_s = ws.outputs()
        a0, b0 = C.c_uint64(), C.c_uint64()
        ffi.lib().gm_sc_stage_counts(C.byref(a0), C.byref(b0))
        ws.prove_image_part(r_pt, evs, tape)            # warm-up (first-use allocations)
        # two timed proofs, each started together (as bench.py's sync_all before its timed call), the faster one recorded
        dt, clock, got = None, None, None
        for _ in range(2):
            comm.sum_fr(np.zeros((1, 4), dtype=np.uint64))
            gd.shard_clock()
            g_ = ws.prove_image_part(r_pt, evs, tape)
            c_ = gd.shard_clock()
            if dt is None or g_["call_s"] < dt:
                dt, clock = g_["call_s"], c_
            got = g_
        a1, b1 = C.c_uint64(), C.c_uint64()
        ffi.lib().gm_sc_stage_counts(C.byref(a1), C.byref(b1))
        ok = (outs_s == outs and bs_s == bs and got["msgs"] == ref["msgs"] and got["point"] == ref["point"] and
              got["evs"] == ref["evs"] and got["rounds"] == ref["rounds"] and got["tape_used"] == ref["tape_used"])
        calls = comm.calls
        ws.close()
        plan_s.close()
        _release_unless_rank_thread()
        # The comparison that separates the cost of SHARDING from the cost of FOUR PROCESSES SHARING ONE GPU: every rank proves, at the
        # same time as the others and with no exchange at all, an independent unsharded image part of its share's size (the first
        # y_size / world windows: the same bucket rows per process, a few rounds fewer because y_logsize is smaller).
        yq = y_size // world
        yq_log = (yq - 1).bit_length()
        plan_q = H.MsmPlan(x_log, d_log, yq)
        plan_q.run(d_pts, d_sc)
        wq = H.PipWitness(plan_q, d_pts, yq_log)
        outs_q, _ = wq.outputs()
        rq = r_pt[:yq_log]

        def evq(poly):
            cur = list(poly)
            for f in reversed(rq):
                cur = [(cur[2 * i] + f * (cur[2 * i + 1] - cur[2 * i])) % P for i in range(len(cur) // 2)]
            return cur[0]
        evs_q = [evq(o) for o in outs_q]
        wq.prove_image_part(rq, evs_q, tape)
        comm.sum_fr(np.zeros((1, 4), dtype=np.uint64))   # start together
        gq = [wq.prove_image_part(rq, evs_q, tape) for _ in range(2)]
        indep = dict(ms=round(1e3 * min(g_["call_s"] for g_ in gq), 1), rounds=gq[0]["rounds"])
        wq.close()
        plan_q.close()
        _release_unless_rank_thread()
        comm.sum_fr(np.zeros((1, 4), dtype=np.uint64))
        one = None
        if rank == 0:
            # the unsharded proof timed ALONE on the GPU: the other ranks are done (they wait in the exchange below without touching it)
            plan = H.MsmPlan(x_log, d_log, y_size)
            plan.run(d_pts, d_sc)
            w = H.PipWitness(plan, d_pts, y_log)
            w.prove_image_part(r_pt, evs, tape)
            one = min(w.prove_image_part(r_pt, evs, tape)["call_s"] for _ in range(2))
            w.close()
            plan.close()
        comm.sum_fr(np.zeros((1, 4), dtype=np.uint64))   # everybody leaves together
        q.put((rank, ok, dict(exchanges=calls, sharded_s=dt, unsharded_alone_s=one, stage_launches=(a1.value - a0.value) // 3,   # (three proofs: one warm-up, two timed)
                              stage_left=b1.value - b0.value, clock=clock, indep=indep), got["rounds"]))
        comm.close()
    except Exception as e:  # report instead of hanging the parent
        import traceback
        q.put((rank, False, repr(e) + traceback.format_exc(), 0))


def test_config_b_image_part_sharded_over_four_ranks():
    """the sharded prover (gm_pip_witness_create_sharded: bucket rows = windows split over the ranks, the round sums exchanged between
    the ranks' host threads) at config B's full size, world 4 on the one GPU.  Every rank's proof equals the unsharded one; the
    sharded rounds take the unsharded device path (pre-enqueued folds, the persistent stage kernel); and -- four ranks sharing ONE
    GPU, so no speed-up is to be had -- the sharded proof stays close to the unsharded proof's time (round 2: 7x slower)."""
    import torch.multiprocessing as mp
    world, x_log, d_log, nbits = 4, 20, 8, 256
    require_host_gib(64, "config B sharded over 4 processes")
    t_begin = time.perf_counter()
    _release_unless_rank_thread()
    torch.cuda.empty_cache()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 35500 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_sharded_worker, args=(r, world, port, x_log, d_log, nbits, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = []
    try:
        for _ in range(world):
            res.append(q.get(timeout=600))
    finally:
        for p in procs:
            p.join(timeout=60)
            if p.is_alive():
                p.kill()
    assert len(res) == world
    res.sort()
    for rank, ok, info, rounds in res:
        assert ok, "rank %d: %s" % (rank, info)
    sharded = max(r[2]["sharded_s"] for r in res)
    alone = res[0][2]["unsharded_alone_s"]
    print("[at-size] config B image-part prover sharded over %d ranks sharing one GPU (x_logsize %d): %d rounds, %.1f ms (slowest rank) "
          "against %.1f ms unsharded alone = %.2fx; %d stage launches per rank, %d left early; equal to the unsharded proof" % (
              world, x_log, res[0][3], 1e3 * sharded, 1e3 * alone, sharded / alone, res[0][2]["stage_launches"], res[0][2]["stage_left"]))
    record("config_b_image_part_sharded_over_four_ranks", x_logsize=x_log, world=world, rounds=res[0][3], transport="shm",
           sharded_ms=round(1e3 * sharded, 1), unsharded_alone_ms=round(1e3 * alone, 1), ratio=round(sharded / alone, 2),
           stage_launches_per_rank=res[0][2]["stage_launches"], stage_left_early=sum(r[2]["stage_left"] for r in res),
           exchanges_per_rank=res[0][2]["exchanges"], proofs_behind_the_exchange_count=3,
           streams_held_per_process=1 + int(os.environ.get("GM_TEST_EXTRA_STREAMS", "3")),
           time_inside_the_communicator_per_rank=[r[2]["clock"] for r in res], per_rank_ms=[round(1e3 * r[2]["sharded_s"], 1) for r in res],
           four_independent_share_sized_proofs_at_once=dict(what="every process proves an unsharded image part over y_size / world windows at the "
                                                            "same time, no exchange: what sharing ONE GPU between the processes costs by itself",
                                                            ms_per_process=[r[2]["indep"]["ms"] for r in res], rounds=res[0][2]["indep"]["rounds"]),
           seconds=round(time.perf_counter() - t_begin, 1), checked="every message equal to the unsharded proof on every rank")
    assert res[0][2]["stage_launches"] >= 30, "the sharded bintree layers did not run in the stage kernel"
    assert sharded <= 2.0 * alone, "sharded over ranks sharing one GPU: %.1f ms against %.1f ms unsharded" % (1e3 * sharded, 1e3 * alone)


def _sharded_pf_worker(rank, world, port, x_log, d_log, nbits, q):
    """one rank of the at-size sharded pushforward argument.  Rank 0 first runs the unsharded image part (its final claims are what the
    argument starts from, pippenger.rs:138-160) and the unsharded argument as the reference, then hands the claims to the others."""
    try:
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        for d in (root, os.path.join(root, "oracle"), os.path.join(root, "tests")):
            if d not in sys.path:
                sys.path.insert(0, d)
        import hashlib
        from gkr_msm_amd import dist as gd
        y_size = (nbits + d_log - 1) // d_log
        y_log = (y_size - 1).bit_length()
        nv = y_log + d_log + x_log
        d_pts, d_sc, sc = device_inputs(x_log, nbits, 0x474B524D534D)
        extra_streams = _hold_hardware_queues()
        pr = np.random.default_rng(7)
        tape = [int.from_bytes(pr.bytes(64), "little") % P for _ in range(4)] + [int.from_bytes(pr.bytes(16), "little") for _ in range(3000)]
        comm = gd.ShmComm("/gm-at-size-pf-%d" % port, rank, world)
        buf = np.zeros((nv + 3, 4), dtype=np.uint64)
        info = {}
        if rank == 0:
            r0 = [int.from_bytes(pr.bytes(64), "little") % P for _ in range(y_log)]
            tape0 = [int.from_bytes(pr.bytes(16), "little") for _ in range(4000)]
            plan = H.MsmPlan(x_log, d_log, y_size)
            plan.run(d_pts, d_sc)
            w = H.PipWitness(plan, d_pts, y_log)
            outs, _ = w.outputs()

            def ev(poly):
                cur = list(poly)
                for f in reversed(r0):
                    cur = [(cur[2 * i] + f * (cur[2 * i + 1] - cur[2 * i])) % P for i in range(len(cur) // 2)]
                return cur[0]
            img = w.prove_image_part(r0, [ev(o) for o in outs], tape0)
            w.close()
            H.pushforward_prove(plan, d_pts, y_log, img["point"], img["evs"], tape)          # warm-up (first-use allocations)
            ref = H.pushforward_prove(plan, d_pts, y_log, img["point"], img["evs"], tape)
            info.update(unsharded_s=ref["call_s"], ref_digest=hashlib.sha256(repr(
                (ref["msgs"], ref["gamma"], ref["matrix"], ref["ac_c"], ref["ac_d"])).encode()).hexdigest())
            plan.close()
            _release_unless_rank_thread()
            buf[:] = codec.to_mont_limbs(list(img["point"]) + list(img["evs"]))
        comm.sum_fr(buf)   # the others contribute zeros: everybody has rank 0's claims
        vals = codec.from_mont_limbs(buf)
        r_pt, evs = vals[:nv], vals[nv:]
        y0, y1 = gd.window_range(rank, world, y_size)
        plan_s = H.MsmPlan(x_log, d_log, y_size, y0, y1)
        plan_s.run(d_pts, d_sc)
        H.pushforward_prove(plan_s, d_pts, y_log, r_pt, evs, tape, comm=comm)      # warm-up: first-use allocations, IPC mappings
        best_s, best_clock, got = None, None, None
        for _ in range(2):                                                          # two timed arguments, started together; the faster one
            comm.sum_fr(np.zeros((1, 4), dtype=np.uint64))
            gd.shard_clock()
            g_ = H.pushforward_prove(plan_s, d_pts, y_log, r_pt, evs, tape, comm=comm)
            c_ = gd.shard_clock()
            if best_s is None or g_["call_s"] < best_s:
                best_s, best_clock = g_["call_s"], c_
            got = g_
        info.update(sharded_s=best_s, rounds=got["rounds"], exchanges=comm.calls, clock=best_clock, ipc=comm.ipc_stats(), digest=hashlib.sha256(repr(
            (got["msgs"], got["gamma"], got["matrix"], got["ac_c"], got["ac_d"])).encode()).hexdigest())
        q.put((rank, True, info))
        comm.sum_fr(np.zeros((1, 4), dtype=np.uint64))   # everybody leaves together
        comm.close()
    except Exception as e:  # report instead of hanging the parent
        import traceback
        q.put((rank, False, repr(e) + traceback.format_exc()))


def test_config_b_pushforward_sharded_over_four_ranks():
    """the pushforward argument with the matrix sharded by windows (gm_pushforward_prove_sharded) at config B's full size, world 4 on
    the one GPU: the messages and claims of every rank equal the unsharded argument's.  The halves of the logup tree's levels are
    re-spread device to device (gm_comm::pull_dev of the shared-memory communicator: HIP IPC handles + copies between the ranks'
    buffers; on a node those copies cross xGMI, here the four ranks share the device -- so the time is a functional check at size
    with all four ranks' work on ONE GPU, not a speed-up)."""
    import torch.multiprocessing as mp
    world, x_log, d_log, nbits = 4, 20, 8, 256
    require_host_gib(64, "config B pushforward sharded over 4 processes")
    t_begin = time.perf_counter()
    _release_unless_rank_thread()
    torch.cuda.empty_cache()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 36500 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_sharded_pf_worker, args=(r, world, port, x_log, d_log, nbits, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = []
    try:
        for _ in range(world):
            res.append(q.get(timeout=900))
    finally:
        for p in procs:
            p.join(timeout=60)
            if p.is_alive():
                p.kill()
    assert len(res) == world
    res.sort()
    for rank, ok, info in res:
        assert ok, "rank %d: %s" % (rank, info)
    ref = res[0][2]["ref_digest"]
    for rank, ok, info in res:
        assert info["digest"] == ref, "rank %d: the sharded argument differs from the unsharded one" % rank
    sharded = max(r[2]["sharded_s"] for r in res)
    print("[at-size] config B pushforward argument sharded over %d ranks sharing one GPU (x_logsize %d): %d rounds, %.0f ms (halves re-spread "
          "device to device over HIP IPC) against %.1f ms unsharded; %d exchanges per rank; equal to the unsharded argument on every rank" % (
              world, x_log, res[0][2]["rounds"], 1e3 * sharded, 1e3 * res[0][2]["unsharded_s"], res[0][2]["exchanges"]))
    record("config_b_pushforward_sharded_over_four_ranks", x_logsize=x_log, world=world, rounds=res[0][2]["rounds"],
           transport="shm (round sums) + HIP IPC pulls (tree halves, access counts)", sharded_ms=round(1e3 * sharded, 1), unsharded_ms=round(1e3 * res[0][2]["unsharded_s"], 1),
           exchanges_per_rank=res[0][2]["exchanges"], seconds=round(time.perf_counter() - t_begin, 1),
           time_inside_the_communicator_per_rank=[r[2]["clock"] for r in res], per_rank_ms=[round(1e3 * r[2]["sharded_s"], 1) for r in res],
           ipc_mappings_opened_closed_held=[r[2]["ipc"] for r in res],
           checked="messages, gamma and the three final claims equal to the unsharded argument on every rank")


def _sharded_worker_q(rank, world, q, port, x_log, d_log, nbits):
    _sharded_worker(rank, world, port, x_log, d_log, nbits, q)


def _sharded_pf_worker_q(rank, world, q, port, x_log, d_log, nbits):
    _sharded_pf_worker(rank, world, port, x_log, d_log, nbits, q)


def test_config_b_sharded_over_four_rank_threads_of_one_process():
    """The same two sharded provers with the four ranks as THREADS of one process (tests/rank_threads.py): the device then runs ONE
    process's queues and does not switch between four -- the switching is what most of the "sharding overhead" of the four-process
    rehearsals above is (a one-GPU artefact: with a GPU per rank there is nothing to switch).  Same checks: every rank's proof equals the
    unsharded one."""
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from rank_threads import run_ranks
    world, x_log, d_log, nbits = 4, 20, 8, 256
    require_host_gib(64, "config B sharded over 4 rank threads")
    t_begin = time.perf_counter()
    ffi.lib().gm_release_cached_memory()
    torch.cuda.empty_cache()
    res = run_ranks(_sharded_worker_q, world, (37500 + os.getpid() % 2000, x_log, d_log, nbits), threads_per_proc=4, timeout=600)
    sharded = max(r[2]["sharded_s"] for r in res)
    alone = res[0][2]["unsharded_alone_s"]
    resp = run_ranks(_sharded_pf_worker_q, world, (38500 + os.getpid() % 2000, x_log, d_log, nbits), threads_per_proc=4, timeout=900)
    ref = resp[0][2]["ref_digest"]
    for rank, ok, info in resp:
        assert info["digest"] == ref, "rank %d: the sharded argument differs from the unsharded one" % rank
    pf_sharded = max(r[2]["sharded_s"] for r in resp)
    pf_alone = resp[0][2]["unsharded_s"]
    print("[at-size] config B over 4 rank THREADS of one process on one GPU: image part %.1f ms against %.1f unsharded alone = %.2fx "
          "(four independent share-sized proofs at once: %s ms); pushforward %.1f ms against %.1f = %.2fx" % (
              1e3 * sharded, 1e3 * alone, sharded / alone, [r[2]["indep"]["ms"] for r in res], 1e3 * pf_sharded, 1e3 * pf_alone, pf_sharded / pf_alone))
    record("config_b_sharded_over_four_rank_threads", x_logsize=x_log, world=world, image_part_sharded_ms=round(1e3 * sharded, 1),
           image_part_unsharded_alone_ms=round(1e3 * alone, 1), image_part_ratio=round(sharded / alone, 2),
           image_part_four_independent_share_sized_proofs_ms=[r[2]["indep"]["ms"] for r in res],
           image_part_time_inside_the_communicator_per_rank=[r[2]["clock"] for r in res],
           pushforward_sharded_ms=round(1e3 * pf_sharded, 1), pushforward_unsharded_ms=round(1e3 * pf_alone, 1),
           pushforward_ratio=round(pf_sharded / pf_alone, 2),
           pushforward_time_inside_the_communicator_per_rank=[r[2]["clock"] for r in resp],
           seconds=round(time.perf_counter() - t_begin, 1),
           checked="every rank's image-part proof and pushforward argument equal the unsharded ones")
    # (rank threads on one device run the plain rounds, tests/rank_threads.py, and so does the unsharded proof of the same process:
    # measured 1.78x and 1.48x; the bound only catches a path that fell off that one -- host-staged pulls, a rank waiting out time-outs)
    assert sharded <= 2.2 * alone and pf_sharded <= 2.2 * pf_alone


def test_config_e_dry_run_of_one_ranks_share_of_the_sharded_prover():
    """BASELINE.json configs[4] (x_logsize=24, bucket rows sharded 8 ways): rank 3's share -- the witness of 4 windows over 2^24
    points (twice config B's cells) and all sumcheck rounds over it -- at full size on one GPU.  A DRY RUN: the all-gather
    callback returns only this rank's slot (the seven other ranks do not exist here), so the round sums and challenges are not
    those of a real proof; what is checked is that the share fits and runs (every kernel at the shape the 8-GPU run launches),
    that its bucket sums are the window-sharded MSM's (pinned by the config D test above), and how long it takes."""
    from gkr_msm_amd import dist as gdist
    x_log, d_log, nbits, world, rank = 24, 8, 256, 8, 3
    require_host_gib(24, "config E's dry run (x_logsize 24)")
    y_size = nbits // d_log
    y_log = (y_size - 1).bit_length()
    d_pts, d_sc, sc = device_inputs(x_log, nbits, 0xE0E0)
    y0, y1 = gdist.window_range(rank, world, y_size)
    plan = H.MsmPlan(x_log, d_log, y_size, y0, y1)
    plan.run(d_pts, d_sc)

    class LoopbackComm:
        def __init__(self):
            self.calls = 0

            def _ag(ctx, buf, nbytes):
                self.calls += 1     # own slot is already in place; the other slots keep whatever the library put there
                return 0
            self._cb = ffi.ALL_GATHER_CB(_ag)
            self.c = ffi.GmComm(None, rank, world, self._cb)
    comm = LoopbackComm()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    w = H.PipWitness(plan, d_pts, y_log, comm=comm)
    torch.cuda.synchronize()
    t_wit = time.perf_counter() - t0
    # this rank's rows of the bucket-sum columns = the bucket sums of its MSM plan
    bs_ptrs = (C.c_void_p * 3)()
    out_ptrs = (C.c_void_p * (3 * (d_log + 1)))()
    n_, ln_ = C.c_uint32(), C.c_uint64()
    ffi.check(w.L.gm_pip_witness_outputs(w.h, out_ptrs, C.byref(n_), C.byref(ln_), bs_ptrs))
    px, py, pz, nb = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_uint64()
    ffi.check(plan.L.gm_msm_bucket_sums(plan.h, C.byref(px), C.byref(py), C.byref(pz), C.byref(nb)))
    rows0 = y0 << d_log
    for k, p in enumerate((px, py, pz)):
        mine = H.read_dev(p, nb.value * 32).reshape(-1, 4)
        full = H.read_dev(bs_ptrs[k], (1 << (y_log + d_log)) * 32).reshape(-1, 4)
        assert np.array_equal(full[rows0:rows0 + nb.value], mine), "bucket-sum rows of this rank"
    pr = np.random.default_rng(5)
    r_pt = [int.from_bytes(pr.bytes(64), "little") % P for _ in range(y_log)]
    r_evs = [int.from_bytes(pr.bytes(64), "little") % P for _ in range(3 * (d_log + 1))]
    tape = [int.from_bytes(pr.bytes(16), "little") for _ in range(6000)]
    g = w.prove_image_part(r_pt, r_evs, tape)
    free, total = torch.cuda.mem_get_info()
    assert g["rounds"] >= 1518 and len(g["msgs"]) > 3 * g["rounds"] and comm.calls > 1000
    print("[at-size] config E dry run, rank %d of %d at x_logsize %d: witness %.0f ms, %d rounds in %.0f ms (%.0f rounds/s), %d exchanges, "
          "%.1f GiB of HBM in use" % (rank, world, x_log, t_wit * 1e3, g["rounds"], g["call_s"] * 1e3, g["rounds"] / g["call_s"],
                                      comm.calls, (total - free) / 2 ** 30))
    record("config_e_dry_run_of_one_ranks_share", x_logsize=x_log, world=world, rank=rank, rounds=g["rounds"],
           seconds=round(g["call_s"] + t_wit, 2), hbm_GiB=round((total - free) / 2 ** 30, 1), checked="fits and runs; bucket-sum rows = the MSM's")
    w.close()
    plan.close()
    del d_pts, d_sc
    ffi.lib().gm_release_cached_memory()
    torch.cuda.empty_cache()


def test_config_e_one_ranks_share_of_the_commitments_at_clm_4():
    """BASELINE.json configs[4]'s commitments: x_logsize=24, commitment_log_multiplicity=4, windows sharded 8 ways.  The KZG key has
    2 * 2^28 - 1 points (pippenger.rs:475-480; 51 GB affine): no rank holds it whole and nobody builds fixed-base tables for it
    (1.5 KB per base).  Rank 3 owns windows 12..15, which use key slices 12..15 of matrix 0 (kzg_basis[x + 2^24 * (y mod 16)],
    pushforward.rs:417): 4 x 2^24 affine points = 6.4 GB on the device.  Its PART of the outer buckets (2 x 2^26 G1 additions) and of
    d_comm / c_comm runs at full size here; the exchange with the other seven ranks is one group element per matrix and commitment
    (gm_g1_combine_parts; exercised with real ranks at small sizes in tests/test_sharded_g1_gpu.py).  Checked: it fits and runs, and
    the part is LINEAR -- the same windows accumulated against the key slices in another slot order give the same share."""
    from gkr_msm_amd import dist as gdist
    x_log, d_log, nbits, world, rank, clm = 24, 8, 256, 8, 3, 4
    require_host_gib(8, "config E's commitment share")
    y_size = nbits // d_log
    n = 1 << x_log
    d_pts, d_sc, sc = device_inputs(x_log, nbits, 0xE1E1)
    y0, y1 = gdist.window_range(rank, world, y_size)
    plan = H.MsmPlan(x_log, d_log, y_size, y0, y1)
    plan.run(d_pts, d_sc)
    need = sorted({y % (1 << clm) for y in range(y0, y1)})
    assert need == [12, 13, 14, 15]
    d_local = H.g1_gen_points(len(need) * n, 0x4B5A47)          # the rank's four key slices (synthetic points: any key works here)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    part = H.msm_g1_outer_part(plan, d_local, {s_: i for i, s_ in enumerate(need)}, clm, n)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    free, total = torch.cuda.mem_get_info()
    assert part["first_matrix"] == 0 and part["n_matrices"] == 1
    # the same share with the slices stored in reverse order: same group elements
    loc_h = H.to_host(d_local).reshape(len(need), -1)
    d_rev = H.to_dev(loc_h[::-1].copy().reshape(-1))
    del loc_h
    part2 = H.msm_g1_outer_part(plan, d_rev, {s_: len(need) - 1 - i for i, s_ in enumerate(need)}, clm, n)
    assert codec.g1_jac_from_limbs(part["d_part"]) == codec.g1_jac_from_limbs(part2["d_part"])
    assert codec.g1_jac_from_limbs(part["c_part"]) == codec.g1_jac_from_limbs(part2["c_part"])
    print("[at-size] config E commitment share, rank %d of %d: 2 x 2^26 G1 additions + 2 weighted sums in %.0f ms, %.1f GiB of HBM in use" % (
        rank, world, dt * 1e3, (total - free) / 2 ** 30))
    record("config_e_commitment_share_clm4", x_logsize=x_log, clm=clm, world=world, rank=rank, key_slices=need, local_key_GB=round(len(need) * n * 96 / 1e9, 1),
           ms=round(dt * 1e3, 1), hbm_GiB=round((total - free) / 2 ** 30, 1), checked="fits and runs; share independent of the slice slot order")
    del d_local, d_rev, part, part2, d_pts, d_sc
    plan.close()
    ffi.lib().gm_release_cached_memory()
    ffi.check(ffi.lib().gm_g1_release_scratch())
    torch.cuda.empty_cache()


def test_config_c_gen1_at_two_to_the_twenty_points():
    """BASELINE.json configs[2], gen-1 (gkr_msm_simple.rs:86-338) at 2^20 points x 2^8 scalar bits -- 16 times past what the CPU
    oracle finishes in a test.  Checked through size-independent properties: the library's verifier (BintreeVerifier /
    SumcheckPolyMapVerifier / SplitVerifier, protocol/bintree.rs:313-395) accepts the prover's stream and ends on the prover's
    claim; that claim is TRUE -- the three final evaluations equal the multilinear extensions of the base columns (bit, px, py;
    gkr_msm_simple.rs:120,161-165) at the final point, computed here from the inputs (px / py with Python integers on the host, the
    2^28-entry bit column by 28 folds of gm_dense_bind); the claimed output (256 x 3) is what the verifier started from; an altered
    stream is rejected."""
    from gkr_msm_amd import verifier as VF
    lp, lb = 20, 8
    t_begin = time.perf_counter()
    n = 1 << lp
    d_pts = H.dev_empty(n * 8)
    ffi.check(ffi.lib().gm_gen_points(C.c_void_p(d_pts.data_ptr()), n, 0x6E32, H.cur_stream()))
    rng = np.random.default_rng(31)
    bits = torch.from_numpy(rng.integers(0, 2, size=(n << lb), dtype=np.uint8)).cuda()
    tape = [int.from_bytes(rng.bytes(64), "little") % P for _ in range(6000)]
    g = H.gkr_msm_prove(d_pts, bits, lp, lb, tape, msgs_cap=1 << 16)
    ffi.lib().gm_release_cached_memory()
    torch.cuda.empty_cache()
    assert g["rounds"] > 1000 and len(g["point"]) == lp + lb
    got = VF.gkr_msm_verify(lp, lb, g["msgs"], tape[: g["tape_used"]])
    assert got["point"] == g["point"] and got["evs"] == g["evs"] and got["tape_used"] == g["tape_used"]
    # the final claim against the inputs: index = point * 2^lb + bit, point[0] <-> the most significant index bit
    r_pt, r_bit = g["point"][:lp], g["point"][lp:]
    pts_host = codec.from_mont_limbs(H.to_host(d_pts).reshape(-1, 4))     # x0, y0, x1, y1, ...

    def mle(vals, pt):
        cur = list(vals)
        for f in reversed(pt):
            cur = [(cur[2 * i] + f * (cur[2 * i + 1] - cur[2 * i])) % P for i in range(len(cur) // 2)]
        return cur[0]
    assert mle(pts_host[0::2], r_pt) == g["evs"][1], "px claim"
    assert mle(pts_host[1::2], r_pt) == g["evs"][2], "py claim"
    one = torch.from_numpy(codec.to_mont_limbs([1]).view(np.int64).reshape(1, 4)).cuda()
    col = bits.to(torch.int64).reshape(-1, 1) * one                        # (2^28, 4): 0 or the Montgomery form of 1
    cols = [col.reshape(-1)]
    del col
    for f in reversed(g["point"]):
        cols = H.dense_bind(cols, f)
    assert codec.from_mont_limbs(H.to_host(cols[0]).reshape(1, 4))[0] == g["evs"][0], "bit claim"
    bad = list(g["msgs"])
    bad[len(bad) // 2] = (bad[len(bad) // 2] + 1) % P
    with pytest.raises(VF.Rejected):
        VF.gkr_msm_verify(lp, lb, bad, tape[: g["tape_used"]])
    record("config_c_gen1_2^20", log_num_points=lp, log_num_scalar_bits=lb, rounds=g["rounds"], messages=len(g["msgs"]),
           prove_ms=round(g["call_s"] * 1e3, 1), seconds=round(time.perf_counter() - t_begin, 1),
           checked="verifier accepts + final claims equal the MLEs of the inputs + tampered stream rejected")
    del cols, bits, d_pts
    ffi.lib().gm_release_cached_memory()
    torch.cuda.empty_cache()


def test_config_c_whole_gen2_proof_at_x_logsize_20():
    """BASELINE.json configs[2], gen-2: PippengerWG::new + Pippenger::prove (pippenger.rs:37-70, 122-294) at x_logsize=20,
    d_logsize=8, nbits=256 under the built-in merlin transcript (real Fiat-Shamir), then verify_pippenger (pippenger.rs:562-606):
    the library verifier reads the proof bytes back, returns the prover's pairing pair, the pairing equation holds against the
    SRS's tau and fails against another; altered proofs are refused by the verifier or by the pairing."""
    from test_verifier_gpu import _prove_merlin, _setup
    from gkr_msm_amd import verifier as VF
    from pyref import g1 as G
    from pyref import pairing as PR
    x_log, d_log, nbits = 20, 8, 256
    t_begin = time.perf_counter()
    s = _setup(x_log, d_log, nbits, 0, 20, device_srs=True)
    t0 = time.perf_counter()
    proof, pair = _prove_merlin(s, b"config-c")
    prove_s = time.perf_counter() - t0
    got = VF.pippenger_verify_merlin(*s["shape"], s["claims"][0], s["claims"][1], G.GEN, 2, b"config-c", proof)
    assert got == pair
    h1 = PR.g2_mul(PR.G2_GEN, s["tau"])
    assert VF.kzg_verify_pair(got, PR.G2_GEN, h1)
    assert not VF.kzg_verify_pair(got, PR.G2_GEN, PR.g2_mul(PR.G2_GEN, s["tau"] + 1))
    refused = 0
    for pos in (7, len(proof) // 3, len(proof) // 2, len(proof) - 9):
        bad = bytearray(proof)
        bad[pos] ^= 4
        try:
            alt = VF.pippenger_verify_merlin(*s["shape"], s["claims"][0], s["claims"][1], G.GEN, 2, b"config-c", bytes(bad))
            assert not VF.kzg_verify_pair(alt, PR.G2_GEN, h1)
        except VF.Rejected:
            refused += 1
    assert refused >= 2
    record("config_c_whole_gen2_proof", x_logsize=x_log, d_logsize=d_log, nbits=nbits, clm=0, proof_bytes=len(proof),
           prove_ms=round(prove_s * 1e3, 1), seconds=round(time.perf_counter() - t_begin, 1),
           checked="merlin proof bytes -> library verifier -> pairing accepts; wrong tau and altered bytes refused")
    del s
    ffi.lib().gm_release_cached_memory()
    ffi.check(ffi.lib().gm_g1_release_scratch())
    torch.cuda.empty_cache()


@pytest.mark.parametrize("kind", ["all_same", "half_in_one_bucket", "zero"])
def test_whole_proof_with_skewed_buckets_at_x_logsize_16(kind):
    """collisions at size: every scalar equal (one bucket of 2^16 points per window: a bintree row 16 levels deep beside 255 empty
    rows, the counter column up to X - 1), half of the points in one bucket, every scalar zero -- whole proof under merlin, library
    verifier, pairing.  The ragged trees, the thin rounds and the access counts see their most skewed shapes."""
    from test_verifier_gpu import _prove_merlin, _setup
    from gkr_msm_amd import verifier as VF
    from pyref import g1 as G
    from pyref import pairing as PR
    x_log, d_log, nbits = int(os.environ.get("GM_TEST_SKEW_XLOG", "16")), 8, 64
    n = 1 << x_log
    t_begin = time.perf_counter()
    sc = np.zeros((n, 4), dtype=np.uint64)
    if kind == "all_same":
        sc[:, 0] = np.uint64(0x9B1B00FF5A3C7E01)
    elif kind == "half_in_one_bucket":
        sc[:, 0] = np.random.default_rng(5).integers(0, 2**63, size=n, dtype=np.uint64)
        sc[::2, 0] = np.uint64(0x0101010101010101)
    # every MSM stage and every message of the image-part prover against the C oracle first
    plan, d_pts, d_sc, pts_host, sc_h = check_msm(x_log, d_log, nbits, 99, scalars=sc)
    check_image_part(plan, d_pts, pts_host, sc_h, x_log, d_log, nbits, 8)
    plan.close()
    del d_pts, d_sc
    s = _setup(x_log, d_log, nbits, 0, 31, device_srs=True, scalars_u64x4=sc)
    t0 = time.perf_counter()
    proof, pair = _prove_merlin(s, b"skew")
    prove_s = time.perf_counter() - t0
    got = VF.pippenger_verify_merlin(*s["shape"], s["claims"][0], s["claims"][1], G.GEN, 2, b"skew", proof)
    assert got == pair
    assert VF.kzg_verify_pair(got, PR.G2_GEN, PR.g2_mul(PR.G2_GEN, s["tau"]))
    record("whole_proof_skewed_buckets_" + kind, x_logsize=x_log, d_logsize=d_log, nbits=nbits, prove_ms=round(prove_s * 1e3, 1),
           seconds=round(time.perf_counter() - t_begin, 1),
           checked="MSM stages + image-part messages bit-exact vs the C oracle; merlin proof bytes -> library verifier -> pairing accepts")
    del s
    ffi.lib().gm_release_cached_memory()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("x_log,d_log,nbits", [(12, 10, 30), (13, 9, 27), (12, 3, 12), (14, 6, 128), (12, 2, 6)])
def test_tiled_scatter_and_block_row_tables_at_other_bucket_widths(x_log, d_log, nbits):
    """the MSM paths that need at least 4096 points (tile-regrouped bucket scatter, block-row tables of the level kernels) at the
    bucket widths the full-size configs do not cover (d_logsize 2, 3, 6, 9, 10), against the C oracle: digits, counter, bucket
    populations, bucket sums, window points, final point"""
    plan, d_pts, d_sc, pts_host, sc = check_msm(x_log, d_log, nbits, 0x7157 + d_log)
    plan.close()
