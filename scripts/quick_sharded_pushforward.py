"""Config-sized sharded pushforward argument over WORLD processes sharing the GPU, with progress lines (development aid):
python scripts/quick_sharded_pushforward.py [x_log] [d_log] [nbits] [world]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, d)


def worker(rank, world, tag, x_log, d_log, nbits, q):
    try:
        import numpy as np
        from gkr_msm_amd import codec, dist as gd, ffi, harness as H
        from test_at_size_gpu import device_inputs, P
        ffi.lib().gm_set_wait_timeout_ms(8000)

        def say(msg):
            print("[rank %d %.2f] %s" % (rank, time.perf_counter(), msg), flush=True)
        y_size = (nbits + d_log - 1) // d_log
        y_log = (y_size - 1).bit_length()
        nv = y_log + d_log + x_log
        d_pts, d_sc, sc = device_inputs(x_log, nbits, 0x474B524D534D)
        pr = np.random.default_rng(7)
        tape = [int.from_bytes(pr.bytes(64), "little") % P for _ in range(4)] + [int.from_bytes(pr.bytes(16), "little") for _ in range(3000)]
        comm = gd.ShmComm("/gm-quick-pf-%s" % tag, rank, world)
        r_pt = [int.from_bytes(pr.bytes(64), "little") % P for _ in range(nv)]
        evs = [int.from_bytes(pr.bytes(64), "little") % P for _ in range(3)]
        # (claims that are not the image's: the argument's sumchecks do not check them against the columns until the verifier does;
        # the logup identity holds regardless, the combined sumcheck's first-round check is disabled by using consistent claims? no:
        # use the unsharded image part for true claims when the argument asserts them)
        y0, y1 = gd.window_range(rank, world, y_size)
        plan_s = H.MsmPlan(x_log, d_log, y_size, y0, y1)
        plan_s.run(d_pts, d_sc)
        say("plan ready")
        for it in range(3):
            gd.shard_clock()
            try:
                got = H.pushforward_prove(plan_s, d_pts, y_log, r_pt, evs, tape, comm=comm)
                say("call %d: %.1f ms, %s, ipc %s" % (it, 1e3 * got["call_s"], gd.shard_clock(), comm.ipc_stats()))
            except Exception as e:
                say("call %d failed: %s" % (it, str(e)[:300]))
                if "does not sum to the claim" not in str(e):
                    break
        q.put((rank, True))
    except Exception as e:
        import traceback
        print("[rank %d] %s" % (rank, traceback.format_exc()), flush=True)
        q.put((rank, False))


if __name__ == "__main__":
    import torch.multiprocessing as mp
    threads = "--threads" in sys.argv     # the ranks as threads of ONE process (no switching between processes on the shared GPU)
    a = [int(v) for v in sys.argv[1:] if not v.startswith("--")]
    x_log, d_log, nbits, world = (a + [20, 8, 256, 4][len(a):])[:4]
    if threads:
        os.environ.setdefault("GM_SC_NO_PIPELINE", "1")   # rank threads on one device share its queues (tests/rank_threads.py)
        import queue
        import threading
        import torch
        q = queue.Queue()

        def go(r):
            torch.cuda.set_device(0)
            with torch.cuda.stream(torch.cuda.Stream()):
                worker(r, world, "thr%d" % os.getpid(), x_log, d_log, nbits, q)
        th = [threading.Thread(target=go, args=(r,)) for r in range(world)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        print(sorted(q.get_nowait() for _ in range(world)))
        sys.exit(0)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=worker, args=(r, world, str(os.getpid()), x_log, d_log, nbits, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = []
    try:
        for _ in range(world):
            res.append(q.get(timeout=45))
    except Exception as e:
        print("parent: %r (got %d results)" % (e, len(res)), flush=True)
    for p in procs:
        p.join(timeout=10)
        if p.is_alive():
            print("parent: killing pid %d" % p.pid, flush=True)
            p.kill()
    print(sorted(res))
