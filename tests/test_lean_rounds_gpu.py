"""The large-round lean kernels of csrc/sumcheck.hip against the Python oracle, at small sizes and at the edges of their lazy bounds.

lean_prim_of is consulted only for rounds above SC_SPLIT_MAX_PAIRS pairs (2^14), so the ordinary small tests never reach
k_round_deg2_lean9x2, k_round_deg2_lean9_split, k_round_generic3_lean or k_round_prod3_lean.  The dispatch reads
GM_SC_SPLIT_MAX_LOG once per process, so the checks run in child pytest processes with a small threshold and GM_SC_NO_TAIL=1
(the persistent k_stage would otherwise absorb the object); the child cases skip when those variables are absent.  Every child case asserts, through gm_sc_profile, which lean kernel
rows ran with how many pairs, and that no k_stage was launched.

The lazy 9 x 29-bit form is argued per operation in comments ("S <= 10", "S grows by <= 1.5 per pair"); the operands here are
built as stored Montgomery words at the extremes of those bounds (p - 1 everywhere, pairs (0, p - 1) that maximise 2 p1 - p0, ...),
because the kernels load the stored words.  test_renormalisation_at_size runs one launch with 16 and 32 grid-stride iterations
per thread, the only way to reach the (it & 15) == 15 renormalisation."""
import ctypes as C
import os
import subprocess
import sys

import pytest

from gkr_msm_amd import ffi, harness as H
from pyref import field as F
from pyref import gen1 as G1
from pyref import polys as PL
from pyref import pushforward as PF
from pyref import sumcheck as SC
from test_poly_sumcheck_gpu import FN, rand_vecvec, run_rounds

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the single-primitive layer functions lean_prim_of accepts, with their profile names
LFN = dict(FN)
LFN["pt_bit_choice"] = (ffi.make_fn((10, 1)), G1.PT_BIT_CHOICE)
LFN["add_inverses"] = (ffi.make_fn((11, 1)), PF.AddInversesFn)
LFN["logup_layer"] = (ffi.make_fn((12, 1)), PF.LogupLayerFn)
PRIM_NAME = {"aff_l1": "AFF_L1", "aff_l2": "AFF_L2", "aff_l3": "AFF_L3", "proj_l1": "PROJ_L1", "proj_l2": "PROJ_L2",
             "proj_l3": "PROJ_L3", "aff_l1_bc": "AFF_L1+BITCHECK", "pt_bit_choice": "PT_BIT_CHOICE",
             "add_inverses": "ADD_INVERSES", "logup_layer": "LOGUP_LAYER"}
LEAN_PRIMS = list(PRIM_NAME)
GENERIC3_PRIMS = [p for p in LEAN_PRIMS if p != "aff_l1_bc"]   # the generic object's lean path excludes AFF_L1 + BITCHECK

R_INV = pow(F.R, -1, F.P)
W_MAX = F.P - 1          # the largest stored word
GAMMA_MAX = (1 << 128) - 1  # the largest value next_bits(128) gives


def word(w):
    """the canonical value whose stored (Montgomery) word is w"""
    return w * R_INV % F.P


# ---- structured columns: patterns of stored words
PATTERNS = ["all_pm1", "pairs_0_pm1", "pairs_pm1_0", "cells_0_1", "mix"]


def pattern_cols(rng, pattern, k, n):
    def cell(i):
        if pattern == "all_pm1":
            return word(W_MAX)
        if pattern == "pairs_0_pm1":
            return word(W_MAX if i & 1 else 0)
        if pattern == "pairs_pm1_0":
            return word(0 if i & 1 else W_MAX)
        if pattern == "cells_0_1":
            return word(rng.next() & 1)
        c = rng.next() % 6   # mix: the edges above and random values
        return [word(0), word(1), word(W_MAX), word(W_MAX if i & 1 else 0), 1, rng.next_fr()][c]
    return [[cell(i) for i in range(n)] for _ in range(k)]


def edge_point(rng, nv):
    """eq-point coordinates 0 and p - 1, and the values whose stored words are 1 and p - 1, with random ones.  A coordinate of 1 is
    outside the protocol: every round divides by 1 - r (from12, vecvec_eq.rs:197-216), which the oracle refuses."""
    pool = [0, F.P - 1, word(1), word(W_MAX)]
    return [pool[i] if i < len(pool) else (pool[rng.next() % 4] if rng.next() & 1 else rng.next_fr()) for i in range(nv)]


# ---- the children's environment
def child_env():
    lg = os.environ.get("GM_SC_SPLIT_MAX_LOG")
    if lg is None or os.environ.get("GM_SC_NO_TAIL") != "1" or "GM_LEAN_GROUP" not in os.environ:
        pytest.skip("runs in the child process of test_lean_kernels_against_oracle (GM_SC_SPLIT_MAX_LOG, GM_SC_NO_TAIL=1)")
    return int(lg), os.environ["GM_LEAN_GROUP"]


def need_group(group):
    lg, g = child_env()
    if g != group:
        pytest.skip("case of the %s group" % group)
    return lg


def stage_launched():
    a, b = C.c_uint64(), C.c_uint64()
    ffi.check(ffi.lib().gm_sc_stage_counts(C.byref(a), C.byref(b)))
    return a.value


class Watch:
    """the lean rows of gm_sc_profile over one object, and the k_stage count"""

    def __enter__(self):
        self.stage0 = stage_launched()
        H.sc_profile(1)
        return self

    def __exit__(self, exc_type, *exc):
        if exc_type is not None:   # reading would synchronise the stream, where a fold may still wait for its challenge
            H.sc_profile(0)
            return False
        rows, _, _ = H.sc_profile_read()
        H.sc_profile(0)
        self.rows = {r["kernel"]: r for r in rows}
        self.stage1 = stage_launched()
        return False

    def check(self, expected):
        """expected: {kernel row: [pairs of every launch]}; rows with no launch must be absent"""
        assert self.stage1 == self.stage0, "k_stage ran: the object did not stay on the round kernels"
        want = {k: v for k, v in expected.items() if v}
        assert sorted(self.rows) == sorted(want), (sorted(self.rows), sorted(want))
        for k, v in want.items():
            assert self.rows[k]["launches"] == len(v) and self.rows[k]["pairs"] == sum(v), (k, self.rows[k], v)


def dense_lean_pairs(nv, lg):
    return [1 << (nv - 1 - r) for r in range(nv) if (1 << (nv - 1 - r)) > (1 << lg)]


def dense_deg2_case(name, nv, cols, point, gamma, lg, rng):
    fn, pyf = LFN[name]
    outs = PL.dense_algfn_map(cols, pyf)
    claims = [PL.evaluate_poly(o, point) for o in outs]
    ref = SC.DenseDeg2SumcheckObjectSO.rlc(cols, pyf, claims, point, gamma)
    with Watch() as w:
        gpu = H.Sumcheckable.dense_deg2(fn, nv, H.cols_to_dev(cols), point, gamma, claims)
        assert gpu.claim() == ref.claim
        run_rounds(gpu, ref, nv, rng)
        gpu.close()
    w.check({"k_round_deg2_lean<%s,dense>" % PRIM_NAME[name]: dense_lean_pairs(nv, lg)})


def generic_case(name, nv, cols, point, gamma, lg, rng):
    if name == "prod3":
        claim = sum(a * b % F.P * c for a, b, c in zip(*cols)) % F.P
        ref = SC.DenseSumcheckObjectSO(cols, SC.Prod3Fn(), nv, claim)
        row = "k_round_prod3_lean"
        with Watch() as w:
            gpu = H.Sumcheckable.dense(1, None, nv, H.cols_to_dev(cols), 0, claim)
            run_rounds(gpu, ref, nv, rng)
            gpu.close()
    else:
        fn, pyf = LFN[name]
        claims = [PL.evaluate_poly(o, point) for o in PL.dense_algfn_map(cols, pyf)]
        ref = SC.dense_eq_sumcheck_object(cols, pyf, point, claims, gamma)
        row = "k_round_generic3_lean<%s>" % PRIM_NAME[name]
        with Watch() as w:
            gpu = H.Sumcheckable.dense(0, fn, nv, H.cols_to_dev(cols + [PL.eq_poly_sequence_last(point)]), gamma, ref.claim)
            run_rounds(gpu, ref, nv, rng)
            gpu.close()
    w.check({row: dense_lean_pairs(nv, lg)})


def vecvec_from_lens(rng, k, row_log, col_log, lens):
    data = [[[rng.next_fr() for _ in range(ln)] for ln in lens] for _ in range(k)]
    rpad = [rng.next_fr() for _ in range(k)]
    cpad = [rng.next_fr() for _ in range(k)]
    return ([PL.VecVec(data[c], rpad[c], cpad[c], row_log, col_log) for c in range(k)],
            H.VV.from_host(data, rpad, cpad, row_log, col_log))


def vecvec_case(name, py, gpu_vv, row_log, col_log, point, gamma, lg, rng):
    """every round against the oracle; the sparse rounds whose capacity bound (ScVecVecDeg2::cells_bound: the total at first,
    then bound / 2 + rows per bind) exceeds the threshold are the lean VecVec kernel's, with the exact cell counts of the oracle's
    rows.  Returns (lean sparse rounds, split sparse rounds)."""
    fn, pyf = LFN[name]
    nv = row_log + col_log
    outs = [p.to_dense() for p in PL.vecvec_map(py, pyf)]
    claims = [PL.evaluate_poly(o, point) for o in outs]
    ref = SC.VecVecDeg2SumcheckObjectSO.rlc(py, pyf, claims, point, col_log, gamma)
    info = gpu_vv.info()
    nrows, cb = info["nrows"], info["total"]
    lean_pairs, n_split = [], 0
    with Watch() as w:
        gpu = H.Sumcheckable.vecvec_deg2(fn, gpu_vv, point, gamma, claims)
        assert gpu.claim() == ref.claim()
        for rnd in range(nv):
            sparse = ref.dense is None and rnd < row_log
            exp = ref.unipoly()
            if sparse:
                if cb // 2 + 1 > (1 << lg):
                    lean_pairs.append(sum(len(r) // 2 for r in ref.polys[0].data))
                else:
                    n_split += 1
                cb = cb // 2 + nrows
            assert gpu.unipoly() == exp, "round %d polynomial" % rnd
            t = rng.next_bits(128)
            gpu.bind(t)
            ref.bind(t)
        assert gpu.final_evals() == ref.final_evals()
        gpu.close()
    assert w.stage1 == w.stage0, "k_stage ran"
    row = "k_round_deg2_lean<%s,vecvec>" % PRIM_NAME[name]
    if lean_pairs:
        assert w.rows[row]["launches"] == len(lean_pairs) and w.rows[row]["pairs"] == sum(lean_pairs), (w.rows.get(row), lean_pairs)
    else:
        assert row not in w.rows
    # the dense rounds after the hand-over may run lean kernels of their own; nothing else may appear
    allowed = {row, "k_round_deg2_lean<%s,dense>" % PRIM_NAME[name], "k_round_generic3_lean<%s>" % PRIM_NAME[name]}
    assert set(w.rows) <= allowed, sorted(w.rows)
    return len(lean_pairs), n_split


# ------------------------------------------------------------------ group "lean": threshold 2^0, every large-round kernel
DENSE_CASES = [(name, nv) for name in LEAN_PRIMS for nv in (2, 3, 7, 10)]


@pytest.mark.parametrize("name,nv", DENSE_CASES)
def test_child_dense_object(name, nv):
    lg = need_group("lean")
    rng = F.SplitMix64(0x1EA4 + 31 * nv + len(name))
    k = LFN[name][1].n_ins
    cols = [[rng.next_fr() for _ in range(1 << nv)] for _ in range(k)]
    point = [rng.next_fr() for _ in range(nv)]
    dense_deg2_case(name, nv, cols, point, rng.next_bits(128), lg, rng)


EDGE_CASES = [(name, pat) for name in LEAN_PRIMS for pat in PATTERNS]


@pytest.mark.parametrize("name,pattern", EDGE_CASES)
def test_child_dense_object_at_the_bounds(name, pattern):
    """stored words at the extremes; eq coordinates 0, p - 1 and the stored words 1 and p - 1; gamma = 2^128 - 1"""
    lg = need_group("lean")
    nv = 6
    rng = F.SplitMix64(0xED6E + PATTERNS.index(pattern) * 16 + len(name))
    cols = pattern_cols(rng, pattern, LFN[name][1].n_ins, 1 << nv)
    dense_deg2_case(name, nv, cols, edge_point(rng, nv), GAMMA_MAX, lg, rng)


GENERIC_CASES = [(name, nv, pat) for name in GENERIC3_PRIMS + ["prod3"] for nv, pat in ((2, None), (5, None), (6, "pairs_0_pm1"),
                                                                                      (6, "mix"))]


@pytest.mark.parametrize("name,nv,pattern", GENERIC_CASES)
def test_child_generic_object(name, nv, pattern):
    """gm_sc_dense_create kind 0 (EqWrapper(GammaWrapper(f))) through k_round_generic3_lean, kind 1 (Prod3Fn) through
    k_round_prod3_lean"""
    lg = need_group("lean")
    rng = F.SplitMix64(0x6E4E + nv * 8 + len(name) + (len(pattern) if pattern else 0))
    k = 3 if name == "prod3" else LFN[name][1].n_ins
    if pattern:
        cols, point, gamma = pattern_cols(rng, pattern, k, 1 << nv), edge_point(rng, nv), GAMMA_MAX
    else:
        cols = [[rng.next_fr() for _ in range(1 << nv)] for _ in range(k)]
        point, gamma = [rng.next_fr() for _ in range(nv)], rng.next_bits(128)
    generic_case(name, nv, cols, point, gamma, lg, rng)


VV_CASES = [("proj_l1", 4, 2, "full"), ("aff_l1_bc", 3, 3, "rows"), ("aff_l2", 4, 2, "nothing"), ("proj_l3", 5, 1, "rows"),
            ("add_inverses", 4, 3, "rows"), ("logup_layer", 3, 2, "full"), ("pt_bit_choice", 4, 2, "nothing"),
            ("proj_l2", 3, 3, "lens01"), ("aff_l3", 2, 3, "lens01"), ("aff_l1", 4, 2, "lens01")]


def vv_operands(rng, name, row_log, col_log, mode):
    k = LFN[name][1].n_ins
    if mode == "lens01":   # rows of length 0 and 1 between full ones, and fewer rows than 2^col_log
        n = (1 << col_log) - 1
        lens = [[0, 1, 1 << row_log, 3][i % 4] for i in range(n)]
        return vecvec_from_lens(rng, k, row_log, col_log, lens)
    return rand_vecvec(rng, k, row_log, col_log, mode)


@pytest.mark.parametrize("name,row_log,col_log,mode", VV_CASES)
def test_child_vecvec_object(name, row_log, col_log, mode):
    lg = need_group("lean")
    rng = F.SplitMix64(0x77 + row_log * 10 + col_log + len(name) + len(mode))
    py, gpu_vv = vv_operands(rng, name, row_log, col_log, mode)
    point = [rng.next_fr() for _ in range(row_log + col_log)]
    n_lean, _ = vecvec_case(name, py, gpu_vv, row_log, col_log, point, rng.next_bits(128), lg, rng)
    assert n_lean > 0


# ------------------------------------------------------------------ group "split": threshold 2^3, lean VecVec then the split kernel
SPLIT_CASES = [("proj_l1", 6, 1, "full"), ("aff_l1_bc", 6, 2, "rows"), ("aff_l2", 5, 0, "rows"), ("aff_l3", 6, 2, "lens01"),
               ("proj_l2", 6, 1, "nothing"), ("proj_l3", 6, 2, "full"), ("aff_l1", 5, 2, "lens01"),
               ("add_inverses", 6, 1, "full"), ("logup_layer", 6, 1, "rows"), ("pt_bit_choice", 6, 1, "full")]


@pytest.mark.parametrize("name,row_log,col_log,mode", SPLIT_CASES)
def test_child_vecvec_lean_then_split(name, row_log, col_log, mode):
    """one object whose large sparse rounds run k_round_deg2_lean9x2<,true> and whose last sparse rounds run
    k_round_deg2_lean9_split; ADD_INVERSES, LOGUP_LAYER and PT_BIT_CHOICE have no split form and run k_round_deg2<true, true>
    there"""
    lg = need_group("split")
    rng = F.SplitMix64(0x5917 + row_log * 10 + col_log + len(name))
    py, gpu_vv = vv_operands(rng, name, row_log, col_log, mode)
    nv = row_log + col_log
    point = edge_point(rng, nv) if mode == "full" else [rng.next_fr() for _ in range(nv)]
    gamma = GAMMA_MAX if mode == "full" else rng.next_bits(128)
    n_lean, n_split = vecvec_case(name, py, gpu_vv, row_log, col_log, point, gamma, lg, rng)
    assert n_lean > 0 and n_split > 0, (n_lean, n_split)


GROUP_CASES = {"lean": len(DENSE_CASES) + len(EDGE_CASES) + len(GENERIC_CASES) + len(VV_CASES), "split": len(SPLIT_CASES)}
FORMS = [("default", "lean", 0), ("split_default", "split", 3)]   # (id, group, GM_SC_SPLIT_MAX_LOG)


@pytest.mark.parametrize("form,group,lg", FORMS, ids=[f[0] for f in FORMS])
def test_lean_kernels_against_oracle(form, group, lg):
    """one child process per split threshold (read once per process); the child must pass every case of its group: a skip there
    means a case did not run"""
    if "GM_LEAN_GROUP" in os.environ:
        pytest.skip("already in a child")
    env = dict(os.environ, GM_SC_SPLIT_MAX_LOG=str(lg), GM_SC_NO_TAIL="1", GM_LEAN_GROUP=group)
    out = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-k", "test_child_"], env=env,
                         cwd=ROOT, capture_output=True, text=True, timeout=600)
    if out.returncode < 0 or out.returncode in (134, 139):   # the device faulted: start nothing more on it
        pytest.exit("child process of %s ended by signal (%d):\n%s" % (form, out.returncode, out.stderr[-3000:]), returncode=1)
    n = GROUP_CASES[group]
    assert out.returncode == 0 and ("%d passed" % n) in out.stdout, out.stdout[-3000:] + out.stderr[-2000:]


# ------------------------------------------------------------------ the renormalisation branch at size
def closed_form_rounds(pyf, gamma, a, b, point, chal):
    """round polynomials of DenseDeg2SumcheckObjectSO.rlc over columns whose pairs are all (a[c], b[c]): the eq weights over the
    unbound variables sum to 1, so round r is M_r ((1 - q) + (2 q - 1) X) F(c(X)) with F the gamma combination of the outputs,
    c(X) = a + X (b - a) in the first round and the constant columns c(t_0) after it, q = point[-1 - r], M_r = prod over the
    bound rounds of (1 - q - t + 2 q t).  Independent of the number of variables."""
    gp = PL.make_gamma_pows(gamma, pyf.n_outs)

    def Fg(v):
        return sum(g * o for g, o in zip(gp, pyf.exec(v))) % F.P
    msgs, M, cur = [], 1, None
    for r, t in enumerate(chal):
        q = point[-1 - r]

        def s(x):
            v = [(ai + x * (bi - ai)) % F.P for ai, bi in zip(a, b)] if cur is None else cur
            return M * ((1 - q) + (2 * q - 1) * x) % F.P * Fg(v) % F.P
        msgs.append(SC.unipoly_from_evals([s(x) for x in range(4)]))
        if cur is None:
            cur = [(ai + t * (bi - ai)) % F.P for ai, bi in zip(a, b)]
        M = M * ((1 - q - t + 2 * q * t) % F.P) % F.P
    return msgs, cur


def at_size_operands(name, nv):
    rng = F.SplitMix64(0xA7 + nv + len(name))
    k = LFN[name][1].n_ins
    a, b = [word(0)] * k, [word(W_MAX)] * k   # pairs (0, p - 1) as stored words: 2 p1 - p0 at its largest
    point = edge_point(rng, nv)
    chal = [rng.next_bits(128) for _ in range(nv)]
    return a, b, point, chal


def period2_claims(pyf, a, b, point):
    """every cell of an output column is f(a) or f(b) alternately: its multilinear extension at the point is
    f(a) + point[-1] (f(b) - f(a)) (the eq weights of the other variables sum to 1)"""
    q = point[-1]
    return [(x + q * (y - x)) % F.P for x, y in zip(pyf.exec(a), pyf.exec(b))]


@pytest.mark.parametrize("name", ["proj_l1", "add_inverses"])
def test_closed_form_matches_the_oracle(name):
    """the closed form test_renormalisation_at_size relies on, against the oracle object at nv = 4 to 8"""
    pyf = LFN[name][1]
    for nv in range(4, 9):
        a, b, point, chal = at_size_operands(name, nv)
        cols = [[a[c], b[c]] * (1 << (nv - 1)) for c in range(pyf.n_ins)]
        claims = [PL.evaluate_poly(o, point) for o in PL.dense_algfn_map(cols, pyf)]
        assert claims == period2_claims(pyf, a, b, point)
        ref = SC.DenseDeg2SumcheckObjectSO.rlc(cols, pyf, claims, point, GAMMA_MAX)
        msgs, cur = closed_form_rounds(pyf, GAMMA_MAX, a, b, point, chal)
        for r in range(nv):
            assert ref.unipoly() == msgs[r], (nv, r)
            ref.bind(chal[r])
        assert ref.final_evals()[:pyf.n_ins] == cur


@pytest.mark.parametrize("name,nv", [("proj_l1", 25), ("add_inverses", 26)])
def test_renormalisation_at_size(name, nv):
    """2^(nv - 1) pairs in the first round over a grid of SC_MAX_BLOCKS x 256 = 2^20 threads: 16 (nv = 25) and 32 (nv = 26)
    grid-stride iterations per thread, so every thread's accumulator passes the (it & 15) == 15 renormalisation of
    k_round_deg2_lean9x2; PROJ_L1 with ordinary terms, ADD_INVERSES with lean9_terms_256.  Worst-case pairs (0, p - 1)."""
    import torch
    from conftest import record_at_size
    fn, pyf = LFN[name]
    k = pyf.n_ins
    free, _ = torch.cuda.mem_get_info()
    need = k * (32 << nv) * 7 // 4 + (32 << nv)   # columns + the fold scratch (half + quarter) + the eq table
    if free < need + (4 << 30):
        pytest.fail("needs %.1f GiB of device memory, %.1f free" % (need / 2 ** 30, free / 2 ** 30))
    a, b, point, chal = at_size_operands(name, nv)
    msgs, cur = closed_form_rounds(pyf, GAMMA_MAX, a, b, point, chal)
    claims = period2_claims(pyf, a, b, point)
    pat = H.cols_to_dev([[a[c], b[c]] for c in range(k)])
    cols = [p.view(1, 8).expand(1 << (nv - 1), 8).contiguous().view(-1) for p in pat]   # period 2, built on the device
    del pat
    gpu = H.Sumcheckable.dense_deg2(fn, nv, cols, point, GAMMA_MAX, claims)
    # the profile is read only after the last round: reading it synchronises the stream, where a pre-enqueued fold waits for
    # the next challenge
    H.sc_profile(1)
    try:
        for r in range(nv):
            assert gpu.unipoly() == msgs[r], "round %d" % r
            gpu.bind(chal[r])
        assert gpu.final_evals()[:k] == cur
        gpu.close()
        rows, _, _ = H.sc_profile_read()
    finally:
        gpu.close()   # releases a fold still waiting for its challenge
        H.sc_profile(0)
    row = {r["kernel"]: r for r in rows}["k_round_deg2_lean<%s,dense>" % PRIM_NAME[name]]
    # the large rounds, from the first: 2^(nv - 1) pairs over 2^20 threads
    assert row["launches"] >= 1 and row["pairs"] == sum(1 << (nv - 1 - r) for r in range(row["launches"])), row
    iters = (1 << (nv - 1)) / (1 << 20)
    del cols
    torch.cuda.empty_cache()
    record_at_size("lean_renormalisation_" + name, num_vars=nv, first_round_pairs=1 << (nv - 1),
                   grid_stride_iterations_per_thread=iters, lean_launches=row["launches"])
    assert iters >= 16
