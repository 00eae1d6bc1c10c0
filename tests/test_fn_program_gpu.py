"""GPU tests of caller-defined AlgFns (gm_fn_program_create) in the maps and the sumcheck objects.  Bit-exact against the Python
oracle (a pyref AlgFn evaluating the same terms) and against the built-in ids the programs restate."""
import ctypes as C

import numpy as np
import pytest

from gkr_msm_amd import codec, ffi, harness as H
from pyref import algfn as A
from pyref import field as F
from pyref import polys as PL
from pyref import sumcheck as SC

pytestmark = pytest.mark.gpu

P = F.P
STATE = 4
A5 = (-F.TE_A) % P      # y1 y2 - a x1 x2 with a = -5: + 5 x1 x2
D = F.TE_D


def py_eval(terms, n_outs, args):
    out = [0] * n_outs
    for coef, o, factors in terms:
        v = coef % P
        for f in factors:
            v = v * args[f] % P
        out[o] = (out[o] + v) % P
    return out


class Prog:
    """a registered program and its Python twin (pyref AlgFn over the same terms)"""

    def __init__(self, name, n_ins, n_outs, deg, terms):
        self.n_ins, self.n_outs, self.deg, self.terms = n_ins, n_outs, deg, terms
        self.id = H.make_program(n_ins, n_outs, deg, terms)
        self.py = A.AlgFn(name, deg, n_ins, n_outs, lambda a: py_eval(terms, n_outs, a))


def proj_l1_terms(m, off_out=0):
    """twisted_edwards_add_l1 over the inputs m[0..6)"""
    x1, y1, z1, x2, y2, z2 = m
    return [(1, off_out, (x1, y2)), (1, off_out + 1, (x2, y1)), (1, off_out + 2, (y1, y2)), (A5, off_out + 2, (x1, x2)),
            (1, off_out + 3, (z1, z2))]


BUILTIN_TERMS = {   # name: (built-in id, n_ins, n_outs, terms)
    "AFF_L1": (1, 4, 3, [(1, 0, (0, 3)), (1, 1, (2, 1)), (1, 2, (1, 3)), (A5, 2, (0, 2))]),
    "AFF_L2": (2, 3, 3, [(1, 0, (0,)), (1, 0, (1,)), (1, 1, (2,)), (1, 2, (0, 1))]),
    "AFF_L3": (3, 3, 3, [(1, 0, (0,)), (P - D, 0, (0, 2)), (1, 1, (1,)), (D, 1, (1, 2)), (1, 2, ()), (P - D * D % P, 2, (2, 2))]),
    "PROJ_L1": (4, 6, 4, proj_l1_terms(range(6))),
    "PROJ_L2": (5, 4, 4, [(1, 0, (0, 3)), (1, 0, (1, 3)), (1, 1, (2, 3)), (1, 2, (3, 3)), (1, 3, (0, 1))]),
    "PROJ_L3": (6, 4, 3, [(1, 0, (2, 0)), (P - D, 0, (3, 0)), (1, 1, (2, 1)), (D, 1, (3, 1)), (1, 2, (2, 2)),
                          (P - D * D % P, 2, (3, 3))]),
    "TRI_L1": (7, 12, 12, proj_l1_terms([0, 1, 2, 6, 7, 8], 0) + proj_l1_terms([3, 4, 5, 9, 10, 11], 4)
               + proj_l1_terms([6, 7, 8, 9, 10, 11], 8)),
    "BITCHECK": (9, 1, 1, [(1, 0, (0, 0)), (P - 1, 0, (0,))]),
    "ADD_INVERSES": (11, 2, 2, [(1, 0, (0,)), (1, 0, (1,)), (1, 1, (0, 1))]),
    "LOGUP_LAYER": (12, 4, 2, [(1, 0, (0, 3)), (1, 0, (1, 2)), (1, 1, (1, 3))]),
}
_PROGS = {}


def builtin_prog(name):
    if name not in _PROGS:
        bid, ni, no, terms = BUILTIN_TERMS[name]
        _PROGS[name] = Prog(name, ni, no, 2, terms)
    return _PROGS[name]


# name: (built-in gm_fn, the same function as a program composition)
def composed(name):
    if name == "L2x5":
        return ffi.make_fn((5, 5)), ffi.make_fn((builtin_prog("PROJ_L2").id, 5))
    if name == "AFF_L1+BCx2":
        return ffi.make_fn((1, 1), (9, 2)), ffi.make_fn((builtin_prog("AFF_L1").id, 1), (builtin_prog("BITCHECK").id, 2))
    bid = BUILTIN_TERMS[name][0]
    return ffi.make_fn((bid, 1)), ffi.make_fn((builtin_prog(name).id, 1))


def shape(fn):
    ni, no, dg = C.c_int32(), C.c_int32(), C.c_int32()
    ffi.check(ffi.lib().gm_fn_shape(C.byref(fn), C.byref(ni), C.byref(no), C.byref(dg)))
    return ni.value, no.value, dg.value


def rand_limbs(rs, n):
    """n random canonical field elements as raw Montgomery limbs (top limb < p's)"""
    a = rs.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64) * 2 + rs.integers(0, 2, size=(n, 4), dtype=np.uint64)
    a[:, 3] &= np.uint64(0x3FFFFFFFFFFFFFFF)
    return a


def rand_dev_cols(rs, k, n):
    return [H.to_dev(rand_limbs(rs, n)) for _ in range(k)]


def raw(tensors):
    return [H.to_host(t).copy() for t in tensors]


def rand_cols(rng, k, n):
    return [[rng.next_fr() for _ in range(n)] for _ in range(k)]


def stage_counts():
    a, b = C.c_uint64(), C.c_uint64()
    ffi.check(ffi.lib().gm_sc_stage_counts(C.byref(a), C.byref(b)))
    return a.value, b.value


def transcript(obj, chal):
    """round polynomials, claims and final evaluations of one object driven with the challenges chal"""
    polys, claims = [], [obj.claim()]
    for t in chal:
        polys.append(obj.unipoly())
        obj.bind(t)
        claims.append(obj.claim())
    return polys, claims, obj.final_evals()


def run_pair(a, b, nrounds, rng):
    """drive two objects with the same challenges, one after the other (objects sharing a stream must not interleave their rounds: a
    pre-enqueued fold of one waits in the stream for its challenge); every round polynomial, claim and final evaluation equal"""
    chal = [rng.next_bits(128) for _ in range(nrounds)]
    pa, ca, fa = transcript(a, chal)
    a.close()
    pb, cb, fb = transcript(b, chal)
    b.close()
    for rnd in range(nrounds):
        assert pa[rnd] == pb[rnd], "round %d polynomial" % rnd
    assert ca == cb and fa == fb


def run_oracle(gpu, ref, nrounds, rng):
    for rnd in range(nrounds):
        assert gpu.unipoly() == ref.unipoly(), "round %d polynomial" % rnd
        t = rng.next_bits(128)
        gpu.bind(t)
        ref.bind(t)
    assert gpu.final_evals() == ref.final_evals()


def rand_vecvec(rng, k, row_log, col_log, mode):
    if mode == "full":
        nrows, lens = 1 << col_log, [1 << row_log] * (1 << col_log)
    elif mode == "rows":
        nrows = 1 << col_log
        lens = [rng.next() % ((1 << row_log) + 1) for _ in range(nrows)]
    else:
        nrows = 1 + rng.next() % (1 << col_log)
        lens = [rng.next() % ((1 << row_log) + 1) for _ in range(nrows)]
    if max(lens) < 2:
        lens[0] = 2
    data = [[[rng.next_fr() for _ in range(l)] for l in lens] for _ in range(k)]
    rpad = [rng.next_fr() for _ in range(k)]
    cpad = [rng.next_fr() for _ in range(k)]
    py = [PL.VecVec(data[c], rpad[c], cpad[c], row_log, col_log) for c in range(k)]
    return py, H.VV.from_host(data, rpad, cpad, row_log, col_log)


def random_program(rng, n_ins, n_outs, deg, n_terms, exact_deg=True):
    terms = []
    for t in range(n_terms):
        nf = deg if (exact_deg and t == 0) else rng.next() % (deg + 1)
        coef = [0, 1, P - 1][t % 3] if t < 3 else rng.next_fr()
        terms.append((coef, rng.next() % n_outs, tuple(rng.next() % n_ins for _ in range(nf))))
    return terms


FOO = [(1, 0, (0,)), (1, 0, (1,)), (1, 1, (1,)), (1, 1, (2,))]   # foo = (i0 + i1, i1 + i2)


# ---------------------------------------------------------------------------------------------------- 1. the reference's ArcedAlgFn tests
def test_reference_arced_algfn_maps():
    foo = Prog("foo", 3, 2, 1, FOO)
    fn = ffi.make_fn((foo.id, 1))
    rng = F.SplitMix64(392)
    nv = 8
    cols = rand_cols(rng, 3, 1 << nv)
    assert H.cols_to_host(H.dense_map(fn, H.cols_to_dev(cols), 2)) == PL.dense_algfn_map(cols, foo.py)
    for idx in (PL.LO(0), PL.HI(0)):
        out = H.cols_to_host(H.dense_map_split(fn, H.cols_to_dev(cols), 2, idx.lo_usize(nv), 1))
        assert out == PL.dense_algfn_map_split(cols, foo.py, idx, 1)
    # VecVec map / map_split / map_split_to_dense (vecvec.rs:791-860)
    for mode in ("full", "rows", "nothing"):
        py, gpu = rand_vecvec(rng, 3, 3, 3, mode)
        m_py, m_gpu = PL.vecvec_map(py, foo.py), gpu.map(fn)
        rows, rp, cp = m_gpu.rows()
        assert rows == [p.data for p in m_py] and rp == [p.row_pad for p in m_py] and cp == [p.col_pad for p in m_py]
        s_py, s_gpu = PL.vecvec_map_split(py, foo.py, PL.LO(0), 1), gpu.map_split(fn, 1)
        rows, rp, cp = s_gpu.rows()
        assert rows == [p.data for p in s_py] and rp == [p.row_pad for p in s_py] and cp == [p.col_pad for p in s_py]
        py1, gpu1 = rand_vecvec(rng, 3, 1, 3, mode)
        exp = PL.vecvec_map_split_to_dense(py1, foo.py, PL.LO(0), 1)
        assert H.cols_to_host(gpu1.map_split_to_dense(fn, 1, 2)) == exp


# ---------------------------------------------------------------------------------------------------- 2. built-ins rewritten as programs
MAP_NAMES = ["AFF_L1", "AFF_L2", "AFF_L3", "PROJ_L1", "PROJ_L2", "PROJ_L3", "TRI_L1", "BITCHECK", "ADD_INVERSES", "LOGUP_LAYER",
             "L2x5", "AFF_L1+BCx2"]


@pytest.mark.parametrize("name", MAP_NAMES)
def test_builtin_twins_maps(name):
    fb, fp = composed(name)
    ni, no, dg = shape(fp)
    assert dg == 2
    rs = np.random.default_rng(len(name))
    n = 1 << 12
    cols = rand_dev_cols(rs, ni, n)
    assert all(np.array_equal(x, y) for x, y in zip(raw(H.dense_map(fp, cols, no)), raw(H.dense_map(fb, cols, no))))
    for lo_bit in (0, 5):
        a, b = raw(H.dense_map_split(fp, cols, no, lo_bit, 1)), raw(H.dense_map_split(fb, cols, no, lo_bit, 1))
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
    if no <= 16:
        rng = F.SplitMix64(7 + len(name))
        _, vv = rand_vecvec(rng, ni, 4, 3, "rows")
        for m_p, m_b in [(vv.map(fp), vv.map(fb)), (vv.map_split(fp, 1), vv.map_split(fb, 1))]:
            assert m_p.rows() == m_b.rows()
        _, vv1 = rand_vecvec(rng, ni, 1, 4, "nothing")
        assert H.cols_to_host(vv1.map_split_to_dense(fp, 1, no)) == H.cols_to_host(vv1.map_split_to_dense(fb, 1, no))


def dev_claims(rng, n):
    return [rng.next_fr() for _ in range(n)]


@pytest.mark.parametrize("name,nv", [("AFF_L1", 16), ("AFF_L2", 16), ("AFF_L3", 16), ("PROJ_L1", 16), ("PROJ_L2", 16), ("PROJ_L3", 16),
                                     ("TRI_L1", 16), ("BITCHECK", 16), ("ADD_INVERSES", 16), ("LOGUP_LAYER", 16), ("L2x5", 16),
                                     ("AFF_L1+BCx2", 16), ("PROJ_L1", 21)])
def test_builtin_twins_dense_deg2(name, nv):
    """at nv >= 16 the first rounds run the one-thread-per-pair form, the last ones the split form; nv 21 = 2^20 pairs"""
    fb, fp = composed(name)
    ni, no, _ = shape(fp)
    rs = np.random.default_rng(nv * 100 + len(name))
    cols = rand_dev_cols(rs, ni, 1 << nv)
    rng = F.SplitMix64(nv + len(name))
    point, gamma, claims = [rng.next_fr() for _ in range(nv)], rng.next_bits(128), dev_claims(rng, no)
    H.sc_profile(1)
    H.sc_profile_read()
    gp = H.Sumcheckable.dense_deg2(fp, nv, cols, point, gamma, claims)
    gb = H.Sumcheckable.dense_deg2(fb, nv, cols, point, gamma, claims)
    run_pair(gp, gb, nv, rng)
    gb.close()
    gp.close()
    rows, _, _ = H.sc_profile_read()
    H.sc_profile(0)
    kernels = {r["kernel"] for r in rows}
    assert "k_round_deg2_prog<dense,pair>" in kernels and "k_round_deg2_prog<dense,split>" in kernels, kernels


def test_program_objects_take_no_builtin_path():
    """an object over a program: no k_stage launch, no lean class in the profile"""
    fb, fp = composed("PROJ_L2")
    rs = np.random.default_rng(5)
    rng = F.SplitMix64(5)
    st0 = stage_counts()
    H.sc_profile(1)
    H.sc_profile_read()
    for nv in (6, 9, 12, 16):
        cols = rand_dev_cols(rs, 4, 1 << nv)
        g = H.Sumcheckable.dense_deg2(fp, nv, cols, [rng.next_fr() for _ in range(nv)], rng.next_bits(128), dev_claims(rng, 4))
        for _ in range(nv):
            g.unipoly()
            g.bind(rng.next_bits(128))
        g.final_evals()
        g.close()
    for mode in ("full", "rows"):
        _, vv = rand_vecvec(rng, 4, 5, 4, mode)
        g = H.Sumcheckable.vecvec_deg2(fp, vv, [rng.next_fr() for _ in range(9)], rng.next_bits(128), dev_claims(rng, 4))
        for _ in range(9):
            g.unipoly()
            g.bind(rng.next_bits(128))
        g.final_evals()
        g.close()
    rows, _, _ = H.sc_profile_read()
    H.sc_profile(0)
    assert stage_counts() == st0
    assert all("_prog<" in r["kernel"] for r in rows), [r["kernel"] for r in rows]


@pytest.mark.parametrize("name,row_log,col_log,mode", [("PROJ_L1", 10, 7, "full"), ("AFF_L1+BCx2", 9, 7, "rows"),
                                                       ("PROJ_L2", 4, 3, "nothing"), ("LOGUP_LAYER", 6, 2, "rows")])
def test_builtin_twins_vecvec_deg2(name, row_log, col_log, mode):
    fb, fp = composed(name)
    ni, no, _ = shape(fp)
    rng = F.SplitMix64(row_log * 31 + col_log)
    _, vv = rand_vecvec(rng, ni, row_log, col_log, mode)
    nv = row_log + col_log
    point, gamma, claims = [rng.next_fr() for _ in range(nv)], rng.next_bits(128), dev_claims(rng, no)
    H.sc_profile(1)
    H.sc_profile_read()
    gp = H.Sumcheckable.vecvec_deg2(fp, vv, point, gamma, claims)
    gb = H.Sumcheckable.vecvec_deg2(fb, vv, point, gamma, claims)
    run_pair(gp, gb, nv, rng)
    gb.close()
    gp.close()
    rows, _, _ = H.sc_profile_read()
    H.sc_profile(0)
    kernels = {r["kernel"] for r in rows}
    assert "k_round_deg2_prog<vecvec,split>" in kernels
    if row_log + col_log >= 16 and mode == "full":
        assert "k_round_deg2_prog<vecvec,pair>" in kernels, kernels


@pytest.mark.parametrize("name,nv", [("PROJ_L1", 16), ("TRI_L1", 8), ("AFF_L1+BCx2", 16), ("LOGUP_LAYER", 6)])
def test_builtin_twins_kind0(name, nv):
    fb, fp = composed(name)
    ni, no, _ = shape(fp)
    rs = np.random.default_rng(nv)
    rng = F.SplitMix64(nv * 3)
    cols = rand_dev_cols(rs, ni + 1, 1 << nv)
    gamma, claim = rng.next_bits(128), rng.next_fr()
    H.sc_profile(1)
    H.sc_profile_read()
    gp = H.Sumcheckable.dense(0, fp, nv, cols, gamma, claim)
    gb = H.Sumcheckable.dense(0, fb, nv, cols, gamma, claim)
    run_pair(gp, gb, nv, rng)
    gp.close()
    gb.close()
    rows, _, _ = H.sc_profile_read()
    H.sc_profile(0)
    kernels = {r["kernel"] for r in rows}
    assert "k_round_generic_prog<3,split>" in kernels
    if nv >= 16:
        assert "k_round_generic_prog<3,pair>" in kernels


# ---------------------------------------------------------------------------------------------------- 3. random programs against the oracle
@pytest.mark.parametrize("deg", [1, 2, 3, 4])
def test_random_program_maps(deg):
    rng = F.SplitMix64(40 + deg)
    p = Prog("p", 4, 3, deg, random_program(rng, 4, 3, deg, 9))
    q = Prog("q", 2, 2, deg, random_program(rng, 2, 2, deg, 5))
    cases = [(ffi.make_fn((p.id, 1)), p.py), (ffi.make_fn((p.id, 3)), A.RepeatedAlgFn(p.py, 3)),
             (ffi.make_fn((p.id, 1), (q.id, 1)), A.StackedAlgFn(p.py, q.py))]
    for fn, pyf in cases:
        cols = rand_cols(rng, pyf.n_ins, 70)
        assert H.cols_to_host(H.dense_map(fn, H.cols_to_dev(cols), pyf.n_outs)) == PL.dense_algfn_map(cols, pyf)
        cols = rand_cols(rng, pyf.n_ins, 64)
        for lo in (0, 3):
            out = H.cols_to_host(H.dense_map_split(fn, H.cols_to_dev(cols), pyf.n_outs, lo, 1))
            assert out == PL.dense_algfn_map_split(cols, pyf, PL.LO(lo), 1)
        if pyf.n_outs <= 16:
            py, vv = rand_vecvec(rng, pyf.n_ins, 3, 2, "rows")
            assert vv.map(fn).to_dense() == [x.to_dense() for x in PL.vecvec_map(py, pyf)]
            s = PL.vecvec_map_split(py, pyf, PL.LO(0), 1)
            assert vv.map_split(fn, 1).rows()[0] == [x.data for x in s]


def test_random_program_deg2_objects():
    rng = F.SplitMix64(2)
    p = Prog("p", 3, 3, 2, random_program(rng, 3, 3, 2, 10))
    q = Prog("q", 2, 2, 2, random_program(rng, 2, 2, 2, 4))
    cases = [(ffi.make_fn((p.id, 1)), p.py), (ffi.make_fn((p.id, 3)), A.RepeatedAlgFn(p.py, 3)),
             (ffi.make_fn((p.id, 1), (q.id, 1)), A.StackedAlgFn(p.py, q.py))]
    for fn, pyf in cases:
        for nv in (1, 5, 8):
            cols = rand_cols(rng, pyf.n_ins, 1 << nv)
            point, gamma = [rng.next_fr() for _ in range(nv)], rng.next_bits(128)
            claims = [PL.evaluate_poly(o, point) for o in PL.dense_algfn_map(cols, pyf)]
            ref = SC.DenseDeg2SumcheckObjectSO.rlc(cols, pyf, claims, point, gamma)
            gpu = H.Sumcheckable.dense_deg2(fn, nv, H.cols_to_dev(cols), point, gamma, claims)
            assert gpu.claim() == ref.claim
            run_oracle(gpu, ref, nv, rng)
        for mode, rl, cl in [("full", 3, 2), ("rows", 4, 2), ("nothing", 3, 3)]:
            py, vv = rand_vecvec(rng, pyf.n_ins, rl, cl, mode)
            nv = rl + cl
            point, gamma = [rng.next_fr() for _ in range(nv)], rng.next_bits(128)
            claims = [PL.evaluate_poly(o.to_dense(), point) for o in PL.vecvec_map(py, pyf)]
            ref = SC.VecVecDeg2SumcheckObjectSO.rlc(py, pyf, claims, point, cl, gamma)
            gpu = H.Sumcheckable.vecvec_deg2(fn, vv, point, gamma, claims)
            assert gpu.claim() == ref.claim()
            run_oracle(gpu, ref, nv, rng)


@pytest.mark.parametrize("deg", [1, 2, 3])
def test_random_program_kind0(deg):
    rng = F.SplitMix64(60 + deg)
    p = Prog("p", 3, 2, deg, random_program(rng, 3, 2, deg, 7))
    q = Prog("q", 2, 2, deg, random_program(rng, 2, 2, deg, 4))
    for fn, pyf in [(ffi.make_fn((p.id, 1)), p.py), (ffi.make_fn((p.id, 3)), A.RepeatedAlgFn(p.py, 3)),
                    (ffi.make_fn((p.id, 1), (q.id, 1)), A.StackedAlgFn(p.py, q.py))]:
        nv = 6
        cols = rand_cols(rng, pyf.n_ins, 1 << nv)
        point, gamma = [rng.next_fr() for _ in range(nv)], rng.next_bits(128)
        claims = [PL.evaluate_poly(o, point) for o in PL.dense_algfn_map(cols, pyf)]
        ref = SC.dense_eq_sumcheck_object(cols, pyf, point, claims, gamma)
        gpu = H.Sumcheckable.dense(0, fn, nv, H.cols_to_dev(cols + [PL.eq_poly_sequence_last(point)]), gamma, ref.claim)
        run_oracle(gpu, ref, nv, rng)


# ---------------------------------------------------------------------------------------------------- 4. gen-1's combfunc
def test_gen1_combfunc_kind0_four_points():
    """combfunc = [i0, i1, i2^2 i0, i2^2 i0] (src/protocol/sumcheck.rs:734): deg 3, D = 4 evaluation points"""
    cf = Prog("combfunc", 3, 4, 3, [(1, 0, (0,)), (1, 1, (1,)), (1, 2, (2, 2, 0)), (1, 3, (2, 2, 0))])
    fn = ffi.make_fn((cf.id, 1))
    st0 = stage_counts()
    H.sc_profile(1)
    H.sc_profile_read()
    rng = F.SplitMix64(734)
    nv = 7
    cols = rand_cols(rng, 3, 1 << nv)
    point, gamma = [rng.next_fr() for _ in range(nv)], rng.next_bits(128)
    claims = [PL.evaluate_poly(o, point) for o in PL.dense_algfn_map(cols, cf.py)]
    ref = SC.dense_eq_sumcheck_object(cols, cf.py, point, claims, gamma)
    gpu = H.Sumcheckable.dense(0, fn, nv, H.cols_to_dev(cols + [PL.eq_poly_sequence_last(point)]), gamma, ref.claim)
    u = gpu.unipoly()
    assert len(u) == 5 and u == ref.unipoly()
    t = rng.next_bits(128)
    gpu.bind(t)
    ref.bind(t)
    run_oracle(gpu, ref, nv - 1, rng)
    gpu.close()
    # the large form (more than 2^14 pairs; too slow for the Python oracle) against the same function with its factors reordered
    cf2 = Prog("combfunc2", 3, 4, 3, [(1, 0, (0,)), (1, 1, (1,)), (1, 2, (0, 2, 2)), (1, 3, (2, 0, 2))])
    rs = np.random.default_rng(734)
    rng = F.SplitMix64(735)
    nv = 16
    cols = rand_dev_cols(rs, 4, 1 << nv)
    gamma, claim = rng.next_bits(128), rng.next_fr()
    a = H.Sumcheckable.dense(0, fn, nv, cols, gamma, claim)
    b = H.Sumcheckable.dense(0, ffi.make_fn((cf2.id, 1)), nv, cols, gamma, claim)
    run_pair(a, b, nv, rng)
    a.close()
    b.close()
    rows, _, _ = H.sc_profile_read()
    H.sc_profile(0)
    kernels = {r["kernel"] for r in rows}
    assert {"k_round_generic_prog<4,split>", "k_round_generic_prog<4,pair>"} <= kernels, kernels
    assert all("_prog<" in r["kernel"] for r in rows)
    assert stage_counts() == st0


# ---------------------------------------------------------------------------------------------------- 5. lifetime
def test_destroy_with_live_object_and_after_map():
    L = ffi.lib()
    p = Prog("pl2", 4, 4, 2, BUILTIN_TERMS["PROJ_L2"][3])
    fn = ffi.make_fn((p.id, 2))
    rng = F.SplitMix64(11)
    nv = 7
    cols = rand_cols(rng, 8, 1 << nv)
    pyf = A.RepeatedAlgFn(A.PROJ_L2, 2)
    point, gamma = [rng.next_fr() for _ in range(nv)], rng.next_bits(128)
    claims = [PL.evaluate_poly(o, point) for o in PL.dense_algfn_map(cols, pyf)]
    ref = SC.DenseDeg2SumcheckObjectSO.rlc(cols, pyf, claims, point, gamma)
    gpu = H.Sumcheckable.dense_deg2(fn, nv, H.cols_to_dev(cols), point, gamma, claims)
    assert L.gm_fn_program_destroy(p.id) == STATE
    assert gpu.unipoly() == ref.unipoly()
    t = rng.next_bits(128)
    gpu.bind(t)
    ref.bind(t)
    assert L.gm_fn_program_destroy(p.id) == STATE
    run_oracle(gpu, ref, nv - 1, rng)
    gpu.close()
    assert L.gm_fn_program_destroy(p.id) == 0
    assert L.gm_fn_program_destroy(p.id) == 1
    # the VecVec object hands its program to the dense stage: held until the object is gone
    q = Prog("pl1", 6, 4, 2, BUILTIN_TERMS["PROJ_L1"][3])
    py, vv = rand_vecvec(rng, 6, 3, 2, "rows")
    point = [rng.next_fr() for _ in range(5)]
    claims = [PL.evaluate_poly(o.to_dense(), point) for o in PL.vecvec_map(py, A.PROJ_L1)]
    ref = SC.VecVecDeg2SumcheckObjectSO.rlc(py, A.PROJ_L1, claims, point, 2, gamma)
    gpu = H.Sumcheckable.vecvec_deg2(ffi.make_fn((q.id, 1)), vv, point, gamma, claims)
    run_oracle(gpu, ref, 5, rng)
    assert L.gm_fn_program_destroy(q.id) == STATE
    gpu.close()
    assert L.gm_fn_program_destroy(q.id) == 0
    # destroying a program right after an enqueued map: the map's output is complete and correct
    r = Prog("pl3", 4, 3, 2, BUILTIN_TERMS["PROJ_L3"][3])
    cols = rand_cols(rng, 4, 1 << 16)
    dev = H.cols_to_dev(cols)
    outs = H.dense_map(ffi.make_fn((r.id, 1)), dev, 3)
    assert L.gm_fn_program_destroy(r.id) == 0
    assert H.cols_to_host(outs) == PL.dense_algfn_map(cols, A.PROJ_L3)
    # an unknown id everywhere
    assert L.gm_dense_map(C.byref(ffi.make_fn((r.id, 1))), H.ptr_array(dev), H.ptr_array(outs), 1 << 16, H.cur_stream()) == 1
    h = C.c_void_p()
    g, c = H.fr_arg([1]), H.fr_arg([0, 0, 0])
    assert L.gm_sc_dense_create(0, C.byref(ffi.make_fn((r.id, 1))), 16, H.ptr_array(dev), g.ctypes.data, c.ctypes.data, C.byref(h),
                                H.cur_stream()) == 1


def test_object_refusals():
    L = ffi.lib()
    p3 = Prog("cube", 2, 2, 3, [(1, 0, (0, 0, 1)), (1, 1, (1,))])
    p4 = Prog("quartic", 2, 2, 4, [(1, 0, (0, 0, 1, 1)), (1, 1, (1,))])
    rs = np.random.default_rng(1)
    cols = rand_dev_cols(rs, 3, 1 << 4)
    g, c = H.fr_arg([3]), H.fr_arg([0, 0])
    h = C.c_void_p()
    pt = H.fr_arg([5] * 4)
    # deg-2 objects take degree-2 programs only; kind 0 degree 1 .. 3; kinds 1 and 2 none
    assert L.gm_sc_dense_deg2_create(C.byref(ffi.make_fn((p3.id, 1))), 4, H.ptr_array(cols), pt.ctypes.data, g.ctypes.data,
                                     c.ctypes.data, C.byref(h), H.cur_stream()) == 1
    assert L.gm_sc_dense_create(0, C.byref(ffi.make_fn((p4.id, 1))), 4, H.ptr_array(cols), g.ctypes.data, c.ctypes.data, C.byref(h),
                                H.cur_stream()) == 1
    for kind in (1, 2):
        assert L.gm_sc_dense_create(kind, C.byref(ffi.make_fn((p3.id, 1))), 4, H.ptr_array(cols), g.ctypes.data, c.ctypes.data,
                                    C.byref(h), H.cur_stream()) == 1
    mixed = ffi.make_fn((p3.id, 1), (ffi.FN_ID, 1))
    assert L.gm_sc_dense_create(0, C.byref(mixed), 4, H.ptr_array(cols), g.ctypes.data, c.ctypes.data, C.byref(h), H.cur_stream()) == 1
    assert b"mixed" in L.gm_last_error()
    H.destroy_program(p3.id)
    H.destroy_program(p4.id)
