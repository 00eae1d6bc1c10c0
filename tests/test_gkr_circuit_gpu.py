"""GPU tests of caller-defined GKR circuits (gm_gkr_circuit_witness_create*, gm_gkr_witness_claims, gm_dense_evaluate,
gm_gkr_verify(_tr), gm_gkr_witness_layers): the two built-in circuits restated as layer lists (built-in ids and programs) are
bit-identical to their own builders and provers; random program circuits match the oracle's SimpleGKR; a proof under merlin
verifies and closes against the input columns."""
import ctypes as C

import numpy as np
import pytest

from gkr_msm_amd import codec, ffi, harness as H
from pyref import algfn as A
from pyref import field as F
from pyref import gkr as G
from pyref import polys as PL

import gkr_circuit_common as GC
from test_fn_program_gpu import builtin_prog, rand_limbs, rand_vecvec

pytestmark = pytest.mark.gpu

P = F.P


# ---------------------------------------------------------------------------------------------- the built-in circuits as lists
def fn_of(programs, *segs):
    """gm_fn of built-in ids, or of the same functions as programs (BUILTIN_TERMS of test_fn_program_gpu)"""
    names = {1: "AFF_L1", 2: "AFF_L2", 3: "AFF_L3", 4: "PROJ_L1", 5: "PROJ_L2", 6: "PROJ_L3", 7: "TRI_L1", 9: "BITCHECK"}
    if programs:
        segs = [(builtin_prog(names[p]).id, c) for p, c in segs]
    return ffi.make_fn(*segs)


def bintree_spec(num_adds, bitcheck, programs=False):
    """bintree_add.rs:247-375 as a layer list (gkr_layers.hpp bintree_layers)"""
    spec = []
    for i in range(num_adds):
        for step in range(3):
            prim = (1 + step) if i == 0 else (4 + step)
            if i == 0 and step == 0 and bitcheck:
                spec.append(("map", fn_of(programs, (1, 1), (9, 2))))
                spec.append(("zerocheck",))
            else:
                spec.append(("map", fn_of(programs, (prim, 1))))
        if i != num_adds - 1:
            spec.append(("split", False, 0, 3))
    return spec


def triangle_spec(num_vars, hi, programs=False):
    """triangle_add.rs:173-232 as a layer list (gkr_layers.hpp triangle_layers)"""
    spec = []
    n = num_vars - hi
    for l in range(n + 1):
        spec.append(("map", fn_of(programs, (7, 1), (4, l))))
        spec.append(("map", fn_of(programs, (5, l + 3))))
        spec.append(("map", fn_of(programs, (6, l + 3))))
        if l < n:
            spec.append(("split", True, hi, 3))
    return spec


def spec_key(spec):
    return [(l[0],) + ((l[1].nseg, tuple(l[1].prim[:l[1].nseg]), tuple(l[1].count[:l[1].nseg])) if l[0] == "map" else tuple(l[1:]))
            for l in spec]


def raw_output(w):
    n, nv = C.c_uint32(), C.c_uint32()
    ffi.check(w.L.gm_gkr_witness_output(w.h, None, 0, C.byref(n), C.byref(nv)))
    ptrs = (C.c_void_p * n.value)()
    ffi.check(w.L.gm_gkr_witness_output(w.h, ptrs, n.value, C.byref(n), C.byref(nv)))
    return [H.read_dev(ptrs[i], 32 << nv.value).copy() for i in range(n.value)], nv.value


def bintree_input(seed, row_log, col_log, bitcheck, mode="rows"):
    """a VecVec of 4 (or 6: + two Boolean columns with zero pads) polynomials of random field elements"""
    rng = F.SplitMix64(seed)
    k = 6 if bitcheck else 4
    py, _ = rand_vecvec(rng, 4, row_log, col_log, mode)
    data = [p.data for p in py]
    rpad, cpad = [p.row_pad for p in py], [p.col_pad for p in py]
    if bitcheck:
        for _ in range(2):
            data.append([[rng.next_bits(1) for _ in r] for r in data[0]])
            rpad.append(0)
            cpad.append(0)
    pys = [PL.VecVec(data[c], rpad[c], cpad[c], row_log, col_log) for c in range(k)]
    return pys, H.VV.from_host(data, rpad, cpad, row_log, col_log)


def check_same(a, b, point, evs, tape):
    oa, nva = raw_output(a)
    ob, nvb = raw_output(b)
    assert nva == nvb and len(oa) == len(ob) and all(np.array_equal(x, y) for x, y in zip(oa, ob))
    ra, rb = a.prove(point, evs, tape), b.prove(point, evs, tape)
    assert ra["msgs"] == rb["msgs"] and ra["point"] == rb["point"] and ra["evs"] == rb["evs"]
    assert ra["tape_used"] == rb["tape_used"] and ra["rounds"] == rb["rounds"]
    return ra


# (row_logsize of the VecVec input, col_logsize, num_adds): the third crosses from VecVec to dense (row_logsize + 1 = 4 < 5 adds)
BINTREE_SIZES = [(2, 1, 2), (4, 3, 3), (3, 2, 5), (7, 5, 4)]


@pytest.mark.parametrize("bitcheck", [False, True])
@pytest.mark.parametrize("row_log,col_log,adds", BINTREE_SIZES)
def test_bintree_restated(row_log, col_log, adds, bitcheck):
    """bintree_layers as a gm_gkr_layer list with built-in ids, and with every function a program: outputs and proofs bit-identical
    to gm_bintree_witness_create + gm_gkr_prove; gm_gkr_witness_layers of the built-in witness is the same list"""
    _, vv = bintree_input(700 + row_log * 10 + adds, row_log, col_log, bitcheck)
    ref = H.GkrWitness.bintree(vv, adds, bitcheck)
    spec = bintree_spec(adds, bitcheck)
    got_spec, ic, iv = H.gkr_witness_layers(ref)
    assert spec_key(got_spec) == spec_key(spec) and (ic, iv) == (6 if bitcheck else 4, row_log + col_log)
    circ = H.GkrCircuit.vecvec(spec, vv)
    out, nv = ref.output()
    rng = F.SplitMix64(71 + adds)
    point = [rng.next_fr() for _ in range(nv)]
    evs = [PL.evaluate_poly(o, point) for o in out]
    tape = [rng.next_bits(128) for _ in range(4000)]
    r = check_same(ref, circ, point, evs, tape)
    progs = H.GkrCircuit.vecvec(bintree_spec(adds, bitcheck, programs=True), vv)
    check_same(ref, progs, point, evs, tape)
    # the built-in witness's own proof verifies through its layer list
    rc, v = H.gkr_verify(got_spec, ic, iv, point, evs, r["msgs"], tape)
    assert rc == 0, ffi.lib().gm_last_error().decode()
    assert v["point"] == r["point"] and v["evs"] == r["evs"]


@pytest.mark.parametrize("num_vars,hi", [(4, 2), (6, 3), (9, 5)])
def test_triangle_restated(num_vars, hi):
    rs = np.random.default_rng(num_vars)
    cols = [H.to_dev(rand_limbs(rs, 1 << num_vars)) for _ in range(12)]
    ref = H.GkrWitness.triangle(cols, num_vars, hi)
    spec = triangle_spec(num_vars, hi)
    got_spec, ic, iv = H.gkr_witness_layers(ref)
    assert spec_key(got_spec) == spec_key(spec) and (ic, iv) == (12, num_vars)
    out, nv = ref.output()
    rng = F.SplitMix64(81 + num_vars)
    point = [rng.next_fr() for _ in range(nv)]
    evs = [PL.evaluate_poly(o, point) for o in out]
    tape = [rng.next_bits(128) for _ in range(4000)]
    r = check_same(ref, H.GkrCircuit.dense(spec, cols, num_vars), point, evs, tape)
    check_same(ref, H.GkrCircuit.dense(triangle_spec(num_vars, hi, programs=True), cols, num_vars), point, evs, tape)
    rc, v = H.gkr_verify(got_spec, ic, iv, point, evs, r["msgs"], tape)
    assert rc == 0, ffi.lib().gm_last_error().decode()
    assert v["evs"] == r["evs"] == [PL.evaluate_poly(c, r["point"]) for c in H.cols_to_host(cols)]


# ---------------------------------------------------------------------------------------------- random program circuits
def oracle_build_vv(pyspec, polys):
    """the builder over a VecVec input in the oracle: map, split (LO(0); to dense at one row variable), zero check"""
    layers, advices = [], []
    kind, cur = "VV", list(polys)
    nv = polys[0].row_logsize + polys[0].col_logsize
    for l in pyspec:
        if l[0] == "map":
            if kind == "VV":
                layers.append(("vecvec", l[1], nv, cur[0].col_logsize)); advices.append(("VV", cur))
                cur = PL.vecvec_map(cur, l[1])
            else:
                layers.append(("dense", l[1], nv)); advices.append(("D", cur))
                cur = PL.dense_algfn_map(cur, l[1])
        elif l[0] == "split":
            idx = PL.HI(l[2]) if l[1] else PL.LO(l[2])
            layers.append(("split", idx, l[3])); advices.append(G.EMPTY)
            if kind == "VV":
                if cur[0].row_logsize == 1:
                    kind, cur = "D", PL.vecvec_map_split_to_dense(cur, A.IdAlgFn(len(cur)), idx, l[3])
                else:
                    cur = PL.vecvec_map_split(cur, A.IdAlgFn(len(cur)), idx, l[3])
            else:
                cur = PL.dense_algfn_map_split(cur, A.IdAlgFn(len(cur)), idx, l[3])
            nv -= 1
        else:
            layers.append(("zerocheck",)); advices.append(G.EMPTY)
            cur = cur[:-2]
    out = [p.to_dense() for p in cur] if kind == "VV" else cur
    return layers, advices, out


def fuse_check(spec):
    return sum(1 for a, b in zip(spec, spec[1:]) if a[0] == "map" and b[0] == "split"), sum(1 for l in spec if l[0] == "split")


def run_random(seed, vecvec):
    rng = F.SplitMix64(seed)
    if vecvec:
        row, col = 2 + rng.next_bits(64) % 3, 1 + rng.next_bits(64) % 3
        in_cols = 1 + rng.next_bits(64) % 4
        py, vv = rand_vecvec(rng, in_cols, row, col, ["full", "rows", "short"][seed % 3])
        nv = row + col
        spec, pyspec, progs = GC.random_circuit(rng, in_cols, nv, 4 + rng.next_bits(64) % 6, vecvec_rows=row, progs_only=True)
        layers, advices, out = oracle_build_vv(pyspec, py)
        w = H.GkrCircuit.vecvec(spec, vv)
        in_dense = [p.to_dense() for p in py]
    else:
        nv = 3 + rng.next_bits(64) % 5
        in_cols = 1 + rng.next_bits(64) % 6
        cols = [[rng.next_fr() for _ in range(1 << nv)] for _ in range(in_cols)]
        spec, pyspec, progs = GC.random_circuit(rng, in_cols, nv, 4 + rng.next_bits(64) % 8, progs_only=True)
        layers, advices, out = GC.oracle_build(pyspec, cols)
        w = H.GkrCircuit.dense(spec, H.cols_to_dev(cols), nv)
        in_dense = cols
    got, onv = w.output()
    assert got == out
    point = [rng.next_fr() for _ in range(onv)]
    evs = [PL.evaluate_poly(o, point) for o in out]
    assert H.gkr_witness_claims(w, point) == evs
    tape = [rng.next_bits(128) for _ in range(4000)]
    res = w.prove(point, evs, tape)
    msgs, fpt, fev, used = GC.oracle_prove(layers, advices, point, evs, tape)
    assert res["msgs"] == msgs and res["point"] == fpt and res["evs"] == fev and res["tape_used"] == used
    assert fev == [PL.evaluate_poly(c, fpt) for c in in_dense]
    rc, v = H.gkr_verify(spec, in_cols, nv, point, evs, res["msgs"], tape)
    assert rc == 0 and v["evs"] == fev
    return spec


@pytest.mark.parametrize("seed", list(range(10)))
def test_random_dense_circuits_vs_oracle(seed):
    run_random(500 + seed, vecvec=False)


@pytest.mark.parametrize("seed", list(range(8)))
def test_random_vecvec_circuits_vs_oracle(seed):
    run_random(600 + seed, vecvec=True)


def test_long_map_chain_fused_and_unfused():
    """ten maps in a row; map + split (fused); split after a split and after a zero check (identity map-splits); HI and LO"""
    rng = F.SplitMix64(42)
    nv, k = 7, 3
    progs = [GC.Prog(k, k, GC.rand_terms(rng, k, k)) for _ in range(10)]
    zc = GC.Prog(12, 14, GC.rand_terms(rng, 12, 14, 2))
    l2 = builtin_prog("AFF_L2")
    tail = [("split", False, 2, 1), ("split", True, 1, 3), ("map", ffi.make_fn((l2.id, 4))), ("map", zc.fn()), ("zerocheck",),
            ("split", True, 0, 4)]
    spec = [("map", p.fn()) for p in progs] + tail
    pyspec = [("map", p.py) for p in progs] + [l if l[0] != "map" else None for l in tail]
    pyspec[12], pyspec[13] = ("map", A.RepeatedAlgFn(l2.py, 4)), ("map", zc.py)
    assert fuse_check(spec) == (1, 3)
    cols = [[rng.next_fr() for _ in range(1 << nv)] for _ in range(k)]
    layers, advices, out = GC.oracle_build(pyspec, cols)
    w = H.GkrCircuit.dense(spec, H.cols_to_dev(cols), nv)
    got, onv = w.output()
    assert got == out and onv == nv - 3 and len(out) == 24
    point = [rng.next_fr() for _ in range(onv)]
    evs = [PL.evaluate_poly(o, point) for o in out]
    tape = [rng.next_bits(128) for _ in range(2000)]
    res = w.prove(point, evs, tape)
    msgs, fpt, fev, used = GC.oracle_prove(layers, advices, point, evs, tape)
    assert res["msgs"] == msgs and res["point"] == fpt and res["evs"] == fev


def test_vecvec_split_rules_and_zerocheck_pads():
    """on VecVec input only LO(0) splits (the verifier, which sees dense shapes, accepts what the builder refuses); a zero check
    covers the pads"""
    rng = F.SplitMix64(9)
    py, vv = rand_vecvec(rng, 2, 3, 2, "rows")
    p = GC.Prog(2, 2, GC.rand_terms(rng, 2, 2))
    for bad in ([("split", False, 1, 2)], [("split", True, 0, 2)], [("map", p.fn()), ("split", True, 4, 1)]):
        with pytest.raises(ffi.GmError, match="LO\\(0\\)"):
            H.GkrCircuit.vecvec(bad, vv)
        assert H.gkr_verify(bad, 2, 5, [0] * 8, [0] * 8, [], [0] * 8)[0] != GC.INVALID
    # identity on two columns + two zero outputs whose pads are f(pads) = 0: accepted; zero check on raw input columns with pads != 0
    z = GC.Prog(2, 4, [(1, 0, (0, 0)), (1, 1, (1, 1))])
    w = H.GkrCircuit.vecvec([("map", z.fn()), ("zerocheck",)], vv)
    assert len(w.output()[0]) == 2
    zero_rows = [[[0] * len(r) for r in py[0].data]] * 2
    vvz = H.VV.from_host([p_.data for p_ in py] + zero_rows, [p_.row_pad for p_ in py] + [0, 5], [p_.col_pad for p_ in py] + [0, 0], 3, 2)
    ident = GC.Prog(4, 4, [(1, o, (o, o)) for o in range(4)])
    with pytest.raises(ffi.GmError, match="pad"):
        H.GkrCircuit.vecvec([("map", ident.fn()), ("zerocheck",)], vvz)


# ---------------------------------------------------------------------------------------------- ZEROCHECK, lifetime
def test_zerocheck_refuses_one_nonzero_cell():
    rs = np.random.default_rng(5)
    nv = 12
    p = GC.Prog(2, 4, [(1, 0, (0, 1)), (1, 1, (1, 1))])   # outputs 2, 3 are zero
    ident = GC.Prog(4, 4, [(1, o, (o, o)) for o in range(4)])
    base = [H.to_dev(rand_limbs(rs, 1 << nv)) for _ in range(2)]
    w = H.GkrCircuit.dense([("map", p.fn()), ("zerocheck",)], base, nv)
    assert len(w.output()[0]) == 2
    for col, cell in ((2, 0), (3, (1 << nv) - 1), (2, 1234)):
        cols = base + [H.to_dev(np.zeros(((1 << nv), 4), dtype=np.uint64)) for _ in range(2)]
        one = codec.to_mont_limbs([1])
        cols[col].view(-1)[4 * cell:4 * cell + 4] = H.to_dev(one).view(-1)
        with pytest.raises(ffi.GmError, match="ZEROCHECK"):
            H.GkrCircuit.dense([("map", ident.fn()), ("zerocheck",)], cols, nv)


def test_program_lifetime():
    rs = np.random.default_rng(6)
    p = GC.Prog(2, 2, GC.rand_terms(F.SplitMix64(6), 2, 2))
    cols = [H.to_dev(rand_limbs(rs, 1 << 6)) for _ in range(2)]
    w = H.GkrCircuit.dense([("map", p.fn()), ("split", False, 0, 1), ("map", ffi.make_fn((p.id, 2)))], cols, 6)
    assert ffi.lib().gm_fn_program_destroy(p.id) == GC.STATE
    w.close()
    assert ffi.lib().gm_fn_program_destroy(p.id) == 0


# ---------------------------------------------------------------------------------------------- gm_dense_evaluate
def host_fold(col, point):
    cur = list(col)
    for r in reversed(point):
        cur = [(cur[2 * i] + r * (cur[2 * i + 1] - cur[2 * i])) % P for i in range(len(cur) // 2)]
    return cur[0]


@pytest.mark.parametrize("num_vars", list(range(0, 13)))
def test_dense_evaluate_vs_host_fold(num_vars):
    rng = F.SplitMix64(300 + num_vars)
    k = 1 + num_vars % 8
    cols = [[rng.next_fr() for _ in range(1 << num_vars)] for _ in range(k)]
    point = [rng.next_fr() for _ in range(num_vars)]
    d = H.cols_to_dev(cols)
    assert H.dense_evaluate(d, num_vars, point) == [host_fold(c, point) for c in cols]
    # a Boolean point picks one element: point[0] is the most significant bit of the index
    idx = (rng.next_bits(64) % (1 << num_vars)) if num_vars else 0
    bpt = [(idx >> (num_vars - 1 - i)) & 1 for i in range(num_vars)]
    assert H.dense_evaluate(d, num_vars, bpt) == [c[idx] for c in cols]


def test_dense_evaluate_2_24_bit_exact_vs_bind_chain():
    rs = np.random.default_rng(24)
    nv = 24
    cols = [H.to_dev(rand_limbs(rs, 1 << nv)) for _ in range(2)]
    rng = F.SplitMix64(24)
    point = [rng.next_fr() for _ in range(nv)]
    evs = np.zeros((2, 4), dtype=np.uint64)
    pa = H.fr_arg(point)
    ffi.check(ffi.lib().gm_dense_evaluate(H.ptr_array(cols), 2, nv, pa.ctypes.data, evs.ctypes.data, H.cur_stream()))
    cur = cols
    for r in reversed(point):
        cur = H.dense_bind(cur, r)
    chain = np.stack([H.to_host(c).reshape(-1, 4)[0] for c in cur])
    assert np.array_equal(evs, chain)


# ---------------------------------------------------------------------------------------------- end to end under merlin
@pytest.mark.parametrize("vecvec", [False, True])
def test_merlin_end_to_end(vecvec):
    rng = F.SplitMix64(77 + vecvec)
    if vecvec:
        py, vv = rand_vecvec(rng, 3, 4, 3, "rows")
        nv, k = 7, 3
        spec, _, progs = GC.random_circuit(rng, k, nv, 7, vecvec_rows=4, progs_only=True)
        w = H.GkrCircuit.vecvec(spec, vv)
        dense_in = [H.dev_empty((1 << nv) * 4) for _ in range(k)]
        ffi.check(ffi.lib().gm_vv_to_dense(vv.h, H.ptr_array(dense_in), H.cur_stream()))
    else:
        nv, k = 10, 4
        rs = np.random.default_rng(77)
        dense_in = [H.to_dev(rand_limbs(rs, 1 << nv)) for _ in range(k)]
        spec, _, progs = GC.random_circuit(rng, k, nv, 8, progs_only=False)
        w = H.GkrCircuit.dense(spec, dense_in, nv)
    out, onv = w.output()
    point = [rng.next_fr() for _ in range(onv)]
    evs = H.gkr_witness_claims(w, point)
    assert evs == [host_fold(o, point) for o in out]
    tr = H.MerlinTranscript()
    res = H.gkr_prove_tr(w, point, evs, tr)
    proof = tr.proof()
    tr.close()
    rc, v = H.gkr_verify_merlin(spec, k, nv, point, evs, proof)
    assert rc == 0, ffi.lib().gm_last_error().decode()
    assert v["unread"] == 0 and v["point"] == res["point"] and v["evs"] == res["evs"]
    # the loop closes: the verifier's claims are the input columns at its point
    assert H.dense_evaluate(dense_in, nv, v["point"]) == v["evs"]
    bad = bytearray(proof)
    bad[len(bad) // 3] ^= 1
    assert H.gkr_verify_merlin(spec, k, nv, point, evs, bytes(bad))[0] == GC.VERIFY
