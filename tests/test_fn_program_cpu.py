"""CPU tests of caller-defined AlgFns (gm_fn_program_create): validation, gm_fn_shape and gm_fn_host against a Python
evaluation of the same terms, lifetime.  gm_fn_program_create is host only: no GPU is touched here."""
import ctypes as C

import numpy as np
import pytest

from gkr_msm_amd import codec, ffi, harness as H
from pyref import field as F

P = F.P
INVALID, STATE = 1, 4


def create_rc(n_ins, n_outs, deg, terms, raw=None):
    arr = H.fn_terms(terms)
    if raw:
        raw(arr)
    pid = C.c_int32(-1)
    rc = ffi.lib().gm_fn_program_create(n_ins, n_outs, deg, arr, len(terms), C.byref(pid))
    return rc, pid.value


def py_eval(terms, n_outs, args):
    out = [0] * n_outs
    for coef, o, factors in terms:
        v = coef % P
        for f in factors:
            v = v * args[f] % P
        out[o] = (out[o] + v) % P
    return out


def host_eval(fn, rows, n_outs):
    n = len(rows)
    a = codec.to_mont_limbs([x for r in rows for x in r])
    o = np.zeros((n * n_outs, 4), dtype=np.uint64)
    ffi.check(ffi.lib().gm_fn_host(C.byref(fn), a.ctypes.data, o.ctypes.data, n))
    flat = codec.from_mont_limbs(o)
    return [flat[i * n_outs:(i + 1) * n_outs] for i in range(n)]


def shape(fn):
    ni, no, dg = C.c_int32(), C.c_int32(), C.c_int32()
    rc = ffi.lib().gm_fn_shape(C.byref(fn), C.byref(ni), C.byref(no), C.byref(dg))
    return rc, (ni.value, no.value, dg.value)


def last_error():
    return ffi.lib().gm_last_error().decode()


FOO = [(1, 0, (0,)), (1, 0, (1,)), (1, 1, (1,)), (1, 1, (2,))]   # foo = (i0 + i1, i1 + i2)  (src/utils.rs:392-520)


def test_validation_errors():
    def bad_reserved(a):
        a[0].reserved = 1

    cases = [
        ((0, 1, 1, [(1, 0, ())]), "n_ins"),
        ((65, 1, 1, [(1, 0, (0,))]), "n_ins"),
        ((1, 0, 1, [(1, 0, (0,))]), "n_outs"),
        ((1, 65, 1, [(1, 0, (0,))]), "n_outs"),
        ((2, 1, 5, [(1, 0, (0,))]), "GM_FN_PROG_MAX_DEG"),
        ((2, 1, 1, [(1, 1, (0,))]), "out of range"),            # out >= n_outs
        ((2, 1, 1, [(1, 0, (2,))]), "out of range"),            # factor >= n_ins
        ((2, 1, 1, [(1, 0, (0, 1))]), "declared degree"),       # n_factors > deg
        ((2, 1, 4, [(1, 0, (0, 1, 1, 0))] + [(1, 0, ())] * 1024), "GM_FN_PROG_MAX_TERMS"),
    ]
    for (ni, no, dg, terms), msg in cases:
        rc, _ = create_rc(ni, no, dg, terms)
        assert rc == INVALID and msg in last_error(), (ni, no, dg, last_error())
    rc, _ = create_rc(2, 1, 1, [(1, 0, (0,))], raw=bad_reserved)
    assert rc == INVALID and "reserved" in last_error()

    def five_factors(a):
        a[0].n_factors = 5
    rc, _ = create_rc(2, 1, 4, [(1, 0, (0,))], raw=five_factors)
    assert rc == INVALID and "GM_FN_PROG_MAX_DEG" in last_error()
    # limits that hold: 64 x 64, 1024 terms, 0 terms (the zero function)
    for ni, no, dg, terms in [(64, 64, 4, [(1, 63, (63, 0, 63, 1))]), (1, 1, 0, []), (3, 2, 2, [(7, 1, (2, 2))] * 1024)]:
        rc, pid = create_rc(ni, no, dg, terms)
        assert rc == 0 and pid >= ffi.FN_PROG_BASE, last_error()
        H.destroy_program(pid)


def test_shape_single_repeated_stacked():
    p = H.make_program(3, 2, 1, FOO)
    q = H.make_program(2, 3, 4, [(5, 2, (0, 0, 1, 1)), (1, 0, ())])
    try:
        assert shape(ffi.make_fn((p, 1))) == (0, (3, 2, 1))
        assert shape(ffi.make_fn((p, 5))) == (0, (15, 10, 1))
        assert shape(ffi.make_fn((p, 1), (q, 3))) == (0, (9, 11, 4))
        assert shape(ffi.make_fn((q, 0), (p, 2))) == (0, (6, 4, 1))   # a segment of count 0 adds nothing, its degree neither
        # the whole function must fit 64 columns
        w = H.make_program(1, 1, 1, [(1, 0, (0,))])
        assert shape(ffi.make_fn((w, 64)))[0] == 0
        assert shape(ffi.make_fn((w, 65)))[0] == INVALID and "too wide" in last_error()
        H.destroy_program(w)
    finally:
        H.destroy_program(p)
        H.destroy_program(q)


def test_host_eval_against_python():
    rng = F.SplitMix64(77)
    terms_p = [
        (0, 0, (0, 1)),                    # coefficient 0
        (1, 0, (2,)),                      # coefficient 1
        (P - 1, 1, (0, 0, 0)),             # p - 1, x^3 as a repeated factor
        (rng.next_fr(), 1, (1, 1, 1, 1)),  # x^4
        (rng.next_fr(), 2, ()),            # a constant term
        (3, 2, (0, 2)), (3, 2, (0, 2)),    # duplicate terms add up
        (rng.next_fr(), 4, (2, 1, 0, 1)),  # output 3 has no terms
    ]
    p = H.make_program(3, 5, 4, terms_p)
    terms_q = [(rng.next_fr(), 0, (0, 1)), (P - 1, 1, (1,)), (2, 1, ())]
    q = H.make_program(2, 2, 2, terms_q)
    try:
        rows = [[rng.next_fr() for _ in range(3)] for _ in range(20)] + [[0, 0, 0], [1, 1, 1], [P - 1, P - 1, P - 1]]
        assert host_eval(ffi.make_fn((p, 1)), rows, 5) == [py_eval(terms_p, 5, r) for r in rows]
        for r in host_eval(ffi.make_fn((p, 1)), rows, 5):
            assert r[3] == 0
        # Stacked(P, Repeated(Q, 3))
        rows = [[rng.next_fr() for _ in range(9)] for _ in range(10)]
        exp = [py_eval(terms_p, 5, r[:3]) + py_eval(terms_q, 2, r[3:5]) + py_eval(terms_q, 2, r[5:7]) + py_eval(terms_q, 2, r[7:9])
               for r in rows]
        assert host_eval(ffi.make_fn((p, 1), (q, 3)), rows, 11) == exp
        # the zero function
        z = H.make_program(2, 3, 1, [])
        assert host_eval(ffi.make_fn((z, 2)), [[5, 6, 7, 8]], 6) == [[0] * 6]
        H.destroy_program(z)
    finally:
        H.destroy_program(p)
        H.destroy_program(q)


def test_coefficients_are_reduced():
    # a coefficient given as any 256-bit word is the field element it represents (Montgomery form, reduced)
    def raw_coef(a):
        for l in range(4):
            a[0].coef[l] = 0xFFFFFFFFFFFFFFFF
    rc, pid = create_rc(1, 1, 1, [(1, 0, (0,))], raw=raw_coef)
    assert rc == 0
    try:
        rinv = pow(codec.R, -1, P)
        c = ((1 << 256) - 1) * rinv % P
        assert host_eval(ffi.make_fn((pid, 1)), [[5]], 1) == [[c * 5 % P]]
    finally:
        H.destroy_program(pid)


def test_destroy_twice_unknown_and_mixed():
    L = ffi.lib()
    p = H.make_program(3, 2, 1, FOO)
    q = H.make_program(3, 2, 1, FOO)
    assert q > p   # ids are not reused
    mixed = ffi.make_fn((p, 1), (ffi.FN_PROJ_L2, 1))
    assert shape(mixed)[0] == INVALID and "mixed built-in / program functions are not supported" in last_error()
    a = codec.to_mont_limbs([1] * 7)
    o = np.zeros((6, 4), dtype=np.uint64)
    assert L.gm_fn_host(C.byref(mixed), a.ctypes.data, o.ctypes.data, 1) == INVALID
    assert L.gm_fn_program_destroy(p) == 0
    assert L.gm_fn_program_destroy(p) == INVALID and "unknown or destroyed" in last_error()
    assert shape(ffi.make_fn((p, 1)))[0] == INVALID
    assert L.gm_fn_host(C.byref(ffi.make_fn((p, 1))), a.ctypes.data, o.ctypes.data, 1) == INVALID
    assert L.gm_fn_program_destroy(ffi.FN_PROG_BASE + 1000000) == INVALID
    r = H.make_program(3, 2, 1, FOO)
    assert r > q
    H.destroy_program(q)
    H.destroy_program(r)


def test_builtin_ids_unchanged():
    # built-in descriptors keep their shapes (ids < 64 never take the program path)
    assert shape(ffi.make_fn((ffi.FN_PROJ_L1, 2)))[1] == (12, 8, 2)
    assert shape(ffi.make_fn((ffi.FN_ID, 3)))[1] == (3, 3, 1)
