"""CPU tests of caller-defined GKR circuits: the shape rules (one host pass, refused with GM_ERR_INVALID before anything else) and
gm_gkr_verify over proofs of random small circuits made by the oracle's SimpleGKR prover.  The verifier is host code: no GPU."""
import pytest

from gkr_msm_amd import ffi, harness as H
from pyref import field as F
from pyref import polys as PL

import gkr_circuit_common as GC

P = F.P


def rc_of(spec, in_cols, nv, n_out_cols=8, out_vars=None):
    out_vars = nv if out_vars is None else out_vars
    rc, _ = H.gkr_verify(spec, in_cols, nv, [1] * max(out_vars, 1), [1] * n_out_cols, [], [3] * 64)
    return rc


def last_error():
    return ffi.lib().gm_last_error().decode()


@pytest.fixture(scope="module")
def progs():
    rng = F.SplitMix64(11)
    d = dict(p3x2=GC.Prog(3, 2, GC.rand_terms(rng, 3, 2)), p2x4=GC.Prog(2, 4, GC.rand_terms(rng, 2, 4)))
    d["deg1"] = GC.Prog(3, 2, [(5, 0, (1,)), (7, 1, (0,))], deg=1)
    d["deg3"] = GC.Prog(3, 2, [(5, 0, (1, 2, 0)), (7, 1, (0,))], deg=3)
    return d


def test_shape_rules_refused(progs):
    L = ffi.lib()
    m = lambda f: ("map", f)
    ok = [m(progs["p3x2"].fn()), m(progs["p2x4"].fn())]
    assert rc_of(ok, 3, 4, n_out_cols=4) == GC.VERIFY, last_error()   # a valid shape: the empty proof is then rejected
    # wrong n_ins
    assert rc_of([m(progs["p2x4"].fn())], 3, 4) == GC.INVALID
    assert "layer 0" in last_error() and "inputs" in last_error()
    assert rc_of([m(progs["p3x2"].fn()), m(progs["p3x2"].fn())], 3, 4) == GC.INVALID
    assert "layer 1" in last_error()
    # degree 1 and 3 programs; a built-in of degree 1 (Id)
    assert rc_of([m(progs["deg1"].fn())], 3, 4) == GC.INVALID and "degree 1" in last_error()
    assert rc_of([m(progs["deg3"].fn())], 3, 4) == GC.INVALID and "degree 3" in last_error()
    assert rc_of([m(ffi.make_fn((ffi.FN_ID, 3)))], 3, 4) == GC.INVALID and "degree" in last_error()
    # bundle not dividing the columns; bundle 0
    assert rc_of([m(progs["p3x2"].fn()), ("split", False, 0, 3)], 3, 4) == GC.INVALID and "bundle" in last_error()
    assert rc_of([("split", False, 0, 0)], 3, 4) == GC.INVALID
    # split with no variable left; index outside the variables
    assert rc_of([("split", True, 0, 3), ("split", True, 0, 6)], 3, 1) == GC.INVALID and "no variable" in last_error()
    assert rc_of([("split", False, 4, 3)], 3, 4) == GC.INVALID and "index" in last_error()
    # ZEROCHECK on fewer than two columns
    assert rc_of(ok + [("zerocheck",), ("zerocheck",), ("zerocheck",)], 3, 4) == GC.INVALID and "layer 4 (ZEROCHECK)" in last_error()
    assert rc_of([("zerocheck",)], 1, 4) == GC.INVALID and "ZEROCHECK" in last_error()
    # mixed built-in / program ids in one gm_fn
    assert rc_of([m(ffi.make_fn((ffi.FN_AFF_L2, 1), (progs["p3x2"].id, 1)))], 6, 4) == GC.INVALID and "mixed" in last_error()
    # unknown and destroyed program ids
    assert rc_of([m(ffi.make_fn((ffi.FN_PROG_BASE + 999999, 1)))], 3, 4) == GC.INVALID and "unknown" in last_error()
    gone = GC.Prog(3, 2, GC.rand_terms(F.SplitMix64(3), 3, 2))
    H.destroy_program(gone.id)
    assert rc_of([m(gone.fn())], 3, 4) == GC.INVALID and "destroyed" in last_error()
    # non-zero reserved; unknown kind
    arr = H.gkr_layers(ok)
    arr[1].reserved = 1
    assert L.gm_gkr_verify(arr, 2, 3, 4, None, None, None, 0, None, 0, None, None, None, None, None) == GC.INVALID
    assert "layer 1" in last_error() and "reserved" in last_error()
    arr = H.gkr_layers(ok)
    arr[0].kind = 7
    assert L.gm_gkr_verify(arr, 2, 3, 4, None, None, None, 0, None, 0, None, None, None, None, None) == GC.INVALID
    # no layers at all
    assert L.gm_gkr_verify(arr, 0, 3, 4, None, None, None, 0, None, 0, None, None, None, None, None) == GC.INVALID


def circuit_case(seed, with_builtins=True):
    rng = F.SplitMix64(seed)
    nv = 2 + rng.next_bits(64) % 5
    in_cols = [1, 2, 3, 4, 6][rng.next_bits(64) % 5]
    spec, pyspec, progs = GC.random_circuit(rng, in_cols, nv, 3 + rng.next_bits(64) % 5, progs_only=not with_builtins)
    cols = [[rng.next_fr() for _ in range(1 << nv)] for _ in range(in_cols)]
    layers, advices, out = GC.oracle_build(pyspec, cols)
    out_nv = PL.log2_exact(len(out[0]))
    point = [rng.next_fr() for _ in range(out_nv)]
    evs = [PL.evaluate_poly(c, point) for c in out]
    tape = [rng.next_bits(128) for _ in range(4096)]
    msgs, fpt, fev, used = GC.oracle_prove(layers, advices, point, evs, tape)
    return dict(spec=spec, progs=progs, in_cols=in_cols, nv=nv, point=point, evs=evs, tape=tape, msgs=msgs, fpt=fpt, fev=fev,
                used=used, cols=cols)


@pytest.mark.parametrize("seed", list(range(12)))
def test_verify_accepts_oracle_proofs_and_rejects_tampering(seed):
    c = circuit_case(100 + seed, with_builtins=seed % 3 != 0)
    rc, got = H.gkr_verify(c["spec"], c["in_cols"], c["nv"], c["point"], c["evs"], c["msgs"], c["tape"])
    assert rc == 0, last_error()
    assert got["point"] == c["fpt"] and got["evs"] == c["fev"] and got["tape_used"] == c["used"]
    # the final claims are claims about the input columns
    assert got["evs"] == [PL.evaluate_poly(col, got["point"]) for col in c["cols"]]
    if c["msgs"]:
        bad = list(c["msgs"])
        bad[0] = (bad[0] + 1) % P   # the first round polynomial
        assert H.gkr_verify(c["spec"], c["in_cols"], c["nv"], c["point"], c["evs"], bad, c["tape"])[0] == GC.VERIFY
        # any other message: rejected, or (an evaluation claim on an input the layer function ignores) a false claim on the input
        bad = list(c["msgs"])
        k = (seed * 7919) % len(bad)
        bad[k] = (bad[k] + 1) % P
        rc, got = H.gkr_verify(c["spec"], c["in_cols"], c["nv"], c["point"], c["evs"], bad, c["tape"])
        assert rc == GC.VERIFY or got["evs"] != [PL.evaluate_poly(col, got["point"]) for col in c["cols"]]
        assert H.gkr_verify(c["spec"], c["in_cols"], c["nv"], c["point"], c["evs"], c["msgs"][:-1], c["tape"])[0] == GC.VERIFY
    assert H.gkr_verify(c["spec"], c["in_cols"], c["nv"], c["point"], c["evs"], c["msgs"] + [1], c["tape"])[0] == GC.VERIFY
    wrong = list(c["evs"])
    wrong[0] = (wrong[0] + 1) % P
    if c["msgs"]:
        assert H.gkr_verify(c["spec"], c["in_cols"], c["nv"], c["point"], wrong, c["msgs"], c["tape"])[0] == GC.VERIFY
