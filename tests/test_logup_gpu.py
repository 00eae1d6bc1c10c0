"""GPU tests of the standalone GKR-logup: gm_logup_witness_create / gm_logup_prove(_tr) against the oracle's logup_make_witness and
logup_mainphase_prove (the reference's witness_gen_works and logup_maincycle_works, logup_mainphase.rs:252-338, at their literal
logsizes and around the tail-launch threshold), the library verifier over the device's proofs, a size no Python oracle reaches, the
refusals, and a lookup argument end to end with gm_logup_multiplicities / gm_logup_denominators."""
import os
import subprocess
import sys

import numpy as np
import pytest

from gkr_msm_amd import codec, ffi, harness as H
from pyref import field as F
from pyref import pushforward as PF

import logup_common as LC

pytestmark = pytest.mark.gpu
P = LC.P
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ids = lambda s: "-".join(map(str, s))


def last_error():
    return ffi.lib().gm_last_error().decode()


def torch_sync():
    H.torch_mod().cuda.synchronize()


def test_witness_gen_works():
    """witness_gen_works at its literal logsizes"""
    logsizes = [5, 5, 3, 3, 3, 3, 1, 0, 0, 0]
    inputs, total = LC.gen_inputs(logsizes, 501)
    nums, dens = LC.to_dev_cols(inputs)
    w = H.LogupWitness(logsizes, nums, dens)
    n, d = w.total()
    _, (on, od) = PF.logup_make_witness(logsizes, inputs)
    assert (n, d) == (on % P, od % P)
    assert d != 0 and total * d % P == n
    w.close()


@pytest.mark.parametrize("logsizes", LC.GPU_SHAPES, ids=ids)
def test_maincycle(logsizes):
    """logup_maincycle_works at its literal [5,5,3,3,3,3] and shapes with inputs joining the tree above, at and below every
    admissible tail threshold (2^8 .. 2^11): messages, claims, tape position and rounds identical to the oracle"""
    inputs, total = LC.gen_inputs(logsizes, 900 + 7 * sum(logsizes) + len(logsizes))
    tape = LC.tape_of(31 + sum(logsizes))
    o = LC.oracle_prove(logsizes, inputs, total, tape)
    nums, dens = LC.to_dev_cols(inputs)
    w = H.LogupWitness(logsizes, nums, dens)
    assert w.total() == (o["msgs"][0], o["msgs"][1])
    g = w.prove(total, tape)
    assert g["msgs"] == o["msgs"]
    assert LC.same_claims(g["claims"], o["claims"])
    assert g["tape_used"] == o["tape_used"] and g["rounds"] == LC.n_rounds(logsizes)
    rc, v = H.logup_verify(logsizes, total, g["msgs"], tape)
    assert rc == 0, last_error()
    assert LC.same_claims(v["claims"], g["claims"]) and v["tape_used"] == g["tape_used"]
    LC.check_claims_against_inputs(logsizes, g["claims"], nums, dens)
    g2 = w.prove(total, tape)   # the witness is not consumed
    assert g2["msgs"] == g["msgs"] and LC.same_claims(g2["claims"], g["claims"])
    w.close()


def test_maincycle_without_tail_launch():
    """the same set in a fresh child process with GM_LOGUP_NO_TAIL=1 (the switch is read once per process): the per-level path
    must match the oracle too"""
    env = dict(os.environ, GM_LOGUP_NO_TAIL="1")
    out = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-k", "test_maincycle and not without"],
                         env=env, cwd=ROOT, capture_output=True, text=True, timeout=900)
    if out.returncode < 0 or out.returncode in (134, 139):   # the device faulted: start nothing more on it
        pytest.exit("child process ended by signal (%d):\n%s" % (out.returncode, out.stderr[-3000:]), returncode=1)
    assert out.returncode == 0 and ("%d passed" % len(LC.GPU_SHAPES)) in out.stdout, out.stdout[-3000:] + out.stderr[-2000:]


@pytest.mark.parametrize("logsizes", [[5, 5, 3, 3, 3, 3], [11, 11, 10, 9, 4], [0, 0]], ids=ids)
def test_merlin_round_trip(logsizes):
    """gm_logup_prove_tr -> proof bytes -> gm_logup_verify_tr under the reference's label"""
    inputs, total = LC.gen_inputs(logsizes, 1234 + sum(logsizes))
    nums, dens = LC.to_dev_cols(inputs)
    w = H.LogupWitness(logsizes, nums, dens)
    tr = H.MerlinTranscript(b"awoo")
    g = w.prove_tr(total, tr)
    proof = tr.proof()
    rc, v = H.logup_verify_merlin(logsizes, total, proof, label=b"awoo")
    assert rc == 0, last_error()
    assert LC.same_claims(v["claims"], g["claims"]) and v["unread"] == 0
    LC.check_claims_against_inputs(logsizes, g["claims"], nums, dens)
    bad = bytearray(proof)
    bad[len(bad) // 2] ^= 1
    rc, _ = H.logup_verify_merlin(logsizes, total, bytes(bad), label=b"awoo")
    assert rc == LC.VERIFY
    w.close()
    tr.close()


def test_at_size():
    """[22, 22, 18, 8]: the pushforward's logsizes at x_logsize 18, y_logsize 5, d_logsize 8"""
    logsizes = [22, 22, 18, 8]
    nums, dens, total = LC.big_inputs(logsizes, 2024)
    w = H.LogupWitness(logsizes, nums, dens)
    n, d = w.total()
    assert d != 0 and total * d % P == n
    tape = LC.tape_of(99, 600)
    g = w.prove(total, tape)
    rc, v = H.logup_verify(logsizes, total, g["msgs"], tape)
    assert rc == 0, last_error()
    assert LC.same_claims(v["claims"], g["claims"]) and v["tape_used"] == g["tape_used"]
    assert g["rounds"] == LC.n_rounds(logsizes)
    LC.check_claims_against_inputs(logsizes, g["claims"], nums, dens)
    g2 = w.prove(total, tape)
    assert g2["msgs"] == g["msgs"]
    w.close()


def test_refusals():
    logsizes = [6, 6, 6, 6, 2]
    inputs, total = LC.gen_inputs(logsizes, 4242)
    nums, dens = LC.to_dev_cols(inputs)
    tape = LC.tape_of(5)
    w = H.LogupWitness(logsizes, nums, dens)
    # a wrong claim: GM_ERR_INVALID and nothing written to the transcript
    rc, _ = w.prove_rc((total + 1) % P, tape)
    assert rc == LC.INVALID and "claim" in last_error()
    live = H.LiveTranscript(lambda: None)
    with pytest.raises(ffi.GmError):
        w.prove_tr((total + 1) % P, live)
    assert live.writes == [] and live.requests == []
    assert w.prove(total, tape)["msgs"][:2] == list(w.total())   # still usable
    w.close()
    # destroy with no prove; the inputs are freed only after the destroy
    w = H.LogupWitness(logsizes, nums, dens)
    w.close()
    # one zero in a denominator column: the total denominator is the product of all of them
    n3, d3 = inputs[3]
    d3 = list(d3)
    d3[17] = 0
    bad_d = H.to_dev(H.fr_arg(d3))
    with pytest.raises(ffi.GmError) as e:
        H.LogupWitness(logsizes, nums, dens[:3] + [bad_d] + dens[4:])
    assert "denominator is zero" in str(e.value)
    # the shape rules are the verifier's
    with pytest.raises(ffi.GmError) as e:
        H.LogupWitness([6, 6, 2, 6], nums[:2] + [nums[4], nums[2]], dens[:2] + [dens[4], dens[2]])
    assert "non-increasing" in str(e.value)
    torch_sync()
    del nums, dens


def poly_eval(vals, point):
    cur = list(vals)
    for f in reversed(point):
        cur = [(cur[2 * i] + f * (cur[2 * i + 1] - cur[2 * i])) % P for i in range(len(cur) // 2)]
    return cur[0]


def test_lookup_end_to_end():
    """every row of (w_0, w_1) (2^14 rows) is a row of (t_0, t_1) (2^8 rows): multiplicities of the index column, lookup side
    (1, tau - v_i) cut into its two HI halves, table side (m_j, u_j - tau), logsizes [13, 13, 8], claimed sum 0"""
    torch = H.torch_mod()
    W, T, k = 14, 8, 2
    rng = F.SplitMix64(0x100c)
    table = [[rng.next_fr() for _ in range(1 << T)] for _ in range(k)]
    idx = np.random.default_rng(5).integers(0, 1 << T, size=1 << W, dtype=np.int64).astype(np.int32)
    looked = [[table[c][j] for j in idx] for c in range(k)]
    psi, tau = rng.next_fr(), rng.next_fr()
    d_idx = torch.from_numpy(idx).cuda()
    d_table = [H.to_dev(H.fr_arg(c)) for c in table]
    d_looked = [H.to_dev(H.fr_arg(c)).reshape(-1) for c in looked]

    d_m = H.logup_multiplicities(d_idx, 1 << W, 1 << T)
    m = codec.from_mont_limbs(H.to_host(d_m).reshape(-1, 4))
    assert m == [int(v) for v in np.bincount(idx, minlength=1 << T)]

    den_of = lambda cols, i: (tau - sum(pow(psi, c, P) * cols[c][i] for c in range(k))) % P
    d_den_w, d_ones = H.logup_denominators(d_looked, psi, tau, negate=False, ones=True)
    d_den_t, none = H.logup_denominators(d_table, psi, tau, negate=True)
    assert none is None
    den_w = codec.from_mont_limbs(H.to_host(d_den_w).reshape(-1, 4))
    den_t = codec.from_mont_limbs(H.to_host(d_den_t).reshape(-1, 4))
    assert den_w == [den_of(looked, i) for i in range(1 << W)]
    assert den_t == [(-den_of(table, j)) % P for j in range(1 << T)]
    assert codec.from_mont_limbs(H.to_host(d_ones).reshape(-1, 4)) == [1] * (1 << W)

    half = 4 << (W - 1)   # int64 words of one HI half
    logsizes = [W - 1, W - 1, T]
    nums = [d_ones[:half], d_ones[half:], d_m]
    dens = [d_den_w[:half], d_den_w[half:], d_den_t]
    w = H.LogupWitness(logsizes, nums, dens)
    n, d = w.total()
    assert n == 0 and d != 0
    tape = LC.tape_of(314)
    g = w.prove(0, tape)
    rc, v = H.logup_verify(logsizes, 0, g["msgs"], tape)
    assert rc == 0, last_error()
    assert LC.same_claims(v["claims"], g["claims"])
    # what the caller checks against its commitments: the claims are the inputs' evaluations
    (pt0, ev0), (pt1, ev1) = g["claims"]
    for h in range(2):   # the two halves of the lookup side: numerator 1, denominator tau - sum psi^k w_k at the point
        cols = H.dense_evaluate([c[h * half:(h + 1) * half] for c in d_looked], W - 1, pt0)
        assert ev0[2 * h] == 1
        assert ev0[2 * h + 1] == (tau - sum(pow(psi, c, P) * cols[c] for c in range(k))) % P
    cols = H.dense_evaluate(d_table, T, pt1)
    assert ev1[0] == poly_eval(m, pt1)
    assert ev1[1] == (sum(pow(psi, c, P) * cols[c] for c in range(k)) - tau) % P
    w.close()

    # one looked-up row changed to a row that is not in the table (index unchanged): the sum is no longer zero
    looked[0][4321] = (looked[0][4321] + 1) % P
    d_looked2 = [H.to_dev(H.fr_arg(looked[0])).reshape(-1), d_looked[1]]
    d_den_w2, _ = H.logup_denominators(d_looked2, psi, tau)
    w = H.LogupWitness(logsizes, nums, [d_den_w2[:half], d_den_w2[half:], d_den_t])
    n, d = w.total()
    assert n != 0 and d != 0
    rc, _ = w.prove_rc(0, tape)
    assert rc == LC.INVALID
    w.close()


def multiplicities_host(d_m):
    return codec.from_mont_limbs(H.to_host(d_m).reshape(-1, 4))


def test_multiplicities_paths():
    torch = H.torch_mod()
    g = np.random.default_rng(77)
    # the global-atomic path: uniform, then every index equal (all adds on one counter: counts must be exact)
    n, tl = 1 << 22, 1 << 20
    idx = g.integers(0, tl, size=n, dtype=np.int64).astype(np.int32)
    got = multiplicities_host(H.logup_multiplicities(torch.from_numpy(idx).cuda(), n, tl))
    assert got == [int(v) for v in np.bincount(idx, minlength=tl)]
    idx = np.full(n, 123457, dtype=np.int32)
    got = multiplicities_host(H.logup_multiplicities(torch.from_numpy(idx).cuda(), n, tl))
    assert got[123457] == n and sum(got) == n
    # both sides of the LDS limit: the same indices give the same counts
    n = (1 << 18) + 3   # not a multiple of the vector width
    idx = g.integers(0, 1 << 14, size=n, dtype=np.int64).astype(np.int32)
    d_idx = torch.from_numpy(idx).cuda()
    ref = [int(v) for v in np.bincount(idx, minlength=(1 << 14) + 1)]
    lds = multiplicities_host(H.logup_multiplicities(d_idx, n, 1 << 14))
    glob = multiplicities_host(H.logup_multiplicities(d_idx, n, (1 << 14) + 1))
    assert lds == ref[:1 << 14] and glob == ref
    # an index column that does not start on a 16-byte boundary
    got = multiplicities_host(H.logup_multiplicities(d_idx[1:], n - 1, 1 << 14))
    assert got == [int(v) for v in np.bincount(idx[1:], minlength=1 << 14)]
    # an out-of-range index on both paths; n = 0
    idx[n // 2] = 1 << 14
    d_idx = torch.from_numpy(idx).cuda()
    for tl in (1 << 14, 1 << 9):
        rc, _ = H.logup_multiplicities_rc(d_idx, n, tl)
        assert rc == LC.INVALID and "table_len" in last_error()
    idx[n // 2] = 1 << 21
    rc, _ = H.logup_multiplicities_rc(torch.from_numpy(idx).cuda(), n, 1 << 20)
    assert rc == LC.INVALID
    assert multiplicities_host(H.logup_multiplicities(d_idx, 0, 300)) == [0] * 300
