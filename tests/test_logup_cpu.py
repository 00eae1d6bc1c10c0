"""CPU tests of the standalone GKR-logup verifier (gm_logup_verify): the shape rules, proofs made by the oracle's
logup_mainphase_prove, and rejections.  The verifier is host code: no GPU."""
import pytest

from gkr_msm_amd import ffi, harness as H

import logup_common as LC

P = LC.P


def last_error():
    return ffi.lib().gm_last_error().decode()


def test_shape_rules_refused():
    """each rule of LogupMainphaseProtocol::new (and the library's bounds) is GM_ERR_INVALID with no message read: the proof
    handed over is empty, so a shape that passed would be GM_ERR_VERIFY"""
    rc_of = lambda ls: H.logup_verify(ls, 0, [], [3] * 64)[0]
    assert rc_of([3, 3, 2]) == LC.VERIFY, last_error()          # a valid shape: the empty proof is then rejected
    assert rc_of([0, 0]) == LC.VERIFY, last_error()             # logsize 0 is legal, also for the first two
    assert rc_of([3]) == LC.INVALID and "at least 2" in last_error()
    assert rc_of([]) == LC.INVALID
    assert rc_of([3, 3, 2, 3]) == LC.INVALID and "non-increasing" in last_error()
    assert rc_of([2, 3]) == LC.INVALID and "non-increasing" in last_error()
    assert rc_of([4, 3, 2]) == LC.INVALID and "first two" in last_error()
    assert rc_of([31, 31, 2]) == LC.INVALID and "at most 30" in last_error()
    assert rc_of([3, 3] + [1] * 63) == LC.INVALID and "at most 64" in last_error()
    assert rc_of([3, 3] + [1] * 62) == LC.VERIFY, last_error()  # 64 inputs are fine
    assert rc_of([30, 30]) == LC.VERIFY, last_error()


@pytest.mark.parametrize("logsizes", LC.CPU_SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_oracle_proofs_accepted(logsizes):
    inputs, total = LC.gen_inputs(logsizes, 1000 + sum(logsizes))
    tape = LC.tape_of(7 + len(logsizes))
    o = LC.oracle_prove(logsizes, inputs, total, tape)
    rc, got = H.logup_verify(logsizes, total, o["msgs"], tape)
    assert rc == 0, last_error()
    assert LC.same_claims(got["claims"], o["claims"])
    v_claims, v_pos = LC.oracle_verify(logsizes, total, o["msgs"], tape)
    assert LC.same_claims(got["claims"], v_claims)
    assert got["tape_used"] == o["tape_used"] == v_pos
    # the shape of ClaimsAfter: group 0 about inputs 0 and 1, group g about input g + 1
    assert [len(p) for p, _ in got["claims"]] == [logsizes[0]] + logsizes[2:]
    assert [len(e) for _, e in got["claims"]] == [4] + [2] * (len(logsizes) - 2)


def test_rejections():
    logsizes = [5, 5, 3, 3, 3, 3]
    inputs, total = LC.gen_inputs(logsizes, 77)
    tape = LC.tape_of(78)
    o = LC.oracle_prove(logsizes, inputs, total, tape)
    msgs = o["msgs"]
    assert H.logup_verify(logsizes, total, msgs, tape)[0] == 0, last_error()
    for i in range(len(msgs)):   # each single message incremented by one, every position of the list
        bad = list(msgs)
        bad[i] = (bad[i] + 1) % P
        assert H.logup_verify(logsizes, total, bad, tape)[0] == LC.VERIFY, "message %d of %d" % (i, len(msgs))
    assert H.logup_verify(logsizes, (total + 1) % P, msgs, tape)[0] == LC.VERIFY and "claim" in last_error()
    assert H.logup_verify(logsizes, total, [msgs[0], 0] + msgs[2:], tape)[0] == LC.VERIFY and "zero denominator" in last_error()
    assert H.logup_verify(logsizes, 0, [0, 0] + msgs[2:], tape)[0] == LC.VERIFY and "zero denominator" in last_error()
    assert H.logup_verify(logsizes, total, msgs[:-1], tape)[0] == LC.VERIFY and "ran out" in last_error()
    assert H.logup_verify(logsizes, total, msgs[:2], tape)[0] == LC.VERIFY
    assert H.logup_verify(logsizes, total, msgs + [0], tape)[0] == LC.VERIFY and "unread" in last_error()
