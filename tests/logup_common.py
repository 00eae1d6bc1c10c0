"""Shared pieces of the GKR-logup tests: seeded inputs as in the reference's tests (logup_mainphase.rs:252-338: random quotient and
non-zero denominator columns, numerator = quotient x denominator, expected sum = the sum of the quotients), the oracle's prover over
them, and the comparison of claim groups."""
import ctypes as C

import numpy as np

from gkr_msm_amd import ffi, harness as H
from pyref import field as F
from pyref import pushforward as PF
from pyref import sumcheck as SC
from pyref import verifier as V

P = F.P
INVALID, STATE, VERIFY = 1, 4, 5

# item 2 of the issue; the GPU suite adds two shapes
CPU_SHAPES = [[0, 0], [0, 0, 0], [1, 1], [5, 5, 3, 3, 3, 3], [5, 5, 3, 3, 3, 3, 1, 0, 0, 0], [6, 6, 6, 6, 2], [11, 11, 10, 9, 4]]
GPU_SHAPES = CPU_SHAPES + [[12, 12, 12, 7, 0], [13, 13, 10, 4]]


def gen_inputs(logsizes, seed):
    """-> ([(num, den), ...] as canonical ints, expected sum)"""
    rng = F.SplitMix64(seed)
    inputs, total = [], 0
    for lg in logsizes:
        q = [rng.next_fr() for _ in range(1 << lg)]
        d = []
        while len(d) < 1 << lg:
            v = rng.next_fr()
            if v:
                d.append(v)
        inputs.append(([a * b % P for a, b in zip(q, d)], d))
        total = (total + sum(q)) % P
    return inputs, total


def tape_of(seed, n=400):
    rng = F.SplitMix64(seed)
    return [rng.next_bits(128) for _ in range(n)]


def oracle_prove(logsizes, inputs, claim, tape):
    """logup_mainphase_prove over a TapeTranscript -> dict(msgs (flat), claims, tape_used, rounds)"""
    tr = SC.TapeTranscript(tape)
    claims = PF.logup_mainphase_prove(tr, list(logsizes), claim, inputs)
    msgs = [v % P for m in tr.msgs for v in m]
    return dict(msgs=msgs, claims=[(list(p), [e % P for e in ev]) for p, ev in claims], tape_used=tr.pos)


def oracle_verify(logsizes, claim, msgs, tape):
    rt = V.ReadTranscript(msgs, [], tape)
    claims = V.logup_mainphase_verify(rt, list(logsizes), claim)
    assert rt.done()
    return [(list(p), [e % P for e in ev]) for p, ev in claims], rt.pos


def n_rounds(logsizes):
    """sumcheck rounds of the main phase: every step runs curr_logsize of them"""
    ls, curr, n = list(logsizes), 0, 0
    while True:
        n += curr
        if ls[-1] == curr:
            if len(ls) == 2:
                return n
            ls.pop()
        else:
            curr += 1


def same_claims(a, b):
    return len(a) == len(b) and all(list(pa) == list(pb) and list(ea) == list(eb) for (pa, ea), (pb, eb) in zip(a, b))


def to_dev_cols(inputs):
    """[(num, den), ...] -> (device numerators, device denominators), Montgomery"""
    return [H.to_dev(H.fr_arg(n)) for n, _ in inputs], [H.to_dev(H.fr_arg(d)) for _, d in inputs]


def check_claims_against_inputs(logsizes, claims, nums, dens):
    """the reference's closing asserts (logup_mainphase.rs:321-336): every final claim is the input column evaluated at the point"""
    pt, ev = claims[0]
    assert H.dense_evaluate([nums[0], dens[0], nums[1], dens[1]], logsizes[0], pt) == ev
    for g in range(1, len(claims)):
        pt, ev = claims[g]
        assert len(pt) == logsizes[g + 1]
        assert H.dense_evaluate([nums[g + 1], dens[g + 1]], logsizes[g + 1], pt) == ev


def big_inputs(logsizes, seed):
    """sizes no Python oracle reaches: 62-bit quotients and odd 64-bit denominators drawn with numpy, turned into Montgomery elements
    and multiplied on the device -> (device numerators, device denominators, expected sum computed on the host from the quotients)"""
    L = ffi.lib()
    g = np.random.default_rng(seed)
    nums, dens, total = [], [], 0
    for lg in logsizes:
        n = 1 << lg
        q = g.integers(0, 1 << 62, size=n, dtype=np.uint64)
        d = g.integers(0, 1 << 63, size=n, dtype=np.uint64) | np.uint64(1)
        total += (int((q >> np.uint64(32)).sum()) << 32) + int((q & np.uint64(0xFFFFFFFF)).sum())
        cols = []
        for v in (q, d):
            limbs = np.zeros((n, 4), dtype=np.uint64)
            limbs[:, 0] = v
            t = H.to_dev(limbs)
            ffi.check(L.gm_fr_batch(5, C.c_void_p(t.data_ptr()), None, C.c_void_p(t.data_ptr()), n, H.cur_stream()))
            cols.append(t)
        num = H.dev_empty(4 * n)
        ffi.check(L.gm_fr_batch(2, C.c_void_p(cols[0].data_ptr()), C.c_void_p(cols[1].data_ptr()), C.c_void_p(num.data_ptr()), n,
                                H.cur_stream()))
        nums.append(num)
        dens.append(cols[1])
    return nums, dens, total % P
