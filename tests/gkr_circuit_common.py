"""Shared pieces of the caller-defined GKR circuit tests: random deg-2 programs with Python twins, random layer lists, and the
oracle's builder + SimpleGKR prover (oracle/pyref/gkr.py) over the same list."""
from gkr_msm_amd import ffi, harness as H
from pyref import algfn as A
from pyref import field as F
from pyref import gkr as G
from pyref import polys as PL
from pyref import sumcheck as SC

P = F.P
INVALID, STATE, VERIFY = 1, 4, 5

BUILTIN_PY = {1: A.AFF_L1, 2: A.AFF_L2, 3: A.AFF_L3, 4: A.PROJ_L1, 5: A.PROJ_L2, 6: A.PROJ_L3, 7: A.TRI_L1, 9: A.BitCheckFn()}
BUILTIN_BY_INS = {1: [9], 3: [2, 3], 4: [1, 5, 6], 6: [4], 12: [7]}


def py_eval(terms, n_outs, args):
    out = [0] * n_outs
    for coef, o, factors in terms:
        v = coef % P
        for f in factors:
            v = v * args[f] % P
        out[o] = (out[o] + v) % P
    return out


class Prog:
    """a registered deg-2 program and its Python twin"""

    def __init__(self, n_ins, n_outs, terms, deg=2):
        self.n_ins, self.n_outs, self.terms = n_ins, n_outs, terms
        self.id = H.make_program(n_ins, n_outs, deg, terms)
        self.py = A.AlgFn("prog%d" % self.id, deg, n_ins, n_outs, lambda a: py_eval(terms, n_outs, a))

    def fn(self):
        return ffi.make_fn((self.id, 1))


def rand_terms(rng, n_ins, n_outs, zero_tail=0):
    """random terms of degree <= 2 (at least one of degree 2 per live output); the last zero_tail outputs have none (always 0)"""
    terms = []
    for o in range(n_outs - zero_tail):
        for _ in range(1 + rng.next_bits(2)):
            nf = rng.next_bits(64) % 3
            terms.append((rng.next_fr(), o, tuple(rng.next_bits(64) % n_ins for _ in range(nf))))
        terms.append((rng.next_fr(), o, (rng.next_bits(64) % n_ins, rng.next_bits(64) % n_ins)))
    return terms


def random_circuit(rng, in_cols, nv, n_layers, max_cols=9, vecvec_rows=None, progs_only=False):
    """-> spec for the library ([("map", GmFn) | ("split", hi, idx, bundle) | ("zerocheck",)]), the same list with Python functions,
    and the programs made (keep them alive).  vecvec_rows: the input is a VecVec with that many row variables (splits LO(0))."""
    spec, pyspec, progs = [], [], []
    cols = in_cols
    rl = vecvec_rows
    if rng.next_bits(1) and nv >= 2 and (rl is None or rl >= 2):   # a leading identity split
        b = 1 if cols == 1 else cols
        hi = rl is None and rng.next_bits(1) == 1
        idx = 0 if rl is not None else rng.next_bits(64) % nv
        spec.append(("split", hi, idx, b)); pyspec.append(("split", hi, idx, b))
        cols, nv = cols * 2, nv - 1
        if rl is not None:
            rl = None if rl == 1 else rl - 1
    while len(spec) < n_layers:
        r = rng.next_bits(64) % 10
        if r < 2 and nv >= 2 and cols * 2 <= max_cols and (rl is None or rl >= 1):
            divs = [b for b in range(1, cols + 1) if cols % b == 0]
            b = divs[rng.next_bits(64) % len(divs)]
            hi = rl is None and rng.next_bits(1) == 1
            idx = 0 if rl is not None else rng.next_bits(64) % nv
            spec.append(("split", hi, idx, b)); pyspec.append(("split", hi, idx, b))
            cols, nv = cols * 2, nv - 1
            if rl is not None:
                rl = None if rl == 1 else rl - 1
            continue
        if not progs_only and cols in BUILTIN_BY_INS and r < 4:
            opts = BUILTIN_BY_INS[cols]
            bid = opts[rng.next_bits(64) % len(opts)]
            f = ffi.make_fn((bid, 1))
            spec.append(("map", f)); pyspec.append(("map", BUILTIN_PY[bid]))
            cols = BUILTIN_PY[bid].n_outs
            continue
        zc = r >= 8
        n_outs = 1 + rng.next_bits(64) % min(max_cols // 2, 4) + (2 if zc else 0)
        if rl is not None:   # the oracle's VecVec object folds with GammaWrapper, which needs two outputs or more
            n_outs = max(n_outs, 2)
        p = Prog(cols, n_outs, rand_terms(rng, cols, n_outs, 2 if zc else 0))
        progs.append(p)
        spec.append(("map", p.fn())); pyspec.append(("map", p.py))
        cols = n_outs
        if zc:
            spec.append(("zerocheck",)); pyspec.append(("zerocheck",))
            cols -= 2
    return spec, pyspec, progs


def oracle_build(pyspec, cols):
    """the builder of bintree_add.rs / triangle_add.rs over a dense input (maps and splits unfused: the same values)
    -> (oracle layer list, advices, output columns)"""
    layers, advices, cur = [], [], [list(c) for c in cols]
    nv = PL.log2_exact(len(cur[0]))
    for l in pyspec:
        if l[0] == "map":
            layers.append(("dense", l[1], nv)); advices.append(("D", cur))
            cur = PL.dense_algfn_map(cur, l[1])
        elif l[0] == "split":
            idx = PL.HI(l[2]) if l[1] else PL.LO(l[2])
            layers.append(("split", idx, l[3])); advices.append(G.EMPTY)
            cur = PL.dense_algfn_map_split(cur, A.IdAlgFn(len(cur)), idx, l[3])
            nv -= 1
        else:
            assert all(v == 0 for v in cur[-2] + cur[-1])
            layers.append(("zerocheck",)); advices.append(G.EMPTY)
            cur = cur[:-2]
    return layers, advices, cur


def oracle_prove(layers, advices, point, evs, tape):
    """SimpleGKR::prove in the oracle under a TapeTranscript -> (flat messages, final point, final evs, challenges used)"""
    tr = SC.TapeTranscript(tape)
    pt, ev = G.simple_gkr_prove(tr, layers, advices, (list(point), list(evs)))
    return [x for m in tr.msgs for x in m], list(pt), list(ev), tr.pos
