// Protocol shapes shared by the provers (prover.hip) and the verifier (verifier.hip): the layer lists of the two GKR circuits
// and the verifier-side polynomials.  Host only.
#pragma once
#include <string>
#include <vector>

#include "fnprog.hpp"
#include "internal.hpp"
#include "segfn.hip.h"

namespace gm {

inline gm_fn mkfn(int p0, int c0, int p1 = 0, int c1 = 0) {
    gm_fn f;
    memset(&f, 0, sizeof(f));
    f.nseg = p1 ? 2 : 1;
    f.prim[0] = p0; f.count[0] = c0;
    f.prim[1] = p1; f.count[1] = c1;
    return f;
}

inline SegPlan plan_of(const gm_fn& f) {
    GmFn g;
    to_gmfn(&f, &g);
    SegPlan sp;
    seg_plan_build(g, &sp);
    return sp;
}

struct Layer {
    enum Kind { VECVEC, DENSE, SPLIT, ZEROCHECK } kind;
    gm_fn f;
    uint32_t num_vars = 0;
    bool split_hi = false;
    uint32_t split_idx = 0, bundle = 3;
};

// bintree_add::builder::protocol::build (bintree_add.rs:247-375)
inline std::vector<Layer> bintree_layers(uint32_t num_vars, uint32_t num_adds, uint32_t row_logsize, bool do_bitcheck) {
    std::vector<Layer> layers;
    for (uint32_t i = 0; i < num_adds; i++) {
        for (int step = 0; step < 3; step++) {
            Layer L;
            L.kind = (i == 0 || i + 1 < row_logsize) ? Layer::VECVEC : Layer::DENSE;
            L.num_vars = num_vars - i - 1;
            const int prim = (i == 0) ? (step == 0 ? GM_FN_AFF_L1 : step == 1 ? GM_FN_AFF_L2 : GM_FN_AFF_L3)
                                      : (step == 0 ? GM_FN_PROJ_L1 : step == 1 ? GM_FN_PROJ_L2 : GM_FN_PROJ_L3);
            L.f = (i == 0 && step == 0 && do_bitcheck) ? mkfn(GM_FN_AFF_L1, 1, GM_FN_BITCHECK, 2) : mkfn(prim, 1);
            layers.push_back(L);
            if (i == 0 && step == 0 && do_bitcheck) {
                Layer Z;
                Z.kind = Layer::ZEROCHECK;
                layers.push_back(Z);
            }
        }
        if (i != num_adds - 1) {
            Layer S;
            S.kind = Layer::SPLIT; S.split_hi = false; S.split_idx = 0; S.bundle = 3;
            layers.push_back(S);
        }
    }
    return layers;
}

// triangle_add::builder::protocol::build (triangle_add.rs:173-232)
inline std::vector<Layer> triangle_layers(uint32_t num_vars, uint32_t hi_idx) {
    std::vector<Layer> layers;
    const uint32_t num_layers = num_vars - hi_idx;
    for (uint32_t l = 0; l <= num_layers; l++) {
        Layer a, b, c;
        a.kind = b.kind = c.kind = Layer::DENSE;
        a.num_vars = b.num_vars = c.num_vars = num_vars - l;
        a.f = mkfn(GM_FN_TRI_L1, 1, GM_FN_PROJ_L1, (int)l);
        b.f = mkfn(GM_FN_PROJ_L2, (int)l + 3);
        c.f = mkfn(GM_FN_PROJ_L3, (int)l + 3);
        layers.push_back(a); layers.push_back(b); layers.push_back(c);
        if (l < num_layers) {
            Layer S;
            S.kind = Layer::SPLIT; S.split_hi = true; S.split_idx = hi_idx; S.bundle = 3;
            layers.push_back(S);
        }
    }
    return layers;
}

// ---- caller-defined circuits (gm_gkr_layer lists): the one shape pass shared by the builder and the verifier
// n_ins / n_outs / deg of a layer function, program or built-in (never a SegPlan for a program: seg_plan_build refuses them)
inline int32_t fn_shape_any(const gm_fn& f, int* n_ins, int* n_outs, int* deg) {
    ProgFn pf;
    const int32_t pr = prog_fn_parse(&f, &pf);
    if (pr) return pr;
    if (pf.nseg) { *n_ins = pf.n_ins; *n_outs = pf.n_outs; *deg = pf.deg; return GM_OK; }
    GmFn g;
    const int32_t rc = to_gmfn(&f, &g);
    if (rc) return rc;
    SegPlan sp;
    if (!seg_plan_build(g, &sp)) return set_err(GM_ERR_INVALID, "function too wide");
    *n_ins = sp.n_ins; *n_outs = sp.n_outs; *deg = sp.deg;
    return GM_OK;
}

struct CircuitShape {
    std::vector<Layer> layers;       // MAP layers as Layer::DENSE (the builder sets VECVEC from its advice), num_vars filled in
    uint32_t in_cols = 0, in_vars = 0, out_cols = 0, out_vars = 0;
};

// Checks every rule of the layer list (include/gkrmsm.h, "caller-defined GKR circuits") from the input's column count and number of
// variables.  vv_row_logsize >= 0: the input is a VecVec with that many row variables (splits must then be LO(0) while it is one).
inline int32_t circuit_shape(const gm_gkr_layer* layers, uint32_t n_layers, uint32_t in_cols, uint32_t in_vars, int vv_row_logsize,
                             CircuitShape* out) {
    if (!layers || n_layers == 0 || n_layers > 65536) return set_err(GM_ERR_INVALID, "the circuit needs 1 .. 65536 layers (got %u)", n_layers);
    if (in_cols < 1 || in_cols > GM_MAX_COLS) return set_err(GM_ERR_INVALID, "%u input columns (1 .. %d)", in_cols, GM_MAX_COLS);
    if (in_vars > 40) return set_err(GM_ERR_INVALID, "%u input variables (at most 40)", in_vars);
    CircuitShape S;
    S.in_cols = in_cols; S.in_vars = in_vars;
    uint32_t cols = in_cols, nv = in_vars;
    int rl = vv_row_logsize;   // VecVec row variables while the columns are VecVec, -1 once dense
    for (uint32_t i = 0; i < n_layers; i++) {
        const gm_gkr_layer& g = layers[i];
        if (g.reserved) return set_err(GM_ERR_INVALID, "layer %u: reserved must be 0", i);
        Layer L;
        L.num_vars = nv;
        if (g.kind == GM_GKR_MAP) {
            int ni = 0, no = 0, dg = 0;
            const int32_t rc = fn_shape_any(g.f, &ni, &no, &dg);
            if (rc) {
                const std::string why = gm_last_error();
                return set_err(rc, "layer %u (MAP): %s", i, why.c_str());
            }
            if ((uint32_t)ni != cols) return set_err(GM_ERR_INVALID, "layer %u (MAP): f takes %d inputs, the layer has %u columns", i, ni, cols);
            if (dg != 2) return set_err(GM_ERR_INVALID, "layer %u (MAP): f has degree %d, a GKR layer needs 2 (dense_eq.rs:200)", i, dg);
            if (no < 1) return set_err(GM_ERR_INVALID, "layer %u (MAP): f has no outputs", i);
            L.kind = Layer::DENSE;
            L.f = g.f;
            cols = (uint32_t)no;
        } else if (g.kind == GM_GKR_SPLIT) {
            if (g.bundle < 1 || cols % g.bundle) return set_err(GM_ERR_INVALID, "layer %u (SPLIT): bundle %u does not divide %u columns", i, g.bundle, cols);
            if (nv < 1) return set_err(GM_ERR_INVALID, "layer %u (SPLIT): no variable left to split", i);
            if (g.split_idx >= nv) return set_err(GM_ERR_INVALID, "layer %u (SPLIT): index %u outside %u variables", i, g.split_idx, nv);
            if (g.split_hi > 1) return set_err(GM_ERR_INVALID, "layer %u (SPLIT): split_hi must be 0 or 1", i);
            if (rl >= 0) {
                if (g.split_hi || g.split_idx) return set_err(GM_ERR_INVALID, "layer %u (SPLIT): a VecVec splits at LO(0) only", i);
                if (rl < 1) return set_err(GM_ERR_INVALID, "layer %u (SPLIT): the VecVec has no row variable left", i);
                rl = rl == 1 ? -1 : rl - 1;   // row_logsize 1: the split goes to dense (bintree_add.rs:186-205)
            }
            L.kind = Layer::SPLIT;
            L.split_hi = g.split_hi != 0;
            L.split_idx = g.split_idx;
            L.bundle = g.bundle;
            cols *= 2;
            nv -= 1;
        } else if (g.kind == GM_GKR_ZEROCHECK) {
            if (cols < 2) return set_err(GM_ERR_INVALID, "layer %u (ZEROCHECK): needs two columns, the layer has %u", i, cols);
            L.kind = Layer::ZEROCHECK;
            cols -= 2;
        } else {
            return set_err(GM_ERR_INVALID, "layer %u: unknown kind %d", i, g.kind);
        }
        if (cols > GM_MAX_COLS) return set_err(GM_ERR_INVALID, "layer %u: %u columns (at most %d)", i, cols, GM_MAX_COLS);
        S.layers.push_back(L);
    }
    if (cols < 1) return set_err(GM_ERR_INVALID, "the circuit has no output column");
    S.out_cols = cols;
    S.out_vars = nv;
    *out = std::move(S);
    return GM_OK;
}

// the public form of a layer list (gm_gkr_witness_layers)
inline gm_gkr_layer layer_public(const Layer& L) {
    gm_gkr_layer g;
    memset(&g, 0, sizeof(g));
    switch (L.kind) {
        case Layer::VECVEC:
        case Layer::DENSE: g.kind = GM_GKR_MAP; g.f = L.f; break;
        case Layer::SPLIT: g.kind = GM_GKR_SPLIT; g.split_hi = L.split_hi ? 1 : 0; g.split_idx = L.split_idx; g.bundle = L.bundle; break;
        case Layer::ZEROCHECK: g.kind = GM_GKR_ZEROCHECK; break;
    }
    return g;
}

// EqTruncPoly::evaluate (verifier_polys.rs:108-147)
inline Fr eq_trunc_evaluate(uint32_t nv, uint64_t k, const Fr* r, const Fr* pt) {
    std::vector<Fr> partial(nv + 1);
    partial[0] = fr_one();
    for (uint32_t i = 0; i < nv; i++) {
        const uint32_t j = nv - i - 1;
        partial[i + 1] = fr_mul(partial[i], eq_bind_factor(r[j], pt[j]));
    }
    if (k >= (1ull << nv)) return partial[nv];
    Fr mult = fr_one(), acc = fr_zero();
    for (uint32_t i = 0; i < nv; i++) {
        const uint64_t left = k >> (nv - i - 1);
        const Fr prev = mult;
        if (left == 1) {
            mult = fr_mul(fr_mul(mult, pt[i]), r[i]);
            acc = fr_add(acc, fr_mul(fr_mul(fr_mul(prev, fr_sub(fr_one(), pt[i])), fr_sub(fr_one(), r[i])), partial[nv - i - 1]));
        } else {
            mult = fr_mul(fr_mul(mult, fr_sub(fr_one(), pt[i])), fr_sub(fr_one(), r[i]));
        }
        k -= left << (nv - i - 1);
    }
    return acc;
}


}  // namespace gm
