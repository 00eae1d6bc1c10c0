// Caller-defined AlgFns ("programs", gm_fn_program_create): a polynomial in monomial form, registered once per process, run by
// kernels of their own (poly.hip, vecvec.hip, sumcheck.hip).  The runtime AlgFn of the reference: ArcedAlgFn::new(f, n_ins,
// n_outs, deg), src/cleanup/utils/algfn.rs:93-131 of the reference crate.
//
// A program never reaches a SegPlan: Seg stores the primitive as int8_t and has at most 6 inputs, and prim_exec / eval_seg switch
// on the id (an unknown id evaluates to nothing).  Every entry point parses its gm_fn with prog_fn_parse first and takes the
// program path or the built-in path before either plan is built.
//
// Evaluation is a loop over terms whose bound and index are the same for every lane of a wave: the term table is read with scalar
// loads (prog_term_load: a uniform address in the constant address space), the factors from the input columns by pointer.
#pragma once
#include <memory>
#include <vector>

#include "internal.hpp"

namespace gm {

// one term on the device (48 bytes): coef * prod_{j < nf} in[(fpack >> 8 j) & 0xff]
struct ProgTerm {
    Fr coef;
    uint32_t nf;
    uint32_t fpack;   // factor j in byte j: an input index of the program (map tables) or an absolute column (object tables)
    uint32_t out;     // output index inside the program
    uint32_t pad;
};
static_assert(sizeof(ProgTerm) == 48, "ProgTerm layout");

// a registered program (host side).  terms are sorted by output (stable); ostart[o] .. ostart[o + 1] are the terms of output o.
// dev[d]: the device copy on device d (terms, then ostart), made on first use, freed by gm_fn_program_destroy
struct FnProgram {
    int32_t id = 0;
    int n_ins = 0, n_outs = 0, deg = 0;
    std::vector<ProgTerm> terms;
    std::vector<uint32_t> ostart;
    void* dev[GM_MAX_DEVICES] = {};
    int live = 0;   // sumcheck objects holding the program (ProgRef)
    const ProgTerm* dev_terms(int d) const { return static_cast<const ProgTerm*>(dev[d]); }
    const uint32_t* dev_ostart(int d) const { return reinterpret_cast<const uint32_t*>(static_cast<const char*>(dev[d]) + terms.size() * sizeof(ProgTerm)); }
};

// the program segments of a gm_fn (at most GM_FN_MAX_SEG): the whole function is sum over segments of count copies, left to right
struct ProgFn {
    int nseg = 0, n_ins = 0, n_outs = 0, deg = 0;   // nseg 0: not a program function
    std::shared_ptr<FnProgram> prog[GM_FN_MAX_SEG];
    int count[GM_FN_MAX_SEG] = {};
};

// f names programs only: *pf filled (pf->nseg >= 1); built-in ids only: pf->nseg = 0 (take the SegPlan path).  Returns an error code
// for a mixed function, an unknown or destroyed id, or one too wide.
int32_t prog_fn_parse(const gm_fn* f, ProgFn* pf);
inline bool fn_has_prog(const gm_fn* f) {
    if (!f || f->nseg < 1 || f->nseg > GM_FN_MAX_SEG) return false;
    for (int s = 0; s < f->nseg; s++) if (f->prim[s] >= GM_FN_PROG_BASE) return true;
    return false;
}
// host evaluation of one row (in: n_ins elements, out: n_outs elements)
void prog_fn_exec_host(const ProgFn& pf, const Fr* in, Fr* out);

// ---- maps: the plan a map kernel receives (kernel argument) -----------------------------------------------------------
struct ProgSegDev {
    const ProgTerm* terms;
    const uint32_t* ostart;
    int32_t n_ins, n_outs, count, in0, out0, pad;
};
struct ProgPlan {
    int32_t nseg, n_ins, n_outs, deg;
    ProgSegDev seg[GM_FN_MAX_SEG];
};
// the device copies of pf's programs on the current device (made on first use), as a map plan
int32_t prog_plan_build(const ProgFn& pf, ProgPlan* pp);

int32_t launch_dense_map_prog(const ProgPlan& pp, const Fr* const* in, Fr* const* out, uint64_t n, hipStream_t s);
int32_t launch_dense_map_split_prog(const ProgPlan& pp, const Fr* const* in, Fr* const* out, uint64_t n, uint32_t lo_bit, uint32_t bundle,
                                    hipStream_t s);

// ---- sumcheck objects: one flat table of the whole function, gamma folded into the coefficients ------------------------
// term t of copy c of segment s: coef * gamma^(out0 + c n_outs + out), factors as absolute columns in0 + c n_ins + f.  The table is
// expanded on the device, in stream order, from the programs' device copies (k_prog_expand, sumcheck.hip).  Holding a ProgRef keeps
// gm_fn_program_destroy from freeing the programs (GM_ERR_STATE).
struct ProgRef {
    ProgFn fn;
    explicit ProgRef(const ProgFn& f);
    ~ProgRef();
};

// ---- device side ----------------------------------------------------------------------------------------------------
#if defined(__HIP_DEVICE_COMPILE__)
typedef const __attribute__((address_space(4))) uint32_t* ConstWords;
#else
typedef const uint32_t* ConstWords;
#endif
// a term at a wave-uniform address: scalar loads (s_load_dword*)
__device__ __forceinline__ void prog_term_load(const ProgTerm* t, Fr* coef, uint32_t* nf, uint32_t* fpack) {
    ConstWords w = (ConstWords)(const void*)t;
#pragma unroll
    for (int l = 0; l < 8; l++) coef->l[l] = w[l];
    *nf = w[8];
    *fpack = w[9];
}
__device__ __forceinline__ uint32_t prog_word_load(const uint32_t* p) { return *(ConstWords)(const void*)p; }

// One row of a map through every copy of every segment: per output, a loop over its terms (scalar loads
// of the table), factors loaded by pointer (repeats hit L1 / L2), the output accumulated in registers and stored once.
// ld(c): input column c of the row; st(o, v): output o of the row.
template <class LD, class ST>
__device__ __forceinline__ void prog_eval_row(const ProgPlan& pp, LD ld, ST st) {
    for (int s = 0; s < pp.nseg; s++) {
        const ProgSegDev& g = pp.seg[s];
        for (int c = 0; c < g.count; c++) {
            const int io = g.in0 + c * g.n_ins, oo = g.out0 + c * g.n_outs;
            for (int o = 0; o < g.n_outs; o++) {
                Fr acc = fr_zero();
                const uint32_t t1 = prog_word_load(g.ostart + o + 1);
                for (uint32_t t = prog_word_load(g.ostart + o); t < t1; t++) {
                    Fr p;
                    uint32_t nf, fp;
                    prog_term_load(g.terms + t, &p, &nf, &fp);
                    for (uint32_t j = 0; j < nf; j++, fp >>= 8) p = fr_mul(p, ld(io + (int)(fp & 0xffu)));
                    acc = fr_add(acc, p);
                }
                st(oo + o, acc);
            }
        }
    }
}

}  // namespace gm
