// Registry of caller-defined AlgFns (gm_fn_program_create / destroy) and their host-side evaluation.  See fnprog.hpp.
#include "fnprog.hpp"

static_assert(sizeof(gm_fn_term) == 40 && offsetof(gm_fn_term, out) == 32 && offsetof(gm_fn_term, n_factors) == 34 &&
                  offsetof(gm_fn_term, reserved) == 35 && offsetof(gm_fn_term, factor) == 36,
              "gm_fn_term layout is part of the C ABI");

namespace gm {

namespace {
struct Registry {
    std::mutex mu;
    std::map<int32_t, std::shared_ptr<FnProgram>> progs;
    int32_t next_id = GM_FN_PROG_BASE;
};
Registry& registry() {
    static Registry r;
    return r;
}
}  // namespace

int32_t prog_fn_parse(const gm_fn* f, ProgFn* pf) {
    *pf = ProgFn();
    if (!fn_has_prog(f)) return GM_OK;
    Registry& R = registry();
    std::lock_guard<std::mutex> g(R.mu);
    ProgFn r;
    r.nseg = f->nseg;
    for (int s = 0; s < f->nseg; s++) {
        if (f->prim[s] < GM_FN_PROG_BASE) return set_err(GM_ERR_INVALID, "mixed built-in / program functions are not supported");
        if (f->count[s] < 0) return set_err(GM_ERR_INVALID, "bad gm_fn segment %d", s);
        auto it = R.progs.find(f->prim[s]);
        if (it == R.progs.end()) return set_err(GM_ERR_INVALID, "unknown or destroyed program id %d", f->prim[s]);
        r.prog[s] = it->second;
        r.count[s] = f->count[s];
        const int64_t ni = (int64_t)r.n_ins + (int64_t)it->second->n_ins * f->count[s];
        const int64_t no = (int64_t)r.n_outs + (int64_t)it->second->n_outs * f->count[s];
        if (ni > GM_MAX_COLS || no > GM_MAX_COLS) return set_err(GM_ERR_INVALID, "function too wide (max %d columns)", GM_MAX_COLS);
        r.n_ins = (int)ni;
        r.n_outs = (int)no;
        if (f->count[s] > 0 && it->second->deg > r.deg) r.deg = it->second->deg;
    }
    *pf = r;
    return GM_OK;
}

void prog_fn_exec_host(const ProgFn& pf, const Fr* in, Fr* out) {
    int io = 0, oo = 0;
    for (int s = 0; s < pf.nseg; s++) {
        const FnProgram& P = *pf.prog[s];
        for (int c = 0; c < pf.count[s]; c++) {
            for (int o = 0; o < P.n_outs; o++) {
                Fr acc = fr_zero();
                for (uint32_t t = P.ostart[o]; t < P.ostart[o + 1]; t++) {
                    const ProgTerm& T = P.terms[t];
                    Fr p = T.coef;
                    for (uint32_t j = 0; j < T.nf; j++) p = fr_mul(p, in[io + ((T.fpack >> (8 * j)) & 0xffu)]);
                    acc = fr_add(acc, p);
                }
                out[oo + o] = acc;
            }
            io += P.n_ins;
            oo += P.n_outs;
        }
    }
}

int32_t prog_plan_build(const ProgFn& pf, ProgPlan* pp) {
    int dev = 0;
    GM_HIP(hipGetDevice(&dev));
    GM_REQUIRE(dev >= 0 && dev < GM_MAX_DEVICES, "device id %d: the per-device tables of this library hold %d devices", dev, GM_MAX_DEVICES);
    memset(pp, 0, sizeof(*pp));
    pp->nseg = pf.nseg; pp->n_ins = pf.n_ins; pp->n_outs = pf.n_outs; pp->deg = pf.deg;
    Registry& R = registry();
    std::lock_guard<std::mutex> g(R.mu);   // rank threads of one process share the programs
    int in0 = 0, out0 = 0;
    for (int s = 0; s < pf.nseg; s++) {
        FnProgram& P = *pf.prog[s];
        if (!R.progs.count(P.id)) return set_err(GM_ERR_INVALID, "unknown or destroyed program id %d", P.id);
        if (!P.dev[dev]) {
            // first use on this device: a private non-blocking stream, so the copy never waits behind a pre-enqueued fold (which waits
            // for this thread's next challenge) on a blocking stream
            const size_t tb = P.terms.size() * sizeof(ProgTerm), bytes = tb + P.ostart.size() * sizeof(uint32_t);
            void* d = nullptr;
            GM_HIP(hipMalloc(&d, bytes));
            hipStream_t st = nullptr;
            hipError_t e = hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
            if (e == hipSuccess && tb) e = hipMemcpyAsync(d, P.terms.data(), tb, hipMemcpyHostToDevice, st);
            if (e == hipSuccess) e = hipMemcpyAsync(static_cast<char*>(d) + tb, P.ostart.data(), P.ostart.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st);
            if (e == hipSuccess) e = hipStreamSynchronize(st);
            if (st) (void)hipStreamDestroy(st);
            if (e != hipSuccess) {
                (void)hipFree(d);
                return set_err(GM_ERR_HIP, "program %d: device copy failed: %s", P.id, hipGetErrorString(e));
            }
            P.dev[dev] = d;
        }
        ProgSegDev& q = pp->seg[s];
        q.terms = P.dev_terms(dev);
        q.ostart = P.dev_ostart(dev);
        q.n_ins = P.n_ins; q.n_outs = P.n_outs; q.count = pf.count[s]; q.in0 = in0; q.out0 = out0;
        in0 += P.n_ins * pf.count[s];
        out0 += P.n_outs * pf.count[s];
    }
    return GM_OK;
}

ProgRef::ProgRef(const ProgFn& f) : fn(f) {
    std::lock_guard<std::mutex> g(registry().mu);
    for (int s = 0; s < fn.nseg; s++) fn.prog[s]->live++;
}
ProgRef::~ProgRef() {
    std::lock_guard<std::mutex> g(registry().mu);
    for (int s = 0; s < fn.nseg; s++) fn.prog[s]->live--;
}

}  // namespace gm

using namespace gm;

extern "C" int32_t gm_fn_program_create(uint32_t n_ins, uint32_t n_outs, uint32_t deg, const gm_fn_term* terms, uint32_t n_terms,
                                        int32_t* prim_id) {
    GM_REQUIRE(prim_id, "null argument");
    GM_REQUIRE(n_ins >= 1 && n_ins <= GM_MAX_COLS, "n_ins must be 1 .. %d (got %u)", GM_MAX_COLS, n_ins);
    GM_REQUIRE(n_outs >= 1 && n_outs <= GM_MAX_COLS, "n_outs must be 1 .. %d (got %u)", GM_MAX_COLS, n_outs);
    GM_REQUIRE(deg <= GM_FN_PROG_MAX_DEG, "deg %u exceeds GM_FN_PROG_MAX_DEG (%d)", deg, GM_FN_PROG_MAX_DEG);
    GM_REQUIRE(n_terms <= GM_FN_PROG_MAX_TERMS, "%u terms exceed GM_FN_PROG_MAX_TERMS (%d)", n_terms, GM_FN_PROG_MAX_TERMS);
    GM_REQUIRE(n_terms == 0 || terms, "null terms");
    std::shared_ptr<FnProgram> P(new FnProgram());
    P->n_ins = (int)n_ins; P->n_outs = (int)n_outs; P->deg = (int)deg;
    std::vector<std::vector<ProgTerm>> by_out(n_outs);
    for (uint32_t t = 0; t < n_terms; t++) {
        const gm_fn_term& T = terms[t];
        GM_REQUIRE(T.reserved == 0, "term %u: reserved must be 0", t);
        GM_REQUIRE(T.out < n_outs, "term %u: output %u out of range (n_outs %u)", t, (unsigned)T.out, n_outs);
        GM_REQUIRE(T.n_factors <= GM_FN_PROG_MAX_DEG, "term %u: %u factors exceed GM_FN_PROG_MAX_DEG", t, (unsigned)T.n_factors);
        GM_REQUIRE(T.n_factors <= deg, "term %u: %u factors exceed the declared degree %u", t, (unsigned)T.n_factors, deg);
        ProgTerm q;
        memset(&q, 0, sizeof(q));
        memcpy(&q.coef, T.coef, 32);
        q.coef = fr_reduce_once(fr_reduce_once(q.coef));   // any 256-bit value: canonical
        q.nf = T.n_factors;
        for (uint32_t j = 0; j < T.n_factors; j++) {
            GM_REQUIRE(T.factor[j] < n_ins, "term %u: factor %u = input %u out of range (n_ins %u)", t, j, (unsigned)T.factor[j], n_ins);
            q.fpack |= (uint32_t)T.factor[j] << (8 * j);
        }
        q.out = T.out;
        by_out[T.out].push_back(q);
    }
    P->ostart.push_back(0);
    for (uint32_t o = 0; o < n_outs; o++) {
        P->terms.insert(P->terms.end(), by_out[o].begin(), by_out[o].end());
        P->ostart.push_back((uint32_t)P->terms.size());
    }
    Registry& R = registry();
    std::lock_guard<std::mutex> g(R.mu);
    GM_REQUIRE(R.next_id < INT32_MAX, "program ids exhausted");
    P->id = R.next_id++;
    R.progs[P->id] = P;
    *prim_id = P->id;
    return GM_OK;
}

extern "C" int32_t gm_fn_program_destroy(int32_t prim_id) {
    Registry& R = registry();
    std::shared_ptr<FnProgram> P;
    {
        std::lock_guard<std::mutex> g(R.mu);
        auto it = R.progs.find(prim_id);
        GM_REQUIRE(it != R.progs.end(), "unknown or destroyed program id %d", prim_id);
        if (it->second->live > 0)
            return set_err(GM_ERR_STATE, "program %d is held by %d sumcheck object(s) or circuit witness(es): destroy them first", prim_id, it->second->live);
        P = it->second;
        R.progs.erase(it);
    }
    // map kernels that read a device copy may still be running: synchronise every device that holds one, then free it
    bool any = false;
    for (int d = 0; d < GM_MAX_DEVICES; d++) any = any || P->dev[d];
    if (!any) return GM_OK;   // never used on a device: no runtime call
    int cur = 0;
    GM_HIP(hipGetDevice(&cur));
    int32_t rc = GM_OK;
    for (int d = 0; d < GM_MAX_DEVICES; d++) {
        if (!P->dev[d]) continue;
        hipError_t e = hipSetDevice(d);
        if (e == hipSuccess) e = hipDeviceSynchronize();
        if (e == hipSuccess) e = hipFree(P->dev[d]);
        P->dev[d] = nullptr;
        if (e != hipSuccess && rc == GM_OK) rc = set_err(GM_ERR_HIP, "program %d: freeing the copy on device %d: %s", prim_id, d, hipGetErrorString(e));
    }
    GM_HIP(hipSetDevice(cur));
    return rc;
}
