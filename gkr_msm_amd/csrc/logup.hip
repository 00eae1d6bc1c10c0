// GKR-logup on caller-supplied fractions: the fraction tree of LogupMainphaseProtocol::make_witness
// (cleanup/protocols/pushforward/logup_mainphase.rs:83-143 of the reference) and the two device helpers a lookup argument needs
// to build its fractions (multiplicities of an index column, denominators tau - sum_k psi^k col_k).
//
// The tree: every level is LogupLayerFn (a, b, c, d) -> (a d + b c, b d) of the two fractions before it, followed either by the
// next input joining (sizes equal) or by the HI split (the two contiguous halves: pointer arithmetic).  Large levels are one dense
// map launch each; once a level has at most 2^tail_log elements ONE workgroup runs every remaining step (k_logup_tail): those
// levels are a few KiB each and a launch per level is pure latency.  The top fraction and every level of one element -- the
// prover's [num, den] message and the values of the zero-variable layers -- come back in one copy.
#include <cstdlib>

#include "internal.hpp"
#include "gkr_layers.hpp"
#include "logup.hpp"

namespace gm {

// one step of the small end of the tree.  MAP: (on, od)[i] = LogupLayerFn(a[i], b[i], c[i], d[i]); COPY: (on, od)[i] = (a[i], b[i]),
// for inputs of one element, which the host wants next to the levels.  g != nullptr: element i also goes to g[2 i], g[2 i + 1].
struct LogupStep {
    const Fr* a;
    const Fr* b;
    const Fr* c;
    const Fr* d;
    Fr* on;
    Fr* od;
    Fr* g;
    uint32_t len;
    uint32_t kind;
};
enum { LOGUP_STEP_MAP = 0, LOGUP_STEP_COPY = 1 };
#define GM_LOGUP_TAIL_THREADS 1024
#define GM_LOGUP_STEPS_BY_VALUE 56   // 56 x 64 bytes: under the 4 KiB of kernel arguments with room for the count
struct LogupStepsArg {
    LogupStep s[GM_LOGUP_STEPS_BY_VALUE];
};

// One workgroup.  A MAP step reads what other lanes of the workgroup stored to global memory in the step before: the steps are
// separated by a workgroup-scope release / acquire.  COPY steps read the caller's columns only and come first.
__device__ __forceinline__ void logup_tail_run(const LogupStep* steps, uint32_t n_steps) {
    for (uint32_t k = 0; k < n_steps; k++) {
        const LogupStep st = steps[k];
        if (st.kind == LOGUP_STEP_COPY) {
            for (uint32_t i = threadIdx.x; i < st.len; i += GM_LOGUP_TAIL_THREADS) {
                fr_store(st.g + 2 * i, fr_load(st.a + i));
                fr_store(st.g + 2 * i + 1, fr_load(st.b + i));
            }
            continue;
        }
        for (uint32_t i = threadIdx.x; i < st.len; i += GM_LOGUP_TAIL_THREADS) {
            const Fr a = fr_load(st.a + i), b = fr_load(st.b + i), c = fr_load(st.c + i), d = fr_load(st.d + i);
            const Fr n = fr_add(fr_mul(a, d), fr_mul(b, c)), dd = fr_mul(b, d);   // FN_LOGUP_LAYER (algfn.hip.h)
            fr_store(st.on + i, n);
            fr_store(st.od + i, dd);
            if (st.g) {
                fr_store(st.g + 2 * i, n);
                fr_store(st.g + 2 * i + 1, dd);
            }
        }
        __threadfence_block();
        __syncthreads();
    }
}

__global__ void __launch_bounds__(GM_LOGUP_TAIL_THREADS) k_logup_tail(LogupStepsArg steps, uint32_t n_steps) {
    logup_tail_run(steps.s, n_steps);
}
__global__ void __launch_bounds__(GM_LOGUP_TAIL_THREADS) k_logup_tail_buf(const LogupStep* __restrict__ steps, uint32_t n_steps) {
    logup_tail_run(steps, n_steps);
}

// ---- multiplicities.  cnt[0] is the out-of-range flag, cnt[1 + j] the counter of table row j.
#define GM_LOGUP_HIST_LDS_MAX (1u << 14)   // counters of a table this long fit a 64 KiB share of the LDS
template <bool LDS>
__global__ void __launch_bounds__(256) k_logup_hist(const uint32_t* __restrict__ idx, uint64_t n, uint32_t table_len,
                                                     uint32_t* __restrict__ cnt) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lcnt[];
    if (LDS) {
        for (uint32_t j = threadIdx.x; j < table_len; j += 256) lcnt[j] = 0;
        __syncthreads();
    }
    bool bad = false;
    auto add = [&](uint32_t v) {
        if (v >= table_len) { bad = true; return; }
        if (LDS) atomicAdd(&lcnt[v], 1u);
        else atomicAdd(&cnt[1 + v], 1u);
    };
    const uint64_t tid = (uint64_t)blockIdx.x * 256 + threadIdx.x, stride = (uint64_t)gridDim.x * 256;
    const uint64_t nv = (reinterpret_cast<uintptr_t>(idx) & 15) == 0 ? n / 4 : 0;   // 16-byte loads when the column allows them
    const uint4* idx4 = reinterpret_cast<const uint4*>(idx);
    for (uint64_t q = tid; q < nv; q += stride) {
        const uint4 v = idx4[q];
        add(v.x); add(v.y); add(v.z); add(v.w);
    }
    for (uint64_t i = 4 * nv + tid; i < n; i += stride) add(idx[i]);
    if (bad) atomicOr(&cnt[0], 1u);
    if (LDS) {
        __syncthreads();
        for (uint32_t j = threadIdx.x; j < table_len; j += 256) {
            const uint32_t c = lcnt[j];
            if (c) atomicAdd(&cnt[1 + j], c);
        }
    }
}

__global__ void __launch_bounds__(256) k_logup_cnt_to_fr(const uint32_t* __restrict__ cnt, uint64_t table_len, Fr* __restrict__ m) {
    const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= table_len) return;
    fr_store(m + j, fr_from_u64(cnt[1 + j]));
}

// ---- denominators: den[i] = tau - (..(col_{k-1}[i] psi + col_{k-2}[i]) psi + ..) psi + col_0[i]), or its negative
struct LogupCols {
    const Fr* p[8];
};
__global__ void __launch_bounds__(256) k_logup_den(LogupCols cols, uint32_t k, uint64_t len, Fr psi, Fr tau, int negate,
                                                    Fr* __restrict__ den, Fr* __restrict__ ones) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= len) return;
    Fr v[8];
#pragma unroll
    for (int j = 0; j < 8; j++)
        if ((uint32_t)j < k) v[j] = fr_load(cols.p[j] + i);
    Fr acc = fr_zero();
#pragma unroll
    for (int j = 7; j >= 0; j--)
        if ((uint32_t)j < k) acc = (uint32_t)j + 1 == k ? v[j] : fr_add(fr_mul(acc, psi), v[j]);
    fr_store(den + i, negate ? fr_sub(acc, tau) : fr_sub(tau, acc));
    if (ones) fr_store(ones + i, fr_one());
}

namespace {

#define TRY(x)                      \
    do {                            \
        int32_t rc__ = (x);         \
        if (rc__) return rc__;      \
    } while (0)

// GM_LOGUP_NO_TAIL=1: every level of the tree is a launch of its own and the one-element levels are fetched one by one (the path
// before k_logup_tail; A/B runs).  GM_LOGUP_TAIL_LOG=8..11: the level size from which the tail launch takes over (measurements).
bool logup_no_tail() {
    static const bool v = [] { const char* e = getenv("GM_LOGUP_NO_TAIL"); return e && e[0] == '1'; }();
    return v;
}
uint32_t logup_tail_log() {
    static const uint32_t v = [] {
        const char* e = getenv("GM_LOGUP_TAIL_LOG");
        const long t = e ? strtol(e, nullptr, 10) : 0;
        return (uint32_t)(t >= 8 && t <= 11 ? t : 9);
    }();
    return v;
}

}  // namespace

int32_t logup_build(const std::vector<LogupFrac>& inputs, const std::vector<uint32_t>& logsizes, LogupTree* tree, hipStream_t s) {
    const size_t n_in = inputs.size();
    GM_REQUIRE(n_in == logsizes.size() && n_in >= 2, "logup witness: %zu inputs for %zu logsizes", n_in, logsizes.size());
    for (size_t i = 0; i < n_in; i++)
        GM_REQUIRE(inputs[i].num && inputs[i].den && inputs[i].len == (1ull << logsizes[i]), "logup witness: input %zu is missing or has the wrong length", i);
    const bool tail_on = !logup_no_tail();
    const uint64_t T = tail_on ? (1ull << logup_tail_log()) : 0;
    tree->logsizes = logsizes;
    tree->layers.clear();
    tree->own.clear();

    // sizes only: what the tail launch writes (two columns per step) and how many one-element fractions there are
    uint64_t tail_elems = 0, n_ones = 0;
    {
        uint64_t cur = inputs[0].len;
        size_t next = 2;
        for (size_t i = 0; i < n_in; i++) n_ones += inputs[i].len == 1;
        for (;;) {
            const uint64_t next_size = next < n_in ? inputs[next].len : 1;
            if (cur <= T) tail_elems += 2 * cur;
            if (cur == next_size) {
                n_ones += cur == 1;   // the level itself (the last one is the top fraction)
                if (next < n_in) next++;
                else break;
            } else {
                if (cur == 2) n_ones += 2;
                cur /= 2;
            }
        }
    }
    std::shared_ptr<DevBuf> slab;   // tail levels, then the gathered one-element fractions
    Fr* slab_next = nullptr;
    Fr* gather = nullptr;
    if (tail_on) {
        slab.reset(new DevBuf());
        TRY(slab->alloc((tail_elems + 2 * n_ones) * sizeof(Fr)));
        tree->own.push_back(slab);
        slab_next = slab->fr();
        gather = slab->fr() + tail_elems;
    }
    std::vector<LogupStep> steps, copies;
    std::vector<LogupFrac>& L = tree->layers;
    std::vector<int64_t> slot;   // per layer: its pair in `gather`, or -1
    uint64_t n_slots = 0;
    auto push = [&](const LogupFrac& f, int64_t sl) {
        L.push_back(f);
        slot.push_back(sl);
    };
    auto push_input = [&](const LogupFrac& f) {
        if (tail_on && f.len == 1) {
            copies.push_back(LogupStep{f.num, f.den, nullptr, nullptr, nullptr, nullptr, gather + 2 * n_slots, 1u, LOGUP_STEP_COPY});
            push(f, (int64_t)n_slots++);
        } else {
            push(f, -1);
        }
    };
    push_input(inputs[0]);
    push_input(inputs[1]);
    size_t next_in = 2;
    const SegPlan logup = plan_of(mkfn(GM_FN_LOGUP_LAYER, 1));
    for (size_t i = 0;; i += 2) {
        const uint64_t next_size = next_in < n_in ? inputs[next_in].len : 1;
        const uint64_t curr = L[i].len;
        GM_REQUIRE(L[i + 1].len == curr, "logup witness: unreachable size order");
        LogupFrac o;
        o.len = curr;
        int64_t o_slot = -1;
        if (curr <= T) {
            Fr* on = slab_next;
            Fr* od = slab_next + curr;
            slab_next += 2 * curr;
            Fr* g = nullptr;
            if (curr <= 2 && (curr == 1 || curr != next_size)) {   // one element, or two that the split turns into two of one
                g = gather + 2 * n_slots;
                o_slot = (int64_t)n_slots;
                n_slots += curr;
            }
            steps.push_back(LogupStep{L[i].num, L[i].den, L[i + 1].num, L[i + 1].den, on, od, g, (uint32_t)curr, LOGUP_STEP_MAP});
            o.num = on; o.den = od;
        } else {
            std::shared_ptr<DevBuf> bn(new DevBuf()), bd(new DevBuf());
            TRY(bn->alloc(curr * sizeof(Fr))); TRY(bd->alloc(curr * sizeof(Fr)));
            tree->own.push_back(bn); tree->own.push_back(bd);
            const Fr* in[4] = {L[i].num, L[i].den, L[i + 1].num, L[i + 1].den};
            Fr* outp[2] = {bn->fr(), bd->fr()};
            TRY(launch_dense_map(logup, in, outp, curr, s));
            o.num = bn->fr(); o.den = bd->fr();
        }
        if (curr == next_size) {
            push(o, o_slot);
            if (next_in < n_in) push_input(inputs[next_in++]);
            else break;
        } else {
            GM_REQUIRE(curr > next_size, "logup witness: unreachable size order");
            LogupFrac lo = o, hi = o;
            lo.len = hi.len = curr / 2;
            hi.num = o.num + curr / 2; hi.den = o.den + curr / 2;
            push(lo, o_slot);
            push(hi, o_slot < 0 ? -1 : o_slot + 1);
        }
    }
    GM_REQUIRE(L.back().len == 1, "logup witness does not end in a single fraction");

    std::vector<Fr> h_gather;
    if (tail_on) {
        GM_REQUIRE(n_slots <= n_ones && (uint64_t)(slab_next - slab->fr()) == tail_elems, "logup witness: tail layout does not match its size pass");
        copies.insert(copies.end(), steps.begin(), steps.end());
        const uint32_t n_steps = (uint32_t)copies.size();
        std::shared_ptr<DevBuf> d_steps;
        if (n_steps <= GM_LOGUP_STEPS_BY_VALUE) {
            LogupStepsArg arg;
            memset(&arg, 0, sizeof(arg));
            memcpy(arg.s, copies.data(), n_steps * sizeof(LogupStep));
            hipLaunchKernelGGL(k_logup_tail, dim3(1), dim3(GM_LOGUP_TAIL_THREADS), 0, s, arg, n_steps);
        } else {
            d_steps.reset(new DevBuf());
            TRY(d_steps->alloc(n_steps * sizeof(LogupStep)));
            GM_HIP(hipMemcpyAsync(d_steps->p, copies.data(), n_steps * sizeof(LogupStep), hipMemcpyHostToDevice, s));
            hipLaunchKernelGGL(k_logup_tail_buf, dim3(1), dim3(GM_LOGUP_TAIL_THREADS), 0, s,
                               reinterpret_cast<const LogupStep*>(d_steps->p), n_steps);
        }
        GM_LAUNCH_CHECK();
        h_gather.resize(2 * n_slots);
        GM_HIP(hipMemcpyAsync(h_gather.data(), gather, 2 * n_slots * sizeof(Fr), hipMemcpyDeviceToHost, s));
        GM_HIP(hipStreamSynchronize(s));   // `copies` and d_steps go out of scope
    }
    for (size_t i = 0; i < L.size(); i++) {
        if (L[i].len != 1) continue;
        if (tail_on) {
            GM_REQUIRE(slot[i] >= 0, "logup witness: a one-element level was not gathered");
            L[i].h_num = h_gather[2 * slot[i]];
            L[i].h_den = h_gather[2 * slot[i] + 1];
        } else {
            GM_HIP(hipMemcpyAsync(&L[i].h_num, L[i].num, sizeof(Fr), hipMemcpyDeviceToHost, s));
            GM_HIP(hipStreamSynchronize(s));
            GM_HIP(hipMemcpyAsync(&L[i].h_den, L[i].den, sizeof(Fr), hipMemcpyDeviceToHost, s));
            GM_HIP(hipStreamSynchronize(s));
        }
    }
    tree->total[0] = L.back().h_num;
    tree->total[1] = L.back().h_den;
    L.pop_back();
    return GM_OK;
}

}  // namespace gm

using namespace gm;

extern "C" int32_t gm_logup_multiplicities(const uint32_t* d_idx, uint64_t n, uint64_t table_len, uint64_t* d_m, void* stream) {
    GM_REQUIRE(d_m && (d_idx || !n), "null argument");
    GM_REQUIRE(table_len >= 1 && table_len <= (1ull << GM_LOGUP_MAX_LOGSIZE), "table_len %llu out of range (1 .. 2^%d)",
               (unsigned long long)table_len, GM_LOGUP_MAX_LOGSIZE);
    GM_REQUIRE(n < (1ull << 32), "n = %llu: the counters are 32 bits wide, n < 2^32 is required", (unsigned long long)n);
    hipStream_t s = as_stream(stream);
    DevBuf cnt;
    TRY(cnt.alloc((table_len + 1) * sizeof(uint32_t)));
    uint32_t* d_cnt = reinterpret_cast<uint32_t*>(cnt.p);
    GM_HIP(hipMemsetAsync(d_cnt, 0, (table_len + 1) * sizeof(uint32_t), s));
    if (n) {
        // 16 indices per thread and pass; at most 8 workgroups per CU's worth of grid so that the per-workgroup flush of the LDS
        // counters stays small next to the counting
        const uint64_t want = (n + 256 * 16 - 1) / (256 * 16);
        const unsigned grid = (unsigned)(want < 2048 ? want : 2048);
        if (table_len <= GM_LOGUP_HIST_LDS_MAX)
            hipLaunchKernelGGL(k_logup_hist<true>, dim3(grid), dim3(256), table_len * sizeof(uint32_t), s, d_idx, n, (uint32_t)table_len, d_cnt);
        else
            hipLaunchKernelGGL(k_logup_hist<false>, dim3(grid), dim3(256), 0, s, d_idx, n, (uint32_t)table_len, d_cnt);
        GM_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_logup_cnt_to_fr, dim3(ceil_div(table_len, 256)), dim3(256), 0, s, d_cnt, table_len, reinterpret_cast<Fr*>(d_m));
    GM_LAUNCH_CHECK();
    uint32_t flag = 0;
    GM_HIP(hipMemcpyAsync(&flag, d_cnt, sizeof(flag), hipMemcpyDeviceToHost, s));
    GM_HIP(hipStreamSynchronize(s));
    GM_REQUIRE(!flag, "an index is >= table_len = %llu", (unsigned long long)table_len);
    return GM_OK;
}

extern "C" int32_t gm_logup_denominators(uint32_t k, const uint64_t* const* d_cols, uint64_t len, const uint64_t* h_psi,
                                         const uint64_t* h_tau, int32_t negate, uint64_t* d_den, uint64_t* d_ones, void* stream) {
    GM_REQUIRE(d_cols && h_psi && h_tau && d_den, "null argument");
    GM_REQUIRE(k >= 1 && k <= 8, "%u columns, 1 .. 8 are supported", k);
    GM_REQUIRE(len <= (1ull << GM_LOGUP_MAX_LOGSIZE), "len %llu out of range", (unsigned long long)len);
    LogupCols cols;
    for (uint32_t j = 0; j < 8; j++) cols.p[j] = nullptr;
    for (uint32_t j = 0; j < k; j++) {
        GM_REQUIRE(d_cols[j], "column %u is null", j);
        cols.p[j] = reinterpret_cast<const Fr*>(d_cols[j]);
    }
    if (!len) return GM_OK;
    Fr psi, tau;
    memcpy(&psi, h_psi, sizeof(Fr));
    memcpy(&tau, h_tau, sizeof(Fr));
    hipLaunchKernelGGL(k_logup_den, dim3(ceil_div(len, 256)), dim3(256), 0, as_stream(stream), cols, k, len, psi, tau, negate != 0,
                       reinterpret_cast<Fr*>(d_den), reinterpret_cast<Fr*>(d_ones));
    GM_LAUNCH_CHECK();
    return GM_OK;
}
