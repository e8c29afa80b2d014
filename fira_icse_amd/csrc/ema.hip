// Exponential moving average of the weights: ema moves toward the parameters by the weight w, for every element
//     diff = p - e;   e = e + w * diff
// the subtraction, the multiply and the add each rounded to fp32 on its own (no fused multiply-add: the element function is
// compiled with contraction off and the three operations are separate statements, as mix_elem in mix.hip), so a loop of
// np.float32 operations is the reference.  An element with p == e keeps its value (diff = 0).
//
// fira_ema_update       the plain form over n floats.  The range is cut at the 16-byte boundaries of EMA: a scalar head (up to 3
//                       elements), a body of 4-element groups -- one 16-byte load and one 16-byte store of ema each, and one
//                       16-byte load of p if p has ema's alignment phase (launch-uniform: the body loop is instantiated for
//                       both cases instead of selecting per element), four 4-byte loads otherwise -- and a scalar tail.  Two
//                       groups per thread are in flight per trip.  Grid-stride; the pass is bound by HBM (12 bytes per element).
// fira_ema_update_rows  the whole flat buffer [0, total) of a model in one launch, the two vocabulary-sized embedding tables
//                       read as a forward pass reads them under the row-sparse Adam: one wave per 256-float row through
//                       adam_rows_load (adam_rows.h), i.e. the stored row with the zero-gradient updates it still owes applied
//                       in registers.  A row that owes nothing loads neither m nor v (the wave-uniform branch of adam_rows_load).
//                       Everything outside the tables runs as the plain form.  The kernel writes ema only.
//
// ema is written once per update and next read one update later: its loads and stores are non-temporal (they do not displace
// the parameters the next forward pass reads from the cache).  p is read with the default policy.
#include <math.h>
#include <algorithm>
#include "adam_rows.h"

namespace fira {

typedef float ema_f4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ int64_t ema_min(int64_t a, int64_t b) { return a < b ? a : b; }

__device__ __forceinline__ float ema_elem(float e, float p, float w) {
#pragma clang fp contract(off)
    const float diff = p - e;
    const float t = w * diff;
    return e + t;
}
__device__ __forceinline__ ema_f4 ema_elem4(ema_f4 e, float4 p, float w) {
    ema_f4 r;
    r.x = ema_elem(e.x, p.x, w);
    r.y = ema_elem(e.y, p.y, w);
    r.z = ema_elem(e.z, p.z, w);
    r.w = ema_elem(e.w, p.w, w);
    return r;
}

// the 4-element groups g = tid, tid + stride, ... of [0, nvec) of e (16-byte aligned); WIDE: p is 16-byte aligned too
template <bool WIDE>
__device__ __forceinline__ void ema_body(float* __restrict__ e, const float* __restrict__ p, int64_t nvec, float w, int64_t tid,
                                         int64_t stride) {
    for (int64_t g0 = tid; g0 < nvec; g0 += 2 * stride) {
        ema_f4 ev[2];
        float4 pv[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int64_t i = 4 * ema_min(g0 + u * stride, nvec - 1);               // (clamped: requested, not used, past the end)
            ev[u] = __builtin_nontemporal_load(reinterpret_cast<const ema_f4*>(e + i));
            if (WIDE) pv[u] = *reinterpret_cast<const float4*>(p + i);
            else pv[u] = make_float4(p[i], p[i + 1], p[i + 2], p[i + 3]);
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int64_t g = g0 + u * stride;
            if (g < nvec) __builtin_nontemporal_store(ema_elem4(ev[u], pv[u], w), reinterpret_cast<ema_f4*>(e + 4 * g));
        }
    }
}

// e[0, n) toward p[0, n) by the threads tid of `stride`; any n >= 0, any 4-byte alignment of either pointer
__device__ __forceinline__ void ema_range(float* __restrict__ e, const float* __restrict__ p, int64_t n, float w, int64_t tid,
                                          int64_t stride) {
    const int64_t head = ema_min((int64_t)(((16u - (unsigned)((uintptr_t)e & 15u)) & 15u) >> 2), n);
    const int64_t nvec = (n - head) >> 2;
    const int64_t tail0 = head + 4 * nvec;
    if (tid < head) e[tid] = ema_elem(e[tid], p[tid], w);
    if (tid < n - tail0) e[tail0 + tid] = ema_elem(e[tail0 + tid], p[tail0 + tid], w);
    if (((uintptr_t)(p + head) & 15u) == 0) ema_body<true>(e + head, p + head, nvec, w, tid, stride);      // (launch-uniform)
    else ema_body<false>(e + head, p + head, nvec, w, tid, stride);
}

__global__ __launch_bounds__(256) void ema_kernel(int64_t n, float* __restrict__ e, const float* __restrict__ p, float w) {
    ema_range(e, p, n, w, (int64_t)blockIdx.x * 256 + threadIdx.x, (int64_t)gridDim.x * 256);
}

// one table of `rows` 256-float rows at e / p (16-byte aligned), one wave per row, two rows per trip
__device__ __forceinline__ void ema_table(float* __restrict__ e, const float* __restrict__ p, int rows, const AdamRowsView& vw,
                                          float w) {
    const int lane = threadIdx.x & 63;
    const int nw = gridDim.x * 4;
    for (int r0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * 2; r0 < rows; r0 += nw * 2) {
        ema_f4 ev[2];
        float4 pv[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int r = min(r0 + u, rows - 1);                                // (clamped, as above)
            ev[u] = __builtin_nontemporal_load(reinterpret_cast<const ema_f4*>(e + (size_t)r * FIRA_D + lane * 4));
            pv[u] = adam_rows_load(p, r, lane, vw);
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int r = r0 + u;
            if (r < rows)
                __builtin_nontemporal_store(ema_elem4(ev[u], pv[u], w), reinterpret_cast<ema_f4*>(e + (size_t)r * FIRA_D + lane * 4));
        }
    }
}

struct EmaRanges { int64_t lo[3], hi[3]; };       // what lies outside the two tables, ascending (empty ranges: lo == hi)

__global__ __launch_bounds__(256) void ema_rows_kernel(float* __restrict__ e, const float* __restrict__ p, int64_t off0, int64_t off1,
                                                       int rows0, int rows1, AdamRowsView vw0, AdamRowsView vw1, EmaRanges rg,
                                                       float w) {
    ema_table(e + off0, p + off0, rows0, vw0, w);
    ema_table(e + off1, p + off1, rows1, vw1, w);
    const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, stride = (int64_t)gridDim.x * 256;
#pragma unroll
    for (int k = 0; k < 3; ++k) ema_range(e + rg.lo[k], p + rg.lo[k], rg.hi[k] - rg.lo[k], w, tid, stride);
}

static int ema_weight_check(const char* who, float w) {
    FIRA_REQUIRE(isfinite(w) && w >= 0.0f && w <= 1.0f, "%s: w = %g outside [0, 1]", who, (double)w);
    return 0;
}

}  // namespace fira

extern "C" int fira_ema_update(void* stream, int64_t n, float* ema, const float* p, float w) {
    using namespace fira;
    FIRA_REQUIRE(n >= 1, "fira_ema_update: n = %lld, the range has at least one element", (long long)n);
    FIRA_REQUIRE(ema && p, "fira_ema_update: null pointer (ema or p)");
    FIRA_REQUIRE((((uintptr_t)ema | (uintptr_t)p) & 3u) == 0, "fira_ema_update: ema and p must be 4-byte aligned");
    FIRA_REQUIRE(p + n <= ema || ema + n <= p, "fira_ema_update: ema overlaps p");
    if (int rc = ema_weight_check("fira_ema_update", w)) return rc;
    const hipStream_t s = (hipStream_t)stream;
    ProfScope prof(s, PROF_ADAM, 0.0, 12.0 * (double)n);
    const int grid = (int)std::min<int64_t>(cdiv64(cdiv64(n, 4), 256 * 2), 256 * 8);
    hipLaunchKernelGGL(ema_kernel, dim3(grid), dim3(256), 0, s, n, ema, p, w);
    FIRA_CHECK_LAUNCH("fira_ema_update");
    return 0;
}

extern "C" int fira_ema_update_rows(void* stream, const fira_dims* d, float* ema, const float* params, const fira_adam_opts* adam,
                                    const int32_t* row_step, float w) {
    using namespace fira;
    const Layout* L = get_layout(d);
    if (!L) return 1;
    FIRA_REQUIRE(ema && params && adam && adam->m && adam->v && row_step && adam->step >= 0, "fira_ema_update_rows: bad argument");
    FIRA_REQUIRE(L->d.d_model == FIRA_D, "fira_ema_update_rows: model width must be %d", FIRA_D);
    FIRA_REQUIRE((((uintptr_t)ema | (uintptr_t)params | (uintptr_t)adam->m | (uintptr_t)adam->v) & 15u) == 0,
                 "fira_ema_update_rows: ema, params and the moments must be 16-byte aligned");
    FIRA_REQUIRE(params + L->total <= ema || ema + L->total <= params, "fira_ema_update_rows: ema overlaps params");
    FIRA_REQUIRE((adam->m + L->total <= ema || ema + L->total <= adam->m) && (adam->v + L->total <= ema || ema + L->total <= adam->v),
                 "fira_ema_update_rows: ema overlaps the moments");
    if (adam->sched) { if (int rc = fira_lr_schedule_check(adam->sched)) return rc; }
    if (int rc = ema_weight_check("fira_ema_update_rows", w)) return rc;
    // the tables as every row-sparse entry sees them (engine.hip: adam_rows_tables); only the view is built from them, and the
    // view is read-only
    AdamRowsTables tb;
    tb.p = const_cast<float*>(params); tb.m = adam->m; tb.v = adam->v;
    tb.off[0] = L->dec_emb; tb.off[1] = L->emb;
    tb.rows[0] = tb.rows[1] = L->d.vocab;
    tb.last = const_cast<int32_t*>(row_step);
    const int64_t len = (int64_t)L->d.vocab * FIRA_D;
    const int a = tb.off[0] <= tb.off[1] ? 0 : 1, b = 1 - a;                    // the tables in address order
    FIRA_REQUIRE(tb.off[a] >= 0 && tb.off[a] + len <= tb.off[b] && tb.off[b] + len <= L->total && tb.off[0] % 4 == 0 && tb.off[1] % 4 == 0,
                 "fira_ema_update_rows: the embedding tables do not fit the layout");
    EmaRanges rg;
    rg.lo[0] = 0;                rg.hi[0] = tb.off[a];
    rg.lo[1] = tb.off[a] + len;  rg.hi[1] = tb.off[b];
    rg.lo[2] = tb.off[b] + len;  rg.hi[2] = L->total;
    const AdamLr lr = adam_lr(*adam);
    const AdamRowsView vw0 = adam_rows_view(tb, 0, lr, adam->beta1, adam->beta2, adam->eps, adam->step);
    const AdamRowsView vw1 = adam_rows_view(tb, 1, lr, adam->beta1, adam->beta2, adam->eps, adam->step);
    const hipStream_t s = (hipStream_t)stream;
    ProfScope prof(s, PROF_ADAM, 0.0, 12.0 * (double)L->total);
    hipLaunchKernelGGL(ema_rows_kernel, dim3(256 * 8), dim3(256), 0, s, ema, params, tb.off[0], tb.off[1], tb.rows[0], tb.rows[1], vw0,
                       vw1, rg, w);
    FIRA_CHECK_LAUNCH("fira_ema_update_rows");
    return 0;
}
