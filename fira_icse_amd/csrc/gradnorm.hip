// Gradient clipping by the global norm, on the device (torch.nn.utils.clip_grad_norm_ around run_model.py:108-111) and the
// guard against non-finite gradients.  With g the loss-SUM gradient and inv = 1 / max(n_tok, 1) the token normaliser:
//     norm = inv * sqrt(sum g_i^2) ;  coef = min(1, C / (norm + 1e-6)) ;  Adam sees g_i * inv * coef
// and a step whose norm is not finite -- an inf / nan element, or a sum of squares that overflows fp32 (an element above about
// 1.8e19: torch's fp32 norm overflows alike) -- is applied as a ZERO-GRADIENT step.  Three pieces:
//   grad_sqsum_kernel        sum of squares of a contiguous fp32 range: one partial per workgroup into caller scratch
//   grad_sqsum_close_kernel  the partials summed in a fixed order (double), optionally followed by the closing step
//   clip_finish              {norm, coef, zero_flag} + counters into fira_clip_state: the Adam kernels read two scalars
// and the clipped forms of the dense and the row-sparse Adam kernels (adam_elem itself is shared: adam_rows.h).
//
// Summation order and accuracy of grad_sqsum.  The range is cut into float4 quads; workgroup b owns the contiguous slice
// [b * slice4, (b + 1) * slice4) of them, slice4 = roundup(ceil(n4 / 1024), 1024) quads (n4 = n / 4), so the grid has at most
// 1024 workgroups and depends on n alone.  A lane runs iters = slice4 / 1024 trips of four independent 16-byte loads, each
// component accumulated by one fused multiply-add into its own accumulator (16 per lane); then a 4-level tree over the 16
// accumulators, the n % 4 tail elements (lanes 0..2 of workgroup 0, one more fused multiply-add), the 6-level DPP wave tree, and
// from there double precision: the four wave sums of a workgroup, the <= 1024 workgroup partials in a fixed order (the closing
// launch: thread t adds partials t, t + 256, ..., then a tree over the 256 threads), rounded to fp32 once.  Nothing depends
// on the order in which workgroups arrive: same bits on every run and replay.
// All terms are non-negative, so the relative error is at most (D + 1) * 2^-24 with D the number of fp32 roundings a value can
// pass through:
//     D(n) = iters + 4 + 1 + 6 + 1 ,   iters = roundup(ceil((n / 4) / 1024), 1024) / 1024
// D = 19 for the 27.8 M live parameters of the model (iters = 7); D = 524 for the largest supported n = 2^31 - 1 (iters = 512).
#include "adam_rows.h"
#include <math.h>
#include <algorithm>

namespace fira {

constexpr int SQ_GRID_MAX = 1024;      // workgroups (= partials) per range
constexpr int SQ_UNROLL = 4;           // 16-byte loads in flight per lane
constexpr int SQ_SLOTS = 4;            // ranges whose sums one fira_clip_state holds
constexpr int SQ_TRIP = 256 * SQ_UNROLL;

__global__ __launch_bounds__(256) void grad_sqsum_kernel(int64_t n, const float* __restrict__ g, int64_t slice4, int iters,
                                                         double* __restrict__ part) {
    const int tid = threadIdx.x;
    const int64_t n4 = n >> 2;
    const float4* __restrict__ g4 = reinterpret_cast<const float4*>(g);
    const int64_t lo = (int64_t)blockIdx.x * slice4 + tid;
    float4 acc[SQ_UNROLL];
#pragma unroll
    for (int u = 0; u < SQ_UNROLL; ++u) acc[u] = make_float4(0.f, 0.f, 0.f, 0.f);
    // (iters is 0 when the range holds no whole quad: no load is issued at all)
    for (int it = 0; it < iters; ++it) {
        float4 x[SQ_UNROLL];
        bool ok[SQ_UNROLL];
        // every load is issued unconditionally at a clamped index; what lies past the range is dropped by a select afterwards
#pragma unroll
        for (int u = 0; u < SQ_UNROLL; ++u) {
            const int64_t i = lo + (int64_t)(it * SQ_UNROLL + u) * 256;
            ok[u] = i < n4;
            x[u] = g4[ok[u] ? i : n4 - 1];
        }
        // (the compiler otherwise sinks a load under the `ok` test of its select, with a full vmcnt wait inside the branch:
        //  the four requests must be in flight together)
#pragma unroll
        for (int u = 0; u < SQ_UNROLL; ++u) asm volatile("" : "+v"(x[u].x), "+v"(x[u].y), "+v"(x[u].z), "+v"(x[u].w));
#pragma unroll
        for (int u = 0; u < SQ_UNROLL; ++u) {
            const float4 v = ok[u] ? x[u] : make_float4(0.f, 0.f, 0.f, 0.f);
            acc[u].x = __builtin_fmaf(v.x, v.x, acc[u].x);
            acc[u].y = __builtin_fmaf(v.y, v.y, acc[u].y);
            acc[u].z = __builtin_fmaf(v.z, v.z, acc[u].z);
            acc[u].w = __builtin_fmaf(v.w, v.w, acc[u].w);
        }
    }
    const float4 a = make_float4((acc[0].x + acc[1].x) + (acc[2].x + acc[3].x), (acc[0].y + acc[1].y) + (acc[2].y + acc[3].y),
                                 (acc[0].z + acc[1].z) + (acc[2].z + acc[3].z), (acc[0].w + acc[1].w) + (acc[2].w + acc[3].w));
    float sum = (a.x + a.y) + (a.z + a.w);
    if (blockIdx.x == 0 && tid < (int)(n & 3)) {          // the n % 4 tail: at most three elements
        const float t = g[(n4 << 2) + tid];
        sum = __builtin_fmaf(t, t, sum);
    }
    sum = wave_sum(sum);
    __shared__ double sh[4];
    if ((tid & 63) == 0) sh[tid >> 6] = (double)sum;
    __syncthreads();
    if (tid == 0) part[blockIdx.x] = ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

// One thread: the norm of the ranges sq[0 .. n_slots), the clip coefficient, the zero-gradient flag and the counters.
__device__ __forceinline__ void clip_finish_dev(fira_clip_state* __restrict__ st, const ClipClose& f) {
    double tot = 0.0;
    for (int k = 0; k < f.n_slots; ++k) tot += (double)st->sq[k];
    float scale;                                           // formed exactly as the Adam kernels form it
    if (f.count) scale = 1.0f / fmaxf(*f.count, 1.0f);
    else { const int nt = *f.n_tok; scale = 1.0f / (float)(nt > 0 ? nt : 1); }
    const float norm = (float)((double)scale * sqrt(tot));
    const bool finite = isfinite(norm);
    const float coef = finite ? fminf(1.0f, f.max_norm / (norm + 1e-6f)) : 1.0f;
    st->norm = norm;
    st->coef = coef;
    st->zero_flag = finite ? 0 : 1;
    if (!finite) st->n_nonfinite += 1;
    else if (coef < 1.0f) st->n_clipped += 1;
}

__global__ __launch_bounds__(256) void grad_sqsum_close_kernel(const double* __restrict__ part, int n_part,
                                                               fira_clip_state* __restrict__ st, int slot, ClipClose fin,
                                                               int do_finish) {
    __shared__ double sh[256];
    const int tid = threadIdx.x;
    double a = 0.0;
    for (int i = tid; i < n_part; i += 256) a += part[i];
    sh[tid] = a;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) sh[tid] += sh[tid + w];
        __syncthreads();
    }
    if (tid == 0) {
        st->sq[slot] = (float)sh[0];
        if (do_finish) clip_finish_dev(st, fin);
    }
}

__global__ void clip_finish_kernel(fira_clip_state* __restrict__ st, ClipClose fin) { clip_finish_dev(st, fin); }

// ------------------------------------------------------------------------------------------------
// adam_kernel (count form) / adam_mb_kernel (one gradient buffer) of copyhead.hip with the clip state: the gradient is
// g * inv * coef -- with coef == 1 the bits of the unclipped kernels -- or exactly 0 under the zero-gradient flag (a select:
// 0 * nan is nan).
__global__ __launch_bounds__(256) void adam_clip_kernel(int64_t n, float* __restrict__ p, const float* __restrict__ g,
                                                        float* __restrict__ m, float* __restrict__ v, float lr, float beta1,
                                                        float beta2, float eps, float bc1, float bc2_sqrt,
                                                        const int32_t* __restrict__ n0, const float* __restrict__ count,
                                                        const fira_clip_state* __restrict__ st) {
#pragma clang fp contract(off)
    float scale;
    if (count) scale = 1.0f / fmaxf(*count, 1.0f);
    else { const int nt = *n0; scale = 1.0f / (float)(nt > 0 ? nt : 1); }
    const float coef = st->coef;
    const bool zf = st->zero_flag != 0;
    const int64_t stride = (int64_t)gridDim.x * 256;
    const float step_size = lr / bc1;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        const float gi = g[i] * scale * coef;
        adam_elem(p[i], m[i], v[i], zf ? 0.f : gi, beta1, beta2, eps, step_size, bc2_sqrt);
    }
}

// adam_rows_kernel of copyhead.hip with the clip state.  Under the zero-gradient flag every row is "untouched" (wave-uniform:
// the flag is one scalar), and a forced step applies the zero-gradient update gz to every row -- what the dense clipped kernel
// does to every element, so the two stay equal bit for bit once fira_adam_rows_sync has run.
__global__ __launch_bounds__(256) void adam_rows_clip_kernel(AdamRowsTables tb, const float* __restrict__ gbase,
                                                             float beta1, float beta2, float eps, int step, AdamRowsHist h,
                                                             const int32_t* __restrict__ n0, const float* __restrict__ count,
                                                             int force, float gz, int it_lo, int it_hi,
                                                             const fira_clip_state* __restrict__ st) {
#pragma clang fp contract(off)
    float scale;
    if (count) scale = 1.0f / fmaxf(*count, 1.0f);
    else { const int nt = *n0; scale = 1.0f / (float)(nt > 0 ? nt : 1); }
    const float coef = st->coef;
    const bool zf = st->zero_flag != 0;
    const int lane = threadIdx.x & 63;
    const int nw = gridDim.x * 4;
    const int total = it_hi;
    const float ss = h.lr[step % ADAM_ROWS_K] / h.bc1[step % ADAM_ROWS_K], b2s = h.bc2s[step % ADAM_ROWS_K];
    for (int it0 = it_lo + (blockIdx.x * 4 + (threadIdx.x >> 6)) * 4; it0 < total; it0 += nw * 4) {
        float4 gq[4];
        size_t oq[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int it = min(it0 + u, total - 1);
            const int t = it >= tb.rows[0] ? 1 : 0;
            oq[u] = (size_t)tb.off[t] + (size_t)(it - (t ? tb.rows[0] : 0)) * 256 + lane * 4;
            gq[u] = *reinterpret_cast<const float4*>(gbase + oq[u]);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int it = it0 + u;
            if (it >= total) break;
            const float4 gv = gq[u];
            const size_t o = oq[u];
            const bool nz = !zf && (gv.x != 0.f || gv.y != 0.f || gv.z != 0.f || gv.w != 0.f);
            if (!force && !__any(nz)) continue;           // wave-uniform: the row waits for its next reader
            const int l = max(tb.last[it], step - ADAM_ROWS_K);
            float4 pv = *reinterpret_cast<float4*>(tb.p + o), mv = *reinterpret_cast<float4*>(tb.m + o),
                   vv = *reinterpret_cast<float4*>(tb.v + o);
            adam_row_zero_steps(pv, mv, vv, l + 1, step - 1, gz, beta1, beta2, eps, h);
            const float gx = gv.x * scale * coef, gy = gv.y * scale * coef, gzz = gv.z * scale * coef, gw = gv.w * scale * coef;
            adam_elem(pv.x, mv.x, vv.x, zf ? gz : gx, beta1, beta2, eps, ss, b2s);
            adam_elem(pv.y, mv.y, vv.y, zf ? gz : gy, beta1, beta2, eps, ss, b2s);
            adam_elem(pv.z, mv.z, vv.z, zf ? gz : gzz, beta1, beta2, eps, ss, b2s);
            adam_elem(pv.w, mv.w, vv.w, zf ? gz : gw, beta1, beta2, eps, ss, b2s);
            *reinterpret_cast<float4*>(tb.p + o) = pv;
            *reinterpret_cast<float4*>(tb.m + o) = mv;
            *reinterpret_cast<float4*>(tb.v + o) = vv;
            if (lane == 0) tb.last[it] = step;
        }
    }
}

// ------------------------------------------------------------------------------------------------ launchers
size_t grad_sqsum_scratch_bytes() { return (size_t)SQ_SLOTS * SQ_GRID_MAX * sizeof(double); }

static int clip_close_check(const ClipClose& fin, const char* who) {
    FIRA_REQUIRE(fin.n_slots >= 1 && fin.n_slots <= SQ_SLOTS, "%s: n_slots must be 1..%d", who, SQ_SLOTS);
    FIRA_REQUIRE(fin.n_tok || fin.count, "%s: n_tok or count is required", who);
    FIRA_REQUIRE(fin.max_norm > 0.f, "%s: max_norm must be > 0 (inf allowed)", who);      // (false for nan)
    return 0;
}

int grad_sqsum(hipStream_t s, int64_t n, const float* g, fira_clip_state* st, int slot, void* scratch, const ClipClose* fin) {
    FIRA_REQUIRE(st && scratch && slot >= 0 && slot < SQ_SLOTS, "grad_sqsum: bad state / scratch / slot");
    FIRA_REQUIRE(n >= 0 && n <= 2147483647LL && (n == 0 || g), "grad_sqsum: bad range");
    FIRA_REQUIRE((uintptr_t)g % 16 == 0 && (uintptr_t)scratch % 8 == 0, "grad_sqsum: the range must be 16-byte aligned");
    if (fin) { if (int rc = clip_close_check(*fin, "grad_sqsum")) return rc; }
    // (profiling: booked in the optimizer class, PROF_ADAM -- with clipping on, that class's time includes the norm pass)
    ProfScope prof(s, PROF_ADAM, 0.0, (double)n * 4.0);
    double* part = static_cast<double*>(scratch) + (size_t)slot * SQ_GRID_MAX;
    int grid = 0;
    if (n > 0) {
        const int64_t n4 = n >> 2;
        const int64_t slice4 = cdiv64(cdiv64(n4, SQ_GRID_MAX), SQ_TRIP) * SQ_TRIP;      // 0 when the range holds no whole quad
        grid = n4 ? (int)cdiv64(n4, slice4) : 1;
        hipLaunchKernelGGL(grad_sqsum_kernel, dim3(grid), dim3(256), 0, s, n, g, slice4, (int)(slice4 / SQ_TRIP), part);
        FIRA_CHECK_LAUNCH("grad_sqsum");
    }
    hipLaunchKernelGGL(grad_sqsum_close_kernel, dim3(1), dim3(256), 0, s, part, grid, st, slot, fin ? *fin : ClipClose{}, fin ? 1 : 0);
    FIRA_CHECK_LAUNCH("grad_sqsum_close");
    return 0;
}

int clip_finish(hipStream_t s, fira_clip_state* st, const ClipClose& fin) {
    FIRA_REQUIRE(st, "clip_finish: state missing");
    if (int rc = clip_close_check(fin, "clip_finish")) return rc;
    hipLaunchKernelGGL(clip_finish_kernel, dim3(1), dim3(1), 0, s, st, fin);
    FIRA_CHECK_LAUNCH("clip_finish");
    return 0;
}

int adam_step_clip(hipStream_t s, int64_t n, float* p, const float* g, float* m, float* v, float lr, float beta1, float beta2,
                   float eps, int step, const int32_t* n0, const float* count, const fira_clip_state* st) {
    ProfScope prof(s, PROF_ADAM, 0.0);
    if (n <= 0) return 0;
    FIRA_REQUIRE(step >= 1 && st && (n0 || count), "adam_step_clip: bad argument");
    const double bc1 = 1.0 - pow((double)beta1, step);          // as adam_step / adam_step_mb form them
    const double bc2 = 1.0 - pow((double)beta2, step);
    const int grid = (int)std::min<int64_t>(cdiv64(n, 256), 256 * 16);
    hipLaunchKernelGGL(adam_clip_kernel, dim3(grid), dim3(256), 0, s, n, p, g, m, v, lr, beta1, beta2, eps, (float)bc1,
                       (float)sqrt(bc2), count ? nullptr : n0, count, st);
    FIRA_CHECK_LAUNCH("adam_step_clip");
    return 0;
}

int adam_rows_step_clip(hipStream_t s, const AdamRowsTables& tb, const float* g, const AdamLr& lr, float beta1, float beta2, float eps,
                        int step, const int32_t* n0, const float* count, int tables, const fira_clip_state* st) {
    ProfScope prof(s, PROF_ADAM, 0.0);
    FIRA_REQUIRE(step >= 1 && tb.last && (n0 || count) && st, "adam_rows_step_clip: bad argument");
    const int it_lo = (tables & 1) ? 0 : tb.rows[0], it_hi = (tables & 2) ? tb.rows[0] + tb.rows[1] : tb.rows[0];
    const int total = it_hi - it_lo;
    if (total <= 0) return 0;
    const int grid = std::min(cdiv(total, 16), 256 * 8);
    hipLaunchKernelGGL(adam_rows_clip_kernel, dim3(grid), dim3(256), 0, s, tb, g, beta1, beta2, eps, step,
                       adam_rows_hist(lr, beta1, beta2, step), count ? nullptr : n0, count, step % ADAM_ROWS_K == 0 ? 1 : 0, 0.0f,
                       it_lo, it_hi, st);
    FIRA_CHECK_LAUNCH("adam_rows_step_clip");
    return 0;
}

}  // namespace fira

extern "C" {
size_t fira_grad_sqsum_scratch_bytes(void) { return fira::grad_sqsum_scratch_bytes(); }
int fira_grad_sqsum(void* stream, int64_t n, const float* g, fira_clip_state* state, int slot, void* scratch) {
    return fira::grad_sqsum((hipStream_t)stream, n, g, state, slot, scratch, nullptr);
}
int fira_clip_finish(void* stream, fira_clip_state* state, int n_slots, const int32_t* n_tok, const float* count,
                     float max_norm) {
    fira::ClipClose fin{n_tok, count, max_norm, n_slots};
    return fira::clip_finish((hipStream_t)stream, state, fin);
}
int fira_adam_step_clip(void* stream, int64_t n, float* p, const float* g, float* m, float* v, float lr, float beta1,
                        float beta2, float eps, int step, const int32_t* n_tok, const float* count,
                        const fira_clip_state* state) {
    FIRA_REQUIRE(p && g && m && v && (n_tok || count) && state && step >= 1, "fira_adam_step_clip: bad argument");
    return fira::adam_step_clip((hipStream_t)stream, n, p, g, m, v, lr, beta1, beta2, eps, step, n_tok, count, state);
}
}
