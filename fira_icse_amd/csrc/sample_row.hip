// Sampling from a distribution row that already exists in memory: the sampler's filters, cuts and Gumbel-max draw
// (sample.hip) applied to dist[r, 0 .. V + S) as the step, the mixing kernels and the edit chain (fira_merge_dist,
// fira_force_dist, fira_constrain_dist) left it.  fira_sample_dist is what lets Searcher.sample_search draw from the search's
// edited distribution: step(s), mix, edit chain, THIS kernel, fira_sample_advance.
//
// One workgroup of 1024 threads per row.  The row sits in registers in WideRow's layout (decode_row.h): thread tid holds
// entries tid + 1024 i (i < 25) of the first V and entry V + tid of the S slots; positions past V or S hold -1, below every
// threshold.  It is loaded from dist + r (V + S) by 4-byte buffer loads (the generator part, 0 past V) and plain loads (the
// slots), so any 4-byte alignment of the row will do -- the stride V + S is odd for the project's geometry.  dist is only read.
//
// pmax is the block maximum of the row, NOT max(sg, sc) as in sample.hip: an edit may have zeroed the entry that held it.  On
// the rows of the fused sampler the two are the same float (its largest entry is exp(0) = 1 times its scale).
//
// Everything after the load is sample_dist_kernel's, expression for expression and in its order: top-k and top-p by bisection
// over float bits with block16_sum, the SampleCuts block, the drop mask, the Gumbel-max draw with noise_stream / gumbel_noise
// and block16_argmax.  On a row the fused sampler stored, this kernel takes the same thresholds and draws the same entry with
// the same best_p, bit for bit (tests/test_sample_search_gpu.py).  The code is a copy on purpose: sample.hip's plain instance
// must keep its gfx950 code instruction for instruction (the comment in its cuts block), so nothing of it moves into a shared
// helper; the ~120 duplicated lines are the price.
//
// Unnormalised rows (the edits renormalise nothing) need nothing more: every filter works relative to the row's own sums --
// need = top_p * (kept mass), q = w / Z, w relative to pmax.  An entry with p = 0 is never kept and never drawn; with fewer
// than top_k positive entries top-k cuts nothing (tau = 0).  best_p[r] is dist[r, best_id[r]] bit for bit: the edited,
// untempered, unfiltered value.
//
// A row without a positive entry: unlike the fused kernel, every row is written.  Such a row gets what the edit chain's ArgMax
// (decode_row.h) reports for an all-zero row -- every candidate ties at 0, the lowest index wins: best_id = 0, best_p = 0.0f.
// fira_sample_advance then carries probability 0 and log-probability -inf for the hypothesis.
//
// Contract: entries finite and non-negative.  On anything else the result is unspecified, but best_id stays inside [0, V + S)
// (only an entry that is > 0 inside the row is ever offered, else 0 is reported) and nothing but best_id / best_p is written;
// every bisection runs over integers and ends whatever the floats hold (pmax is formed from 0 upwards, so it is never NaN).
#include <float.h>
#include <math.h>
#include "engine.h"
#include "epilogue.h"
#include "decode_row.h"

namespace fira {

__device__ __forceinline__ int row16_min(int v, int* sm) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
    __syncthreads();
    int t = sm[0];
#pragma unroll
    for (int k = 1; k < DDW_NT / 64; ++k) t = min(t, sm[k]);
    return t;
}
__device__ __forceinline__ float row16_max(float v, float* sm) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
    __syncthreads();
    float t = sm[0];
#pragma unroll
    for (int k = 1; k < DDW_NT / 64; ++k) t = fmaxf(t, sm[k]);
    return t;
}

template <bool CUT>
__global__ __launch_bounds__(DDW_NT) void sample_row_kernel(int V, int S, const float* __restrict__ dist, int n_sample, int T,
                                                            int step, const int32_t* __restrict__ key,
                                                            const uint64_t* __restrict__ seed_dev, float inv_temp, int top_k,
                                                            float top_p, SampleCuts cut, int32_t* __restrict__ best_id,
                                                            float* __restrict__ best_p) {
    __shared__ float smf[DDW_NT / 64];
    __shared__ int smi[DDW_NT / 64];
    const int r = blockIdx.x, tid = threadIdx.x;
    const float* __restrict__ drow = dist + (size_t)r * (V + S);
    const rsrc_t rD = buf_rsrc(drow, (unsigned)V * 4u);
    float x[DDW_NPT];
#pragma unroll
    for (int i = 0; i < DDW_NPT; ++i) x[i] = buf_load_f32(rD, (unsigned)(tid + DDW_NT * i) * 4u);   // p of entry tid + 1024 i; past V: 0, replaced below
    float pc = tid < S ? drow[V + tid] : -1.f;               // p of entry V + tid
    // entries past V / S: p = -1, below every threshold t >= 0 (the bits of a non-negative float order like its value)
#pragma unroll
    for (int i = 0; i < DDW_NPT; ++i) x[i] = tid + DDW_NT * i < V ? x[i] : -1.f;
    float own_max = fmaxf(0.f, pc);                          // (from 0 upwards: never NaN, never below 0)
#pragma unroll
    for (int i = 0; i < DDW_NPT; ++i) own_max = fmaxf(own_max, x[i]);
    const float pmax = row16_max(own_max, smf);              // the largest entry of the row as it stands
    const int top = __float_as_int(pmax) + 1;               // #{p >= top} = 0
    // ---- top-k: the largest t with #{p_i >= t} >= k
    int tau = 0;
    if (top_k > 0) {
        int lo = 0, hi = top;                                // #{p >= 0} = V + S >= k (checked by the caller), #{p >= hi} = 0 < k
        while (hi - lo > 1) {
            const int mid = lo + ((hi - lo) >> 1);
            int c = __float_as_int(pc) >= mid;
#pragma unroll
            for (int i = 0; i < DDW_NPT; ++i) c += __float_as_int(x[i]) >= mid;
            if (block16_sum((float)c, smf) >= (float)top_k) lo = mid; else hi = mid;
        }
        tau = lo;
    }
    // ---- top-p over the entries top-k kept: the largest t whose upper set holds at least top_p of their tempered mass
    if (top_p < 1.f) {
        const float lmax = log2f(pmax);
        float w[DDW_NPT];
        float m = 0.f;
#pragma unroll
        for (int i = 0; i < DDW_NPT; ++i) {
            w[i] = __float_as_int(x[i]) >= tau ? (inv_temp == 1.f ? x[i] : exp2f((log2f(x[i]) - lmax) * inv_temp)) : 0.f;
            m += w[i];
        }
        const float wc = __float_as_int(pc) >= tau ? (inv_temp == 1.f ? pc : exp2f((log2f(pc) - lmax) * inv_temp)) : 0.f;
        m += wc;
        const float need = top_p * block16_sum(m, smf);      // mass(>= tau) = the whole kept mass >= need
        int lo = tau, hi = top;                              // mass(>= hi) = 0 < need
        while (hi - lo > 1) {
            const int mid = lo + ((hi - lo) >> 1);
            float s = 0.f;
#pragma unroll
            for (int i = 0; i < DDW_NPT; ++i) s += __float_as_int(x[i]) >= mid ? w[i] : 0.f;
            s += __float_as_int(pc) >= mid ? wc : 0.f;
            if (block16_sum(s, smf) >= need) lo = mid; else hi = mid;
        }
        tau = lo;
    }
    int drop = 0;                                            // bit i: x[i] (bit 25: pc) lies outside the typical band
    if constexpr (CUT) {
        // ---- the cuts, on q = w / Z over what top-k and top-p kept (w as top-p's block above forms it, now over the final tau)
        const float lmax = log2f(pmax), wmax = inv_temp == 1.f ? pmax : 1.f;
        const bool typical = cut.typical_p < 1.f;
        float w[DDW_NPT];
        float m = 0.f;
#pragma unroll
        for (int i = 0; i < DDW_NPT; ++i) {
            w[i] = __float_as_int(x[i]) >= tau ? (inv_temp == 1.f ? x[i] : exp2f((log2f(x[i]) - lmax) * inv_temp)) : 0.f;
            m += w[i];
        }
        const float wc = __float_as_int(pc) >= tau ? (inv_temp == 1.f ? pc : exp2f((log2f(pc) - lmax) * inv_temp)) : 0.f;
        m += wc;
        const float Z = block16_sum(m, smf);
        float wlw = 0.f;                                     // sum(w ln w) / Z = ln Z - H
        if (typical || cut.eta > 0.f) {
            float e = 0.f;
#pragma unroll
            for (int i = 0; i < DDW_NPT; ++i) e += w[i] > 0.f ? w[i] * logf(w[i]) : 0.f;
            e += wc > 0.f ? wc * logf(wc) : 0.f;
            wlw = block16_sum(e, smf) / Z;
        }
        if (!typical) {
            // lower thresholds on w; sqrt(eta) e^-H Z = sqrt(eta) e^(wlw) (e^-H = e^(wlw) / Z)
            float thr = fmaxf(cut.min_p * wmax, cut.epsilon * Z);
            if (cut.eta > 0.f) thr = fmaxf(thr, fminf(cut.eta * Z, sqrtf(cut.eta) * expf(wlw)));
            thr = fminf(thr, wmax);
            int lowest = __float_as_int(pmax);
#pragma unroll
            for (int i = 0; i < DDW_NPT; ++i) lowest = w[i] > 0.f && w[i] >= thr ? min(lowest, __float_as_int(x[i])) : lowest;
            lowest = wc > 0.f && wc >= thr ? min(lowest, __float_as_int(pc)) : lowest;
            tau = max(tau, row16_min(lowest, smi));          // (a threshold that rounds to 0 cuts nothing: tau only rises)
        } else {
            int sb[DDW_NPT];                                 // the bits of s_i; entries without weight: above every sigma
#pragma unroll
            for (int i = 0; i < DDW_NPT; ++i) sb[i] = w[i] > 0.f ? __float_as_int(fabsf(wlw - logf(w[i]))) : 0x7fffffff;
            const int sbc = wc > 0.f ? __float_as_int(fabsf(wlw - logf(wc))) : 0x7fffffff;
            const float need = fmaxf(cut.typical_p * Z, FLT_MIN);
            int lo = -1, hi = 0x7f800000;                    // mass(s <= -1) = 0 < need, mass(s <= inf) = Z >= need
            while (hi - lo > 1) {
                const int mid = lo + ((hi - lo) >> 1);
                float s = 0.f;
#pragma unroll
                for (int i = 0; i < DDW_NPT; ++i) s += sb[i] <= mid ? w[i] : 0.f;
                s += sbc <= mid ? wc : 0.f;
                if (block16_sum(s, smf) >= need) hi = mid; else lo = mid;
            }
#pragma unroll
            for (int i = 0; i < DDW_NPT; ++i) drop |= (sb[i] > hi && x[i] < pmax) ? 1 << i : 0;
            drop |= (sbc > hi && pc < pmax) ? 1 << DDW_NPT : 0;
        }
    }
    // ---- Gumbel-max over the kept entries (p = 0 entries have score -inf and are skipped)
    const uint64_t seed = *seed_dev;
    const int b = r / n_sample, jsample = r - b * n_sample;
    const uint32_t stream = noise_stream((uint32_t)key[b], seed, jsample, T, step);
    float best = -INFINITY, bp_own = 0.f;
    int bi = 0x7fffffff;
#pragma unroll
    for (int i = 0; i < DDW_NPT; ++i) {                      // ascending index within the thread: the first maximum wins
        if (__float_as_int(x[i]) >= tau && x[i] > 0.f && !(CUT && (drop >> i & 1))) {
            const int j = tid + DDW_NT * i;
            const float sc_i = logf(x[i]) * inv_temp + gumbel_noise(stream, (uint32_t)j);
            if (sc_i > best) { best = sc_i; bi = j; bp_own = x[i]; }
        }
    }
    if (__float_as_int(pc) >= tau && pc > 0.f && !(CUT && (drop >> DDW_NPT & 1))) {
        const float sc_c = logf(pc) * inv_temp + gumbel_noise(stream, (uint32_t)(V + tid));
        if (sc_c > best) { best = sc_c; bi = V + tid; bp_own = pc; }
    }
    const int own = bi;
    block16_argmax(best, bi, smf, smi);
    if (bi == 0x7fffffff) {                                  // no positive entry: ArgMax's report for an all-zero row
        if (tid == 0) { best_id[r] = 0; best_p[r] = 0.f; }
    } else if (own == bi) {                                  // the owner of the winning entry reports it
        best_id[r] = bi;
        best_p[r] = bp_own;
    }
}

}  // namespace fira

extern "C" int fira_sample_dist(void* stream, const fira_dims* d, int R, int rows_per_commit, int step, const float* dist,
                                const int32_t* key, const uint64_t* seed_dev, float temperature, int top_k, float top_p,
                                float min_p, float epsilon, float eta, float typical_p, int32_t* best_id, float* best_p) {
    using namespace fira;
    const char* who = "fira_sample_dist";
    if (int e = require_row_geometry(d, rows_per_commit, R, best_id, best_p, who)) return e;
    FIRA_REQUIRE(best_id && best_p, "%s: best_id and best_p are required", who);
    FIRA_REQUIRE(rows_per_commit <= 8, "%s: rows_per_commit = %d outside 1..8", who, rows_per_commit);
    FIRA_REQUIRE(step >= 0, "%s: step = %d is negative", who, step);
    FIRA_REQUIRE(temperature > 0.f && temperature < INFINITY, "%s: temperature %g must be finite and > 0", who,
                 (double)temperature);
    const int V = d->vocab, S = d->sou_len + d->sub_len;
    FIRA_REQUIRE(top_k >= 0 && top_k <= V + S, "%s: top_k %d outside 0..%d", who, top_k, V + S);
    FIRA_REQUIRE(top_p > 0.f && top_p <= 1.f, "%s: top_p %g outside (0, 1]", who, (double)top_p);
    // (every comparison also refuses nan)
    FIRA_REQUIRE(min_p >= 0.f && min_p < 1.f, "%s: min_p %g outside [0, 1)", who, (double)min_p);
    FIRA_REQUIRE(epsilon >= 0.f && epsilon < 1.f, "%s: epsilon %g outside [0, 1)", who, (double)epsilon);
    FIRA_REQUIRE(eta >= 0.f && eta < 1.f, "%s: eta %g outside [0, 1)", who, (double)eta);
    FIRA_REQUIRE(typical_p > 0.f && typical_p <= 1.f, "%s: typical_p %g outside (0, 1]", who, (double)typical_p);
    if (typical_p < 1.f) {                                   // a band in p, not a lower threshold: temperature and top-k only
        FIRA_REQUIRE(top_p == 1.f, "%s: typical_p %g does not combine with top_p %g", who, (double)typical_p, (double)top_p);
        FIRA_REQUIRE(min_p == 0.f, "%s: typical_p %g does not combine with min_p %g", who, (double)typical_p, (double)min_p);
        FIRA_REQUIRE(epsilon == 0.f, "%s: typical_p %g does not combine with epsilon %g", who, (double)typical_p, (double)epsilon);
        FIRA_REQUIRE(eta == 0.f, "%s: typical_p %g does not combine with eta %g", who, (double)typical_p, (double)eta);
    }
    if (R == 0) return 0;
    FIRA_REQUIRE(dist && key && seed_dev, "%s: null pointer (dist, key or seed_dev)", who);
    SampleCuts cut;
    cut.min_p = min_p; cut.epsilon = epsilon; cut.eta = eta; cut.typical_p = typical_p;
    const hipStream_t s = (hipStream_t)stream;
    const SampleCuts off;
    if (cut.on())
        hipLaunchKernelGGL(sample_row_kernel<true>, dim3(R), dim3(DDW_NT), 0, s, V, S, dist, rows_per_commit, d->tar_len, step, key,
                           seed_dev, 1.0f / temperature, top_k, top_p, cut, best_id, best_p);
    else                                                     // every cut off: the plain instance, as sample_dist chooses
        hipLaunchKernelGGL(sample_row_kernel<false>, dim3(R), dim3(DDW_NT), 0, s, V, S, dist, rows_per_commit, d->tar_len, step,
                           key, seed_dev, 1.0f / temperature, top_k, top_p, off, best_id, best_p);
    FIRA_CHECK_LAUNCH(who);
    return 0;
}
