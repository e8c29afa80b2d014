// On-device sampling of the decode step's output distribution: temperature, top-k and top-p, drawn by Gumbel-max.
//
// One workgroup of 1024 threads per (commit, sample) row.  The row is WideRow (decode_row.h), the distribution p over V + S
// entries that fira_decode_step writes; the optional `dist` row is stored from it.  What this kernel adds:
//   top-k   tau_k = the k-th largest p counted with multiplicity: the largest t with #{p_i >= t} >= k
//   top-p   over the entries top-k kept, w_i = p_i^(1/T) (relative to the row's maximum); tau_p = the largest t with
//           sum{w_i : p_i >= t} >= top_p * sum{w_i}; both thresholds live in p-space (p -> p^(1/T) is monotone), and
//           tau_p >= tau_k, so ONE threshold decides what is kept; ties at it are kept
//   draw    i* = argmax over kept i of (log p_i / T + g_i), g_i Gumbel noise of a counter hash; ties to the lowest index
// Both searches bisect over the bits of a non-negative float (ordered like the values): ~30 rounds of a block sum each.
// Counts are sums of small integers (exact in fp32); masses are fp32 sums in one fixed order (block16_sum: per-thread
// ascending index, then the DPP tree, then the 16 wave partials in order) -- no atomics, so every run and every graph
// replay takes the same thresholds.  A fixed-order sum of non-negative terms is monotone in each term, so the bisection's
// predicate is monotone in t.
//
// The truncation cuts of fira_decode_step_sample_cut (SampleCuts; the second instance of the kernel, the first one is the
// plain sampler and is what a call with every cut off launches).  q = w / Z, w the tempered weights top-p uses, over what
// top-k and top-p kept, Z their block sum; H = ln Z - sum(w ln w) / Z, one more block sum.
//   min_p / epsilon / eta   lower thresholds on q, compared as w_i >= max(min_p wmax, epsilon Z, min(eta, sqrt(eta) e^-H) Z)
//           (capped at wmax: the maximum stays); the lowest p that passes becomes THE threshold (one block minimum), so still
//           one threshold decides what is kept and ties at it are kept.  No bisection.
//   typical s_i = |-ln q_i - H| = |sum(w ln w) / Z - ln w_i|; sigma = the smallest t with sum{w_i : s_i <= t} >= typical_p Z by
//           the same bisection over the bits of s (31 rounds of a block sum).  A band in p, not a threshold: the entries
//           outside it are marked in one bit each of a per-thread mask that the draw consults.  The maximum stays.
#include <float.h>
#include "engine.h"
#include "epilogue.h"
#include "decode_row.h"

namespace fira {

__device__ __forceinline__ int block16_min(int v, int* sm) {
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

template <bool CUT>
__global__ __launch_bounds__(DDW_NT) void sample_dist_kernel(int V, int S, const float* __restrict__ logits, int ldl,
                                                             const float* __restrict__ score,
                                                             const int32_t* __restrict__ mem_valid, int n_sample,
                                                             const float* __restrict__ xrow, const float* __restrict__ wp,
                                                             const float* __restrict__ bp, int T, int step,
                                                             const int32_t* __restrict__ key,
                                                             const uint64_t* __restrict__ seed_dev, float inv_temp,
                                                             int top_k, float top_p, SampleCuts cut,
                                                             float* __restrict__ dist, int32_t* __restrict__ best_id,
                                                             float* __restrict__ best_p) {
    __shared__ float smf[DDW_NT / 64];
    __shared__ int smi[DDW_NT / 64];
    const int r = blockIdx.x, tid = threadIdx.x;
    WideRow row;
    row.form(V, S, logits + (size_t)r * ldl, score + (size_t)r * S, mem_valid + (size_t)(r / n_sample) * S, r, nullptr, xrow, wp,
             bp, smf, smi);
    if (dist) row.store(dist + (size_t)r * (V + S), V, S);
    const float sg = row.sg, sc = row.sc;
    float(&x)[DDW_NPT] = row.x;
#pragma unroll
    for (int i = 0; i < DDW_NPT; ++i) x[i] = sg * x[i];      // p of entry tid + 1024 i
    float pc = sc * row.ce;                                  // p of entry V + tid
    // entries past V / S: p = -1, below every threshold t >= 0 (the bits of a non-negative float order like its value)
#pragma unroll
    for (int i = 0; i < DDW_NPT; ++i) x[i] = tid + DDW_NT * i < V ? x[i] : -1.f;
    pc = tid < S ? pc : -1.f;
    const float pmax = fmaxf(sg, sc);                        // the largest entry: exp(0) = 1 times its scale
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
        // ---- the cuts, on q = w / Z over what top-k and top-p kept
        // (w as top-p's block above forms it, now over the final tau.  That block stays as it is written: moving the two into
        // one inlined helper rewrites the plain instance's gfx950 code, which is the kernel's of before the cuts instruction
        // for instruction -- the plain sampler's bits must not move.)
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
            tau = max(tau, block16_min(lowest, smi));        // (a threshold that rounds to 0 cuts nothing: tau only rises)
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
    if (own == bi && bi != 0x7fffffff) {                     // the owner of the winning entry reports it
        best_id[r] = bi;
        best_p[r] = bp_own;
    }
}

int sample_dist(hipStream_t s, int R, int n_sample, int V, int S, const float* logits, int ldl, const float* score,
                const int32_t* mem_valid, const float* x, const float* wp, const float* bp, int T, int step,
                const int32_t* key, const uint64_t* seed_dev, float temperature, int top_k, float top_p, float* dist,
                int32_t* best_id, float* best_p, const SampleCuts* cut) {
    ProfScope prof(s, PROF_HEAD, 0.0);
    if (R <= 0) return 0;
    FIRA_REQUIRE(V <= ROW_MAX_V && S <= ROW_MAX_SLOTS,
                 "sample_dist: vocabulary %d / %d memory slots exceed the register-resident row (%d / %d)", V, S, ROW_MAX_V,
                 ROW_MAX_SLOTS);
    const SampleCuts off;
    if (cut && cut->on())
        hipLaunchKernelGGL(sample_dist_kernel<true>, dim3(R), dim3(DDW_NT), 0, s, V, S, logits, ldl, score, mem_valid, n_sample,
                           x, wp, bp, T, step, key, seed_dev, 1.0f / temperature, top_k, top_p, *cut, dist, best_id, best_p);
    else                                                     // every cut off: the plain sampler itself
        hipLaunchKernelGGL(sample_dist_kernel<false>, dim3(R), dim3(DDW_NT), 0, s, V, S, logits, ldl, score, mem_valid, n_sample,
                           x, wp, bp, T, step, key, seed_dev, 1.0f / temperature, top_k, top_p, off, dist, best_id, best_p);
    FIRA_CHECK_LAUNCH("sample_dist");
    return 0;
}

}  // namespace fira
