// The sampler body: what sample_dist_kernel (sample.hip, the row formed inside the step) and sample_row_kernel
// (sample_row.hip, the row loaded from memory) do once the row sits in registers -- top-k, top-p, the SampleCuts block, the
// drop mask and the Gumbel-max draw.  One body, so the two kernels take the same thresholds and draw the same entry with the
// same best_p on the same row, bit for bit, by construction.
//
// The row is in WideRow's layout (decode_row.h): thread tid holds entries tid + 1024 i (i < 25) of the first V in x[i] and entry
// V + tid of the S slots in pc; positions past V or S hold -1, below every threshold t >= 0 (the bits of a non-negative float
// order like its value).  pmax is the row's largest entry; the caller says how it knows it.
//
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
// The truncation cuts (SampleCuts; compiled in with CUT only).  q = w / Z, w the tempered weights top-p uses, over what top-k
// and top-p kept, Z their block sum; H = ln Z - sum(w ln w) / Z, one more block sum.
//   min_p / epsilon / eta   lower thresholds on q, compared as w_i >= max(min_p wmax, epsilon Z, min(eta, sqrt(eta) e^-H) Z)
//           (capped at wmax: the maximum stays); the lowest p that passes becomes THE threshold (one block minimum), so still
//           one threshold decides what is kept and ties at it are kept.  No bisection.
//   typical s_i = |-ln q_i - H| = |sum(w ln w) / Z - ln w_i|; sigma = the smallest t with sum{w_i : s_i <= t} >= typical_p Z by
//           the same bisection over the bits of s (31 rounds of a block sum).  A band in p, not a threshold: the entries
//           outside it are marked in one bit each of a per-thread mask that the draw consults.  The maximum stays.
#pragma once
#include <float.h>
#include <math.h>
#include "engine.h"
#include "decode_row.h"

namespace fira {

// What a thread knows after the draw: its own candidate, the block's winner (0x7fffffff: no positive entry was kept anywhere)
// and the probability of its own candidate.  The thread with own == win owns the winning entry.
struct SampleDraw {
    int own, win;
    float bp_own;
};

// r: the row (commit r / n_sample, sample r % n_sample of it); T, step, key, seed_dev: the noise coordinates (noise_stream).
template <bool CUT>
__device__ __forceinline__ SampleDraw sampler_draw(const float (&x)[DDW_NPT], float pc, float pmax, int V, int r, int n_sample,
                                                   int T, int step, const int32_t* __restrict__ key,
                                                   const uint64_t* __restrict__ seed_dev, float inv_temp, int top_k, float top_p,
                                                   const SampleCuts& cut, float* smf, int* smi) {
    const int tid = threadIdx.x;
    // The tempered weights of the entries at or above tau, relative to the row's maximum: w = p^(1/T) / pmax^(1/T) (p itself at
    // T = 1), 0 below tau; returns the thread's own sum, ascending index, the slot last.  top-p forms them over top-k's tau, the
    // cuts over the final one.  (A lambda: as a function of its own the same text timed 0.003 ms per step slower with top-k
    // and top-p on)
    auto tempered_weights = [&](int tau, float (&w)[DDW_NPT], float& wc) {
        const float lmax = log2f(pmax);
        float m = 0.f;
#pragma unroll
        for (int i = 0; i < DDW_NPT; ++i) {
            w[i] = __float_as_int(x[i]) >= tau ? (inv_temp == 1.f ? x[i] : exp2f((log2f(x[i]) - lmax) * inv_temp)) : 0.f;
            m += w[i];
        }
        wc = __float_as_int(pc) >= tau ? (inv_temp == 1.f ? pc : exp2f((log2f(pc) - lmax) * inv_temp)) : 0.f;
        return m + wc;
    };
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
        float w[DDW_NPT], wc;
        const float m = tempered_weights(tau, w, wc);
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
        // ---- the cuts, on q = w / Z over what top-k and top-p kept: the weights again, now over the final tau
        const float wmax = inv_temp == 1.f ? pmax : 1.f;
        const bool typical = cut.typical_p < 1.f;
        float w[DDW_NPT], wc;
        const float Z = block16_sum(tempered_weights(tau, w, wc), smf);
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
    return {own, bi, bp_own};
}

}  // namespace fira
