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
#include "engine.h"
#include "epilogue.h"
#include "decode_row.h"

namespace fira {

__global__ __launch_bounds__(DDW_NT) void sample_dist_kernel(int V, int S, const float* __restrict__ logits, int ldl,
                                                             const float* __restrict__ score,
                                                             const int32_t* __restrict__ mem_valid, int n_sample,
                                                             const float* __restrict__ xrow, const float* __restrict__ wp,
                                                             const float* __restrict__ bp, int T, int step,
                                                             const int32_t* __restrict__ key,
                                                             const uint64_t* __restrict__ seed_dev, float inv_temp,
                                                             int top_k, float top_p, float* __restrict__ dist,
                                                             int32_t* __restrict__ best_id, float* __restrict__ best_p) {
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
    // ---- Gumbel-max over the kept entries (p = 0 entries have score -inf and are skipped)
    const uint64_t seed = *seed_dev;
    const int b = r / n_sample, jsample = r - b * n_sample;
    const uint32_t stream = noise_stream((uint32_t)key[b], seed, jsample, T, step);
    float best = -INFINITY, bp_own = 0.f;
    int bi = 0x7fffffff;
#pragma unroll
    for (int i = 0; i < DDW_NPT; ++i) {                      // ascending index within the thread: the first maximum wins
        if (__float_as_int(x[i]) >= tau && x[i] > 0.f) {
            const int j = tid + DDW_NT * i;
            const float sc_i = logf(x[i]) * inv_temp + gumbel_noise(stream, (uint32_t)j);
            if (sc_i > best) { best = sc_i; bi = j; bp_own = x[i]; }
        }
    }
    if (__float_as_int(pc) >= tau && pc > 0.f) {
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
                int32_t* best_id, float* best_p) {
    ProfScope prof(s, PROF_HEAD, 0.0);
    if (R <= 0) return 0;
    FIRA_REQUIRE(V <= ROW_MAX_V && S <= ROW_MAX_SLOTS,
                 "sample_dist: vocabulary %d / %d memory slots exceed the register-resident row (%d / %d)", V, S, ROW_MAX_V,
                 ROW_MAX_SLOTS);
    hipLaunchKernelGGL(sample_dist_kernel, dim3(R), dim3(DDW_NT), 0, s, V, S, logits, ldl, score, mem_valid, n_sample, x, wp,
                       bp, T, step, key, seed_dev, 1.0f / temperature, top_k, top_p, dist, best_id, best_p);
    FIRA_CHECK_LAUNCH("sample_dist");
    return 0;
}

}  // namespace fira
