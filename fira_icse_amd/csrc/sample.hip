// On-device sampling of the decode step's output distribution: temperature, top-k and top-p, drawn by Gumbel-max, and the
// truncation cuts of fira_decode_step_sample_cut.
//
// One workgroup of 1024 threads per (commit, sample) row.  The row is WideRow (decode_row.h), the distribution p over V + S
// entries that fira_decode_step writes; the optional `dist` row is stored from it.  This kernel scales the row to p, knows its
// maximum without a reduction (max(sg, sc): the largest entry of either part is exp(0) = 1 times its scale) and hands both to
// the sampler body (sampler_row.h: the filters, the cuts and the draw, shared with sample_row.hip).  A row always has a
// winner here (its maximum is positive and always kept); the report writes nothing otherwise.
//
// Two instances: <false> is the plain sampler and is what a call with every cut off launches, <true> has the SampleCuts block.
// require_sampler_args: the host's range and combination checks of temperature, top-k, top-p and the cuts, one copy for
// fira_decode_step_sample[_cut] and fira_sample_dist.
#include "engine.h"
#include "epilogue.h"
#include "decode_row.h"
#include "sampler_row.h"

namespace fira {

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
    const SampleDraw d = sampler_draw<CUT>(x, pc, pmax, V, r, n_sample, T, step, key, seed_dev, inv_temp, top_k, top_p, cut, smf, smi);
    if (d.own == d.win && d.win != 0x7fffffff) {             // the owner of the winning entry reports it; no winner: no write
        best_id[r] = d.win;
        best_p[r] = d.bp_own;
    }
}

int require_sampler_args(const char* who, int W, float temperature, int top_k, float top_p, const SampleCuts* cut) {
    FIRA_REQUIRE(temperature > 0.f && temperature < INFINITY, "%s: temperature %g must be finite and > 0", who,
                 (double)temperature);
    FIRA_REQUIRE(top_k >= 0 && top_k <= W, "%s: top_k %d outside 0..%d", who, top_k, W);
    FIRA_REQUIRE(top_p > 0.f && top_p <= 1.f, "%s: top_p %g outside (0, 1]", who, (double)top_p);
    if (!cut) return 0;
    // (every comparison also refuses nan)
    FIRA_REQUIRE(cut->min_p >= 0.f && cut->min_p < 1.f, "%s: min_p %g outside [0, 1)", who, (double)cut->min_p);
    FIRA_REQUIRE(cut->epsilon >= 0.f && cut->epsilon < 1.f, "%s: epsilon %g outside [0, 1)", who, (double)cut->epsilon);
    FIRA_REQUIRE(cut->eta >= 0.f && cut->eta < 1.f, "%s: eta %g outside [0, 1)", who, (double)cut->eta);
    FIRA_REQUIRE(cut->typical_p > 0.f && cut->typical_p <= 1.f, "%s: typical_p %g outside (0, 1]", who, (double)cut->typical_p);
    if (cut->typical_p < 1.f) {                              // a band in p, not a lower threshold: temperature and top-k only
        FIRA_REQUIRE(top_p == 1.f, "%s: typical_p %g does not combine with top_p %g", who, (double)cut->typical_p, (double)top_p);
        FIRA_REQUIRE(cut->min_p == 0.f, "%s: typical_p %g does not combine with min_p %g", who, (double)cut->typical_p,
                     (double)cut->min_p);
        FIRA_REQUIRE(cut->epsilon == 0.f, "%s: typical_p %g does not combine with epsilon %g", who, (double)cut->typical_p,
                     (double)cut->epsilon);
        FIRA_REQUIRE(cut->eta == 0.f, "%s: typical_p %g does not combine with eta %g", who, (double)cut->typical_p,
                     (double)cut->eta);
    }
    return 0;
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
