// Sampling from a distribution row that already exists in memory: the sampler's filters, cuts and Gumbel-max draw
// (sampler_row.h) applied to dist[r, 0 .. V + S) as the step, the mixing kernels and the edit chain (fira_merge_dist,
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
// Everything after the load is the sampler body (sampler_row.h), the code sample_dist_kernel runs too: top-k and top-p by
// bisection over float bits, the SampleCuts block, the drop mask, the Gumbel-max draw.  On a row the fused sampler stored, this
// kernel therefore takes the same thresholds and draws the same entry with the same best_p, bit for bit
// (tests/test_sample_search_gpu.py).
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
#include <math.h>
#include "engine.h"
#include "epilogue.h"
#include "decode_row.h"
#include "sampler_row.h"

namespace fira {

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
    const float pmax = block16_max(own_max, smf);            // the largest entry of the row as it stands
    const SampleDraw d = sampler_draw<CUT>(x, pc, pmax, V, r, n_sample, T, step, key, seed_dev, inv_temp, top_k, top_p, cut, smf, smi);
    if (d.win == 0x7fffffff) {                               // no positive entry: ArgMax's report for an all-zero row
        if (tid == 0) { best_id[r] = 0; best_p[r] = 0.f; }
    } else if (d.own == d.win) {                             // the owner of the winning entry reports it
        best_id[r] = d.win;
        best_p[r] = d.bp_own;
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
    const int V = d->vocab, S = d->sou_len + d->sub_len;
    SampleCuts cut;
    cut.min_p = min_p; cut.epsilon = epsilon; cut.eta = eta; cut.typical_p = typical_p;
    if (int e = require_sampler_args(who, V + S, temperature, top_k, top_p, &cut)) return e;
    if (R == 0) return 0;
    FIRA_REQUIRE(dist && key && seed_dev, "%s: null pointer (dist, key or seed_dev)", who);
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
