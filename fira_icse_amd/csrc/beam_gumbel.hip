// Stochastic beam search: the selection step (include/fira_hip.h).
//
// fira_beam_select_gumbel is fira_beam_select (beam.hip) with a random ranking key: the Gumbel-perturbed log-probability of a
// hypothesis, a child's key conditioned on its parent's (Kool, van Hoof and Welling, 2019).  The n hypotheses a search returns
// are then a sample WITHOUT replacement from the model's distribution over messages, best key first.  The state has the beam's
// shape -- gen, length, parent, double-buffered -- with three fp32 values per slot in place of prob:
//     phi   log-probability of the hypothesis under the sampling model   G   its perturbed key (-inf: the slot is VOID)
//     logp  the untempered sum of logf(p_entry) of the entries taken (what fira_sample_advance accumulates)
// Per commit b, for every RUNNING slot j (G_j > -inf, not finished), with its row p = dist[b * n + j, :] as it stands:
//     valid entry   0 < p_i <= FLT_MAX (a zero, a NaN and an inf are void)
//     t_i = logf(p_i),  u_i = t_i * inv_T,  s_i = fmaf(t_i, inv_T, gumbel_i)      -- the sampler's score, bit for bit
//     lnZ = um + logf(sum_i expf(u_i - um)),  um = logf(max_i p_i) * inv_T         -- the sampling model q_i = p_i^(1/T) / Z
//     a   = argmax_i s_i (lowest index on ties),  c = phi_j - lnZ,  g_i = c + s_i,  Zmax = c + s_a
//     key_a = G_j by definition;  for i != a, d = g_i - Zmax:
//         d < 0:   v = (G_j - g_i) + log1pf(-expf(d)),   key_i = (G_j - fmaxf(0, v)) - log1pf(expf(-fabsf(v)))
//         else     key_i = G_j                                  (a tie with the arg-max: log1p(-1) = -inf stays out of it)
// A finished hypothesis with G > -inf is CARRIED: it competes with its own key.  Total order of a commit's candidates: void
// last (they are never offered), key descending, a row's arg-max entry before every other candidate, then fira_beam_select's
// flattened index ascending (running slots in slot order, then the carried ones in slot order).  The last two are one
// integer: code = (arg-max ? 0 : n * W + n) + index, so the candidates are the toolkit's Cand under better().
//
// One workgroup of 1024 threads per commit.  A running row is requested ONCE, 26 loads in flight per thread (W <= 26 * 1024),
// and stays in registers: first as p, then as s.  Three block reductions per row (the maximum, the sum, the arg-max), then every
// valid entry's key goes to the thread's TopList of the commit; thread 0 offers the carried candidates; n rounds of the block
// arg-max pop the winners; n threads resolve them (phi, logp and the id from the winner's own entry, re-read).  No key is formed
// from an infinite operand: G_j, phi_j are finite for a running slot, s_i is finite for a valid entry.  Plain vector stores,
// no atomics on global memory.
#include <float.h>
#include <limits.h>
#include <math.h>
#include "engine.h"
#include "decode_row.h"

namespace fira {

constexpr int BG_NPT = DDW_NPT + 1;             // entries of a row per thread: 25 generator registers + one copy slot
constexpr int BG_START = 2;                     // <start> (config.START), the one id of a void hypothesis

template <int NB>
__global__ __launch_bounds__(DDW_NT) void beam_select_gumbel_kernel(
    int n, int T, int W, int V, int L, int S, int step, float inv_temp, const float* __restrict__ dist,
    const int32_t* __restrict__ fin, const int32_t* __restrict__ done, const int32_t* __restrict__ sou,
    const int32_t* __restrict__ sub, const int32_t* __restrict__ key, const uint64_t* __restrict__ seed_dev,
    const int32_t* __restrict__ gen_in, const int32_t* __restrict__ len_in, const float* __restrict__ phi_in,
    const float* __restrict__ G_in, const float* __restrict__ logp_in, int32_t* __restrict__ gen_out,
    int32_t* __restrict__ len_out, float* __restrict__ phi_out, float* __restrict__ G_out, float* __restrict__ logp_out,
    int32_t* __restrict__ parent) {
    __shared__ float smf[DDW_NT / 64];
    __shared__ int smi[DDW_NT / 64];
    __shared__ float sel_v[BEAM_MAX], lnz_of[BEAM_MAX];
    __shared__ int sel_i[BEAM_MAX], order[BEAM_MAX], src_of[BEAM_MAX], tok_of[BEAM_MAX], kind_of[BEAM_MAX];
    const int b = blockIdx.x, t = threadIdx.x, r0 = b * n;
    if (*done) {                                                     // search over: the state is handed on unchanged
        for (int x = t; x < n * T; x += DDW_NT) gen_out[(size_t)r0 * T + x] = gen_in[(size_t)r0 * T + x];
        if (t < n) {
            len_out[r0 + t] = len_in[r0 + t]; phi_out[r0 + t] = phi_in[r0 + t]; G_out[r0 + t] = G_in[r0 + t];
            logp_out[r0 + t] = logp_in[r0 + t]; parent[r0 + t] = r0 + t;
        }
        return;
    }
    const uint64_t seed = *seed_dev;
    const uint32_t kb = (uint32_t)key[b];
    const int other = n * W + n;                                     // code offset of a candidate that is no row's arg-max
    TopList<NB, Cand> top;
    top.clear();
    for (int j = 0; j < n; ++j) {
        const float Gj = G_in[r0 + j], phij = phi_in[r0 + j];
        if (!(Gj > -INFINITY) || fin[r0 + j]) continue;              // (workgroup-uniform) void, or carried below
        const float* row = dist + (size_t)(r0 + j) * W;
        float x[BG_NPT];
#pragma unroll
        for (int k = 0; k < BG_NPT; ++k) x[k] = row[min(t + DDW_NT * k, W - 1)];
        float pmax = 0.f;
#pragma unroll
        for (int k = 0; k < BG_NPT; ++k) {
            x[k] = (t + DDW_NT * k < W && x[k] > 0.f && x[k] <= FLT_MAX) ? x[k] : 0.f;      // void entries: 0
            pmax = fmaxf(pmax, x[k]);
        }
        int dummy = 0;
        block16_argmax(pmax, dummy, smf, smi);
        if (!(pmax > 0.f)) continue;                                 // (uniform) nothing left of the row: no candidate
        const float um = logf(pmax) * inv_temp;
        const uint32_t stream = noise_stream(kb, seed, j, T, step);
        float sum = 0.f;
        ArgMax am;
#pragma unroll
        for (int k = 0; k < BG_NPT; ++k) {                           // ascending index within the thread: the first maximum wins
            float s = -INFINITY;
            if (x[k] > 0.f) {
                const int i = t + DDW_NT * k;
                const float ti = logf(x[k]);
                sum += expf(ti * inv_temp - um);
                s = fmaf(ti, inv_temp, gumbel_noise(stream, (uint32_t)i));
                if (s > am.v) { am.v = s; am.i = i; }
            }
            x[k] = s;
        }
        sum = block16_sum(sum, smf);
        am.reduce(smf, smi);
        const float lnZ = um + logf(sum);
        const float c = phij - lnZ, Zmax = c + am.v;
        if (t == 0) lnz_of[j] = lnZ;
#pragma unroll
        for (int k = 0; k < BG_NPT; ++k) {
            const float s = x[k];
            if (s > -INFINITY) {
                const int i = t + DDW_NT * k;
                float kv = Gj;
                const float gi = c + s, d = gi - Zmax;
                if (i != am.i && d < 0.f) {
                    const float v = (Gj - gi) + log1pf(-expf(d));
                    kv = (Gj - fmaxf(0.f, v)) - log1pf(expf(-fabsf(v)));
                }
                top.offer({kv, (i == am.i ? 0 : other) + j * W + i});
            }
        }
    }
    if (t == 0) {                                                    // the finished hypotheses of the commit, slot order
        int c = 0;
        for (int j = 0; j < n; ++j)
            if (fin[r0 + j] && G_in[r0 + j] > -INFINITY) { order[c] = j; top.offer({G_in[r0 + j], other + n * W + c}); ++c; }
        for (int q = c; q < n; ++q) order[q] = 0;
    }
    // n rounds of a block-wide arg-max over the list heads; the owner of the winner pops it
    for (int round = 0; round < n; ++round) {
        Cand cd = top.e[0];
        block16_argmax(cd.v, cd.i, smf, smi);
        if (t == 0) { sel_v[round] = cd.v; sel_i[round] = cd.i; }
        if (cd.i != INT_MAX && top.e[0].i == cd.i) top.pop();
    }
    __syncthreads();
    if (t < n) {
        const int code = sel_i[t];
        int kind = 2, src = t, nt = 0;                               // kind 0: extended, 1: carried, 2: void
        if (code != INT_MAX) {
            const int idx = code >= other ? code - other : code;
            const int which = idx / W, w = idx - which * W;
            kind = which >= n;
            src = kind ? order[min(w, n - 1)] : which;
            if (!kind) nt = entry_word(w, sou, sub, (size_t)b, V, L, S);
            if (kind) {
                len_out[r0 + t] = len_in[r0 + src]; phi_out[r0 + t] = phi_in[r0 + src]; G_out[r0 + t] = G_in[r0 + src];
                logp_out[r0 + t] = logp_in[r0 + src];
            } else {
                const float lp = logf(dist[(size_t)(r0 + src) * W + w]);
                len_out[r0 + t] = len_in[r0 + src] + 1;
                phi_out[r0 + t] = phi_in[r0 + src] + (lp * inv_temp - lnz_of[src]);
                G_out[r0 + t] = sel_v[t];
                logp_out[r0 + t] = logp_in[r0 + src] + lp;
            }
        } else {                                                     // fewer than n candidates: a void slot
            len_out[r0 + t] = 1; phi_out[r0 + t] = -INFINITY; G_out[r0 + t] = -INFINITY; logp_out[r0 + t] = -INFINITY;
        }
        parent[r0 + t] = r0 + src;
        src_of[t] = src; tok_of[t] = nt; kind_of[t] = kind;
    }
    __syncthreads();
    for (int x = t; x < n * T; x += DDW_NT) {                        // write_hypotheses, plus the void hypothesis: <start> alone
        const int cidx = x / T, p = x - cidx * T;
        const int src = src_of[cidx], kind = kind_of[cidx];
        int g = gen_in[(size_t)(r0 + src) * T + p];
        if (kind == 0 && p == min(len_in[r0 + src], T - 1)) g = tok_of[cidx];
        if (kind == 2) g = p == 0 ? BG_START : 0;
        gen_out[(size_t)(r0 + cidx) * T + p] = g;
    }
}

}  // namespace fira

extern "C" int fira_beam_select_gumbel(void* stream, const fira_dims* d, int B, int n_beam, int step, float temperature,
                                       const float* dist, const int32_t* finished, const int32_t* done, const int32_t* sou,
                                       const int32_t* sub_token, const int32_t* key, const uint64_t* seed_dev,
                                       const int32_t* gen_in, const int32_t* len_in, const float* phi_in, const float* G_in,
                                       const float* logp_in, int32_t* gen_out, int32_t* len_out, float* phi_out, float* G_out,
                                       float* logp_out, int32_t* parent) {
    using namespace fira;
    FIRA_REQUIRE(d, "fira_beam_select_gumbel: null dims");
    FIRA_REQUIRE(B > 0, "fira_beam_select_gumbel: B = %d must be positive", B);
    FIRA_REQUIRE(n_beam >= 1 && n_beam <= BEAM_MAX, "fira_beam_select_gumbel: n_beam = %d outside 1..%d", n_beam, BEAM_MAX);
    FIRA_REQUIRE(temperature > 0.0f && temperature <= FLT_MAX, "fira_beam_select_gumbel: temperature = %g must be finite and > 0",
                 (double)temperature);
    FIRA_REQUIRE(d->tar_len >= 2 && d->tar_len <= ROW_MAX_T, "fira_beam_select_gumbel: tar_len = %d outside 2..%d", d->tar_len,
                 ROW_MAX_T);
    FIRA_REQUIRE(step >= 0 && step + 1 < d->tar_len, "fira_beam_select_gumbel: step = %d outside 0..tar_len - 2 = %d", step,
                 d->tar_len - 2);
    FIRA_REQUIRE(d->vocab > BEAM_MAX && d->vocab <= ROW_MAX_V && d->sou_len >= 0 && d->sub_len >= 0 &&
                     d->sou_len + d->sub_len <= ROW_MAX_SLOTS,
                 "fira_beam_select_gumbel: vocabulary %d / %d memory slots outside %d..%d / 0..%d", d->vocab,
                 d->sou_len + d->sub_len, BEAM_MAX + 1, ROW_MAX_V, ROW_MAX_SLOTS);
    FIRA_REQUIRE(dist && finished && done && sou && sub_token && key && seed_dev && gen_in && len_in && phi_in && G_in && logp_in &&
                     gen_out && len_out && phi_out && G_out && logp_out && parent,
                 "fira_beam_select_gumbel: null pointer");
    const int S = d->sub_len, L = d->sou_len, W = d->vocab + L + S;  // <= 25 600 + 1 024 = 26 * 1 024: BG_NPT entries per thread
#define FIRA_BG_LAUNCH(NB)                                                                                                      \
    hipLaunchKernelGGL((beam_select_gumbel_kernel<NB>), dim3(B), dim3(DDW_NT), 0, (hipStream_t)stream, n_beam, d->tar_len, W,   \
                       d->vocab, L, S, step, 1.0f / temperature, dist, finished, done, sou, sub_token, key, seed_dev, gen_in,   \
                       len_in, phi_in, G_in, logp_in, gen_out, len_out, phi_out, G_out, logp_out, parent)
    if (n_beam <= 4) FIRA_BG_LAUNCH(4);
    else FIRA_BG_LAUNCH(BEAM_MAX);
#undef FIRA_BG_LAUNCH
    FIRA_CHECK_LAUNCH("fira_beam_select_gumbel");
    return 0;
}
