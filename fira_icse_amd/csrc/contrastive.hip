// Contrastive search: the selection of one step (include/fira_hip.h; Su et al., NeurIPS 2022).
//
// The deterministic search that looks one word ahead.  The k slots of a commit hold the same chosen prefix and one candidate
// next word each; the decoder step has consumed the candidates, so every slot has its hidden state h_j and the distribution
// after it.  fira_contrastive_select scores the candidates,
//     score_j = (1 - alpha) p_j - alpha max_{i < step} cos(h_j, H[b, i]),
// H the hidden states of the positions chosen so far, takes the best (ties to the lowest slot), appends its state to H and
// refills the slots with the k most probable continuations of the winner alone.
//
// One workgroup of 1024 threads per commit.
//   1. wave j (j < k) forms slot j's cosines: a lane holds 4 of the 256 floats of h_j and of a history row, the dot product
//      and the row's squared norm are two independent DPP butterflies (common.h: wave_sum), no LDS round trip.  The history
//      is k * step KB, read once per wave from L2.
//   2. every thread forms the k scores' arg-max from the k (sim, p) pairs in LDS: workgroup-uniform.
//   3. the ONE picked row of dist is streamed with fira_beam_select's loop into the thread's TopList (positive entries only),
//      then k block arg-max rounds over the list heads -- selection without a sort (beam.hip).  1 / k of the bytes
//      fira_beam_select reads.
//   4. k threads resolve the picks to words; write_hypotheses (decode_row.h) forms the new rows.
// Plain vector stores, no atomics on global memory.
#include <limits.h>
#include <math.h>
#include "engine.h"
#include "decode_row.h"

namespace fira {

// a commit that is over (or has no live slot): its rows are handed on unchanged, fira_beam_select's pass_through_done per commit
__device__ __forceinline__ void contrastive_copy_through(int b, int r0, int k, int T, const int32_t* __restrict__ gen_in,
                                                         const int32_t* __restrict__ len_in, const float* __restrict__ p_in,
                                                         const float* __restrict__ prob_in, int32_t* __restrict__ gen_out,
                                                         int32_t* __restrict__ len_out, float* __restrict__ p_out,
                                                         float* __restrict__ prob_out, int32_t* __restrict__ parent,
                                                         int32_t* __restrict__ pick_out, float* __restrict__ sim_out,
                                                         float* __restrict__ score_out) {
    const int t = threadIdx.x;
    pass_through_done(r0, k, T, gen_in, len_in, p_in, gen_out, len_out, p_out, parent);
    if (t < k) {
        if (sim_out) sim_out[r0 + t] = 0.f;
        if (score_out) score_out[r0 + t] = 0.f;
    }
    if (t == 0) {
        prob_out[b] = prob_in[b];
        if (pick_out) pick_out[b] = -1;
    }
}

template <int NB>
__global__ __launch_bounds__(DDW_NT) void contrastive_select_kernel(
    int k, int T, int W, int V, int L, int S, int step, float alpha, const float* __restrict__ dist,
    const float* __restrict__ hidden, const int32_t* __restrict__ fin, const int32_t* __restrict__ sou,
    const int32_t* __restrict__ sub, const int32_t* __restrict__ gen_in, const int32_t* __restrict__ len_in,
    const float* __restrict__ p_in, const float* __restrict__ prob_in, float* __restrict__ hist, int32_t* __restrict__ ended,
    int32_t* __restrict__ gen_out, int32_t* __restrict__ len_out, float* __restrict__ p_out, float* __restrict__ prob_out,
    int32_t* __restrict__ parent, int32_t* __restrict__ pick_out, float* __restrict__ sim_out, float* __restrict__ score_out) {
    __shared__ float smv[DDW_NT / 64];
    __shared__ int smi[DDW_NT / 64];
    __shared__ float sim_s[BEAM_MAX], sel_v[BEAM_MAX];
    __shared__ int sel_i[BEAM_MAX], src_of[BEAM_MAX], tok_of[BEAM_MAX], carry_of[BEAM_MAX];
    const int b = blockIdx.x, t = threadIdx.x, r0 = b * k, wave = t >> 6, lane = t & 63;
    if (ended[b]) {                                                  // (workgroup-uniform; nobody has written ended[b] yet)
        contrastive_copy_through(b, r0, k, T, gen_in, len_in, p_in, prob_in, gen_out, len_out, p_out, prob_out, parent, pick_out,
                                 sim_out, score_out);
        return;
    }
    // 1. the degeneration penalty of slot `wave`: lane l holds floats 4 l .. 4 l + 3 of the row
    if (wave < k) {
        const float4 h = reinterpret_cast<const float4*>(hidden + (size_t)(r0 + wave) * FIRA_D)[lane];
        const float nh = wave_sum(h.x * h.x + h.y * h.y + h.z * h.z + h.w * h.w);
        const float rh = sqrtf(nh);
        float sim = step > 0 ? -INFINITY : 0.f;
        const float4* H = reinterpret_cast<const float4*>(hist + (size_t)b * T * FIRA_D);
        for (int i = 0; i < step; ++i) {
            const float4 g = H[i * (FIRA_D / 4) + lane];
            const float dot = wave_sum(h.x * g.x + h.y * g.y + h.z * g.z + h.w * g.w);
            const float ng = wave_sum(g.x * g.x + g.y * g.y + g.z * g.z + g.w * g.w);
            const float c = (nh == 0.f || ng == 0.f) ? 0.f : dot / (rh * sqrtf(ng));
            sim = fmaxf(sim, c);
        }
        if (lane == 0) sim_s[wave] = sim;
    }
    __syncthreads();
    // 2. the scores and their arg-max (every thread, the same values); each product and the difference round on their own
    const float one_minus = 1.0f - alpha;
    int js = -1;
    float best = -INFINITY;
    for (int j = 0; j < k; ++j) {
        const float p = p_in[r0 + j];
        const bool live = p > 0.f;
        const float sc = __fsub_rn(__fmul_rn(one_minus, p), __fmul_rn(alpha, sim_s[j]));
        if (t == j) {
            if (sim_out) sim_out[r0 + j] = live ? sim_s[j] : 0.f;
            if (score_out) score_out[r0 + j] = live ? sc : 0.f;
        }
        if (live && (js < 0 || sc > best)) { best = sc; js = j; }
    }
    if (js < 0) {                                                    // no live slot: the commit ends where it is
        contrastive_copy_through(b, r0, k, T, gen_in, len_in, p_in, prob_in, gen_out, len_out, p_out, prob_out, parent, pick_out,
                                 sim_out, score_out);
        if (t == 0) ended[b] = 1;
        return;
    }
    const int rs = r0 + js;
    const float pj = p_in[rs];
    // 3. the winner's state joins the history
    if (t < FIRA_D / 4)
        reinterpret_cast<float4*>(hist + ((size_t)b * T + step) * FIRA_D)[t] = reinterpret_cast<const float4*>(hidden + (size_t)rs * FIRA_D)[t];
    if (t == 0) {
        prob_out[b] = __fmul_rn(prob_in[b], pj);
        if (pick_out) pick_out[b] = js;
    }
    const bool ends = fin[rs] != 0;                                  // (uniform) the winner's word is <eos>
    if (ends) {
        if (t < k) { src_of[t] = js; tok_of[t] = 0; carry_of[t] = 1; len_out[r0 + t] = len_in[rs]; p_out[r0 + t] = pj; parent[r0 + t] = rs; }
        if (t == 0) ended[b] = 1;
    } else {
        // the k largest positive entries of the winner's row: fira_beam_select's loop over one row
        TopList<NB, Cand> top;
        top.clear();
        const float* row = dist + (size_t)rs * W;
        for (int w0 = t; w0 < W; w0 += 4 * DDW_NT) {
            float x[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) x[u] = row[min(w0 + u * DDW_NT, W - 1)];
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (w0 + u * DDW_NT < W && x[u] > 0.f) top.offer({x[u], w0 + u * DDW_NT});
        }
        for (int round = 0; round < k; ++round) {
            Cand c = top.e[0];
            block16_argmax(c.v, c.i, smv, smi);
            if (t == 0) { sel_v[round] = c.v; sel_i[round] = c.i; }
            if (c.i != INT_MAX && top.e[0].i == c.i) top.pop();
        }
        __syncthreads();
        if (t < k) {
            const int idx = sel_i[t];
            const bool none = idx == INT_MAX;                        // fewer than k positive entries: a void slot
            src_of[t] = js; carry_of[t] = none;
            tok_of[t] = none ? 0 : entry_word(idx, sou, sub, (size_t)b, V, L, S);
            const int sl = len_in[rs];
            len_out[r0 + t] = none ? sl : sl + 1;
            p_out[r0 + t] = none ? -1.0f : sel_v[t];
            parent[r0 + t] = rs;
        }
    }
    __syncthreads();
    write_hypotheses(r0, k, T, src_of, tok_of, carry_of, gen_in, len_in, gen_out);
}

}  // namespace fira

extern "C" int fira_contrastive_select(void* stream, const fira_dims* d, int B, int k, int step, float alpha, const float* dist,
                                       const float* hidden, const int32_t* finished, const int32_t* sou, const int32_t* sub_token,
                                       const int32_t* gen_in, const int32_t* len_in, const float* p_in, const float* prob_in,
                                       float* hist, int32_t* ended, int32_t* gen_out, int32_t* len_out, float* p_out,
                                       float* prob_out, int32_t* parent, int32_t* pick_out, float* sim_out, float* score_out) {
    using namespace fira;
    FIRA_REQUIRE(d, "fira_contrastive_select: null dims");
    FIRA_REQUIRE(B > 0, "fira_contrastive_select: B = %d must be positive", B);
    FIRA_REQUIRE(k >= 2 && k <= BEAM_MAX, "fira_contrastive_select: k = %d outside 2..%d", k, BEAM_MAX);
    FIRA_REQUIRE(d->tar_len >= 2 && d->tar_len <= ROW_MAX_T, "fira_contrastive_select: tar_len = %d outside 2..%d", d->tar_len,
                 ROW_MAX_T);
    FIRA_REQUIRE(step >= 0 && step <= d->tar_len - 2, "fira_contrastive_select: step = %d outside 0..tar_len - 2 = %d", step,
                 d->tar_len - 2);
    FIRA_REQUIRE(alpha >= 0.f && alpha <= 1.f, "fira_contrastive_select: alpha = %g outside [0, 1]", (double)alpha);   // (also nan)
    FIRA_REQUIRE(d->vocab > BEAM_MAX && d->vocab <= ROW_MAX_V && d->sou_len >= 0 && d->sub_len >= 0 &&
                     d->sou_len + d->sub_len <= ROW_MAX_SLOTS,
                 "fira_contrastive_select: vocabulary %d / %d memory slots outside %d..%d / 0..%d", d->vocab,
                 d->sou_len + d->sub_len, BEAM_MAX + 1, ROW_MAX_V, ROW_MAX_SLOTS);
    FIRA_REQUIRE(dist && hidden && finished && sou && sub_token && gen_in && len_in && p_in && prob_in && hist && ended && gen_out &&
                     len_out && p_out && prob_out && parent,
                 "fira_contrastive_select: null pointer (pick_out, sim_out and score_out alone may be NULL)");
    FIRA_REQUIRE((uintptr_t)hidden % 16 == 0 && (uintptr_t)hist % 16 == 0,
                 "fira_contrastive_select: hidden and hist must be 16-byte aligned");
    const int S = d->sub_len, L = d->sou_len, W = d->vocab + L + S;
#define FIRA_CS_LAUNCH(NB)                                                                                                     \
    hipLaunchKernelGGL((contrastive_select_kernel<NB>), dim3(B), dim3(DDW_NT), 0, (hipStream_t)stream, k, d->tar_len, W, d->vocab, \
                       L, S, step, alpha, dist, hidden, finished, sou, sub_token, gen_in, len_in, p_in, prob_in, hist, ended,   \
                       gen_out, len_out, p_out, prob_out, parent, pick_out, sim_out, score_out)
    if (k <= 4) FIRA_CS_LAUNCH(4);
    else FIRA_CS_LAUNCH(BEAM_MAX);
#undef FIRA_CS_LAUNCH
    FIRA_CHECK_LAUNCH("fira_contrastive_select");
    return 0;
}
