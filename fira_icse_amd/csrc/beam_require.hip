// Lexically constrained beam search: the selection step with dynamic beam allocation (include/fira_hip.h;
// Post and Vilar, NAACL 2018).
//
// fira_beam_select_required is fira_beam_select (beam.hip) with the beam divided into BANKS by the number of required words a
// hypothesis holds.  The state is the same -- gen, length, raw probability, double-buffered -- because that number is a function
// of the hypothesis's gen row.  Per commit b: C = n_required[b] clamped to 0..4, R_k = required[b, k] for k < C, and
//     met(h)  = { k : R_k occurs among gen[1 .. length - 1] },   bank(h) = |met(h)|.
// Candidates of a step, in fira_beam_select's flattened index order (running slots in slot order, then the carried list):
//     running   entry i of running slot j:  p = fp32(dist[j, i] * prob[j])  (the product fira_beam_select forms),
//               bank = |met(h_j) u { k : R_k == w(i) }|, w(i) the word of the entry: i below V, the sou / sub_token id of its
//               copy slot above
//     carried   a finished hypothesis:  p = prob[j],  bank = bank(h_j)
//     void      fira_beam_select's two -1 (the row of a finished hypothesis, the padding of the carried list) and every entry
//               with w(i) == <eos> of a running row with bank(h_j) < C: a message may not end before it holds all its words
// Phase 1, round robin: among the candidates with p > 0, ranked within a bank by (p descending, index ascending), repeat "for
// c = C down to 0: take the best unpicked candidate of bank c, if it has one" until n_beam picks are made or none is left.
// Phase 2, fill: the slots still free take the remaining candidates by (value descending, index ascending) -- they all have
// value 0.  The picks are written sorted by (p > 0 first, bank descending, p descending, pick order ascending).  With C = 0
// there is one bank, the two phases are (p descending, index ascending) and the sort is stable: the four outputs are then
// fira_beam_select's bit for bit.
// A void candidate is never reached, so none is ever offered: a commit with r >= 1 running rows has at least
// r * (W - copies of <eos> - 1) >= r * (V - 1) >= 8 >= n_beam candidates that are not void (vocab > 8; the row's own <eos>
// entry and the copy slots that carry <eos> are the only ones the rule can void), and a commit with r = 0 carries all its
// n_beam hypotheses.
//
// One workgroup of 1024 threads per commit.
//   1. wave j forms met(h_j): lane p compares gen[j, p] with the C words, one ballot per word.
//   2. every running row is streamed once with fira_beam_select's loop (thread t owns the entries i = t mod 1024).  A row feeds
//      its own bank, bank(h_j) -- workgroup-uniform, so the thread's TopList (decode_row.h) of that bank is chosen outside the
//      loop -- except for its PROMOTING entries, those of an unmet required word.  They are few and their places are known:
//      at most C generator entries, re-read by threads 0 .. C - 1 after the loop (4 bytes each), and the copy slots that carry
//      the word, of which a thread owns at most one (sou_len + sub_len <= 1024): it keeps that entry aside while streaming.
//   3. thread 0 offers the carried candidates.  Every thread now holds, per bank, its NB >= n_beam best candidates; zeros rank
//      below the positive ones, so the lists serve both phases.
//   4. phase 1: one block arg-max (decode_row.h) over the heads of bank c per pick; a bank found without a positive head is
//      dry for good, so at most n_beam + C + 1 reductions.  Phase 2: one arg-max over every thread's best head per pick.
//      The owner of a winner pops it.  Five lists cannot lose a candidate that a phase needs: no bank gives more than n_beam
//      picks, and phase 2 runs only when fewer than n_beam candidates are positive, so each list still holds its first zeros.
//   5. n_beam threads rank the picks (a count of the picks that sort before one's own) and resolve them as fira_beam_select does.
// Plain vector stores, no atomics on global memory.
#include <limits.h>
#include "engine.h"
#include "decode_row.h"

namespace fira {

constexpr int RQ_MAX = 4;                       // required words per commit
constexpr int RQ_BANKS = RQ_MAX + 1;
constexpr int RQ_EOS = 1;                       // <eos> (config.EOS)

// The thread's lists, one per bank.  `bank` is indexed through an unrolled chain so that the lists stay in registers.
template <int NB>
struct BankLists {
    TopList<NB, Cand> top[RQ_BANKS];
    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int c = 0; c < RQ_BANKS; ++c) top[c].clear();
    }
    __device__ __forceinline__ void offer(int bank, const Cand& cd) {
#pragma unroll
        for (int c = 0; c < RQ_BANKS; ++c)
            if (c == bank) top[c].offer(cd);
    }
    __device__ __forceinline__ Cand head(int bank) const {
        Cand h = Cand::none();
#pragma unroll
        for (int c = 0; c < RQ_BANKS; ++c)
            if (c == bank) h = top[c].e[0];
        return h;
    }
    // the list whose head is candidate `idx` (indices are unique over the lists) gives it up; its bank, or -1
    __device__ __forceinline__ int pop(int idx) {
        int bank = -1;
#pragma unroll
        for (int c = 0; c < RQ_BANKS; ++c)
            if (bank < 0 && top[c].e[0].i == idx) { top[c].pop(); bank = c; }
        return bank;
    }
};

// the bits k < C with R_k == word
__device__ __forceinline__ int rq_match(int word, int C, const int (&R)[RQ_MAX]) {
    int m = 0;
#pragma unroll
    for (int k = 0; k < RQ_MAX; ++k) m |= (k < C && word == R[k]) ? 1 << k : 0;
    return m;
}

template <int NB>
__global__ __launch_bounds__(DDW_NT) void beam_select_required_kernel(
    int beam, int T, int W, int V, int L, int S, const float* __restrict__ dist, const int32_t* __restrict__ fin,
    const int32_t* __restrict__ active, const int32_t* __restrict__ done, const int32_t* __restrict__ sou,
    const int32_t* __restrict__ sub, const int32_t* __restrict__ gen_in, const int32_t* __restrict__ len_in,
    const float* __restrict__ prob_in, const int32_t* __restrict__ required, const int32_t* __restrict__ n_required,
    int32_t* __restrict__ gen_out, int32_t* __restrict__ len_out, float* __restrict__ prob_out, int32_t* __restrict__ parent,
    int32_t* __restrict__ met_out) {
    __shared__ float smv[DDW_NT / 64];
    __shared__ int smi[DDW_NT / 64];
    __shared__ float sel_v[BEAM_MAX];
    __shared__ int sel_i[BEAM_MAX], sel_b[BEAM_MAX], act_slot[BEAM_MAX], order[BEAM_MAX], src_of[BEAM_MAX], tok_of[BEAM_MAX],
        carry_of[BEAM_MAX], met_s[BEAM_MAX];
    const int b = blockIdx.x, t = threadIdx.x, r0 = b * beam;
    const int C = min(max(n_required[b], 0), RQ_MAX);
    int R[RQ_MAX];
#pragma unroll
    for (int k = 0; k < RQ_MAX; ++k) R[k] = required[(size_t)b * RQ_MAX + k];

    // 1. met(h_j) of the commit's hypotheses: wave j, one position per lane (T <= 64)
    if ((t >> 6) < beam) {
        const int j = t >> 6, p = t & 63;
        const int len = min(max(len_in[r0 + j], 1), T);
        const int g = gen_in[(size_t)(r0 + j) * T + min(p, T - 1)];
        int m = 0;
#pragma unroll
        for (int k = 0; k < RQ_MAX; ++k)
            if (__ballot(p >= 1 && p < len && k < C && g == R[k]) != 0ull) m |= 1 << k;
        if (p == 0) met_s[j] = m;
    }
    __syncthreads();
    if (*done) {
        pass_through_done(r0, beam, T, gen_in, len_in, prob_in, gen_out, len_out, prob_out, parent);
        if (t < beam && met_out) met_out[r0 + t] = __popc(met_s[t]);
        return;
    }
    const int n_act = active[BEAM_MAX];
    // the word of the one copy slot this thread streams: entry V + s with V + s = t (mod 1024)
    const int my_word = slot_word(sou, sub, (size_t)b, L, S, (t - V % DDW_NT + DDW_NT) % DDW_NT);

    BankLists<NB> lists;
    lists.clear();
    // 2. the running rows
    int k = 0;
    for (int j = 0; j < beam; ++j) {
        if (!active[j]) continue;
        if (t == 0) act_slot[k] = j;
        if (!fin[r0 + j]) {                                          // (workgroup-uniform) a finished row is void
            const int mj = met_s[j], bj = __popc(mj);
            const bool no_eos = bj < C;
            const float pj = prob_in[r0 + j];
            const float* row = dist + (size_t)(r0 + j) * W;
            Cand aside = Cand::none();                               // this thread's promoting copy entry of the row
            int aside_bank = 0;
#pragma unroll
            for (int c = 0; c < RQ_BANKS; ++c) {
                if (c != bj) continue;                               // (uniform) the row's own bank
                for (int w0 = t; w0 < W; w0 += 4 * DDW_NT) {         // four loads in flight per trip
                    float x[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) x[u] = row[min(w0 + u * DDW_NT, W - 1)];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const int i = w0 + u * DDW_NT;
                        if (i < W) {
                            const int word = i < V ? i : my_word;
                            const int all = mj | rq_match(word, C, R);
                            const Cand cd = {x[u] * pj, k * W + i};
                            if (no_eos && word == RQ_EOS) {
                                // void
                            } else if (all == mj) {
                                lists.top[c].offer(cd);
                            } else if (i >= V) {
                                aside = cd; aside_bank = __popc(all);
                            }                                        // (a promoting generator entry: below)
                        }
                    }
                }
            }
            if (aside.i != INT_MAX) lists.offer(aside_bank, aside);
            // the promoting generator entries: thread q takes R_q if the word is unmet, inside the generator's range, not <eos>
            // while that is void, and not listed before (a duplicate would be offered twice)
            if (t < C) {
                int word = R[0];
#pragma unroll
                for (int q = 1; q < RQ_MAX; ++q) word = t == q ? R[q] : word;
                const int hit = rq_match(word, C, R);
                const bool first = (hit & ((1 << t) - 1)) == 0;
                if (first && (hit & ~mj) != 0 && word >= 0 && word < V && !(no_eos && word == RQ_EOS))
                    lists.offer(__popc(mj | hit), {row[word] * pj, k * W + word});
            }
        }
        ++k;
    }
    // 3. the carried candidates: finished hypotheses in slot order (the -1 padding is void)
    if (t == 0) {
        int c = 0;
        for (int j = 0; j < beam; ++j)
            if (fin[r0 + j]) { order[c] = j; lists.offer(__popc(met_s[j]), {prob_in[r0 + j], n_act * W + c}); ++c; }
        for (int q = c; q < beam; ++q) order[q] = 0;
    }
    // 4. phase 1: round robin over the banks, the highest first; positive candidates only
    int npick = 0;
    unsigned dry = 0;                                                // (uniform) banks without a positive candidate left
    while (npick < beam && dry != (2u << C) - 1u) {
        for (int c = C; c >= 0 && npick < beam; --c) {
            if (dry >> c & 1u) continue;
            const Cand h = lists.head(c);
            Cand w = h.v > 0.f ? h : Cand::none();
            block16_argmax(w.v, w.i, smv, smi);
            if (w.i == INT_MAX) { dry |= 1u << c; continue; }
            if (t == 0) { sel_v[npick] = w.v; sel_i[npick] = w.i; sel_b[npick] = c; }
            if (h.i == w.i) lists.pop(w.i);
            ++npick;
        }
    }
    // phase 2: the free slots take what is left, fira_beam_select's order
    for (; npick < beam; ++npick) {
        Cand h = Cand::none();
#pragma unroll
        for (int c = 0; c < RQ_BANKS; ++c)
            if (lists.top[c].e[0].before(h)) h = lists.top[c].e[0];
        Cand w = h;
        block16_argmax(w.v, w.i, smv, smi);
        if (t == 0) { sel_v[npick] = w.v; sel_i[npick] = w.i; sel_b[npick] = -1; }   // (the owner names the bank)
        __syncthreads();
        if (w.i != INT_MAX && h.i == w.i) sel_b[npick] = lists.pop(w.i);
    }
    __syncthreads();
    // 5. the written order, then run_model.py:305-340
    if (t < beam) {
        const int idx = sel_i[t];
        const bool none = idx == INT_MAX;                            // fewer than n_beam candidates: fira_beam_select's -1 padding
        const float v = none ? -1.0f : sel_v[t];
        const int bank = none ? -1 : sel_b[t];
        int o = 0;                                                   // picks that are written before this one
        for (int u = 0; u < beam; ++u) {
            const bool un = sel_i[u] == INT_MAX;
            const float uv = un ? -1.0f : sel_v[u];
            const int ub = un ? -1 : sel_b[u];
            const int upos = uv > 0.f, pos = v > 0.f;
            const bool first = upos != pos ? upos > pos : ub != bank ? ub > bank : uv != v ? uv > v : u < t;
            o += (u != t && first) ? 1 : 0;
        }
        const int which = none ? n_act : idx / W, w = none ? 0 : idx - which * W;
        const int carry = which >= n_act;
        const int src = carry ? order[min(w, beam - 1)] : act_slot[which];
        src_of[o] = src; tok_of[o] = entry_word(w, sou, sub, (size_t)b, V, L, S); carry_of[o] = carry;
        const int sl = len_in[r0 + src];
        len_out[r0 + o] = carry ? sl : sl + 1;
        prob_out[r0 + o] = v;
        parent[r0 + o] = r0 + src;
        if (met_out) met_out[r0 + o] = none ? __popc(met_s[src]) : bank;
    }
    __syncthreads();
    write_hypotheses(r0, beam, T, src_of, tok_of, carry_of, gen_in, len_in, gen_out);
}

}  // namespace fira

extern "C" int fira_beam_select_required(void* stream, const fira_dims* d, int B, int n_beam, const float* dist,
                                         const int32_t* finished, const int32_t* active, const int32_t* done, const int32_t* sou,
                                         const int32_t* sub_token, const int32_t* gen_in, const int32_t* len_in,
                                         const float* prob_in, int32_t* gen_out, int32_t* len_out, float* prob_out,
                                         int32_t* parent, const int32_t* required, const int32_t* n_required, int32_t* met_out) {
    using namespace fira;
    FIRA_REQUIRE(d, "fira_beam_select_required: null dims");
    FIRA_REQUIRE(B > 0, "fira_beam_select_required: B = %d must be positive", B);
    FIRA_REQUIRE(n_beam >= 2 && n_beam <= BEAM_MAX, "fira_beam_select_required: n_beam = %d outside 2..%d", n_beam, BEAM_MAX);
    FIRA_REQUIRE(d->tar_len >= 1 && d->tar_len <= ROW_MAX_T, "fira_beam_select_required: tar_len = %d outside 1..%d", d->tar_len,
                 ROW_MAX_T);
    FIRA_REQUIRE(d->vocab > BEAM_MAX && d->vocab <= ROW_MAX_V && d->sou_len >= 0 && d->sub_len >= 0 &&
                     d->sou_len + d->sub_len <= ROW_MAX_SLOTS,
                 "fira_beam_select_required: vocabulary %d / %d memory slots outside %d..%d / 0..%d", d->vocab,
                 d->sou_len + d->sub_len, BEAM_MAX + 1, ROW_MAX_V, ROW_MAX_SLOTS);
    FIRA_REQUIRE(dist && finished && active && done && sou && sub_token && gen_in && len_in && prob_in && gen_out && len_out &&
                     prob_out && parent && required && n_required,
                 "fira_beam_select_required: null pointer (met_out alone may be NULL)");
    const int S = d->sub_len, L = d->sou_len, W = d->vocab + L + S;
#define FIRA_RQ_LAUNCH(NB)                                                                                                      \
    hipLaunchKernelGGL((beam_select_required_kernel<NB>), dim3(B), dim3(DDW_NT), 0, (hipStream_t)stream, n_beam, d->tar_len, W, \
                       d->vocab, L, S, dist, finished, active, done, sou, sub_token, gen_in, len_in, prob_in, required,         \
                       n_required, gen_out, len_out, prob_out, parent, met_out)
    if (n_beam <= 4) FIRA_RQ_LAUNCH(4);
    else FIRA_RQ_LAUNCH(BEAM_MAX);
#undef FIRA_RQ_LAUNCH
    FIRA_CHECK_LAUNCH("fira_beam_select_required");
    return 0;
}
