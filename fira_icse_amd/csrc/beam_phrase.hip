// Lexically constrained beam search over PHRASES: the selection step with dynamic beam allocation where a required item is a word
// sequence (include/fira_hip.h; Post and Vilar, NAACL 2018, who define the banks for phrases).
//
// fira_beam_select_phrases is fira_beam_select_required (beam_require.hip) with one change: how a candidate's bank is decided.
// Per commit b the items are given flattened: n = n_items[b] clamped to 0..4 items, item k of l_k = item_len[b, k] words (clamped
// so that the lengths sum to at most 4), its words words[b, o_k .. o_k + l_k) with o_k = l_0 + .. + l_{k-1}; total = sum l_k.
// For a hypothesis h = gen[1 .. len - 1]:
//     done(h)     = { k : item k occurs contiguously in h }
//     partial(h)  = the largest q >= 1 such that some item k outside done(h) has q < l_k and its first q words are the last q
//                   words of h; 0 if there is none
//     progress(h) = sum of l_k over done(h) + partial(h),    bank(h) = progress(h) in 0 .. total
// -- a function of the gen row alone, so the state is fira_beam_select's.  Candidates, in fira_beam_select's flattened order:
//     running   entry i of running slot j:  p = fp32(dist[j, i] * prob[j]),  bank = progress(h_j . w(i))
//     carried   a finished hypothesis:  p = prob[j],  bank = progress(h_j)
//     void      fira_beam_select's two -1, and every entry with w(i) == <eos> of a running row with progress(h_j) < total
// Everything else is beam_require.hip's header with C = total: the round robin from the fullest bank down, the fill phase, the
// written order, the resolution of entries, met_out = the progress of every written hypothesis, the `done` pass-through, and the
// argument that a void candidate is never reached.  With every item one word long the five outputs are
// fira_beam_select_required's bit for bit; with no item they are fira_beam_select's.
//
// The streaming structure.  Appending a word w to h_j changes done() only if w completes an item whose other words are the tail of
// h_j, and gives a partial credit only if w continues (or starts) such an item.  So with S(k, q) = "the first q words of item k
// are the last q words of h_j" (S(k, 0) always holds) the EXCEPTION words of a row are
//     X = { item k's word q : k outside done(h_j), 0 <= q < l_k, S(k, q) }              at most sum l_k <= 4 words
// and every other word leaves the row in bank D_j = sum of l_k over done(h_j): the bank WITHOUT h_j's partial credit, which an
// unrelated word loses.  progress(h_j . w) of an exception word follows from done(h_j) and the S(k, q) alone:
//     done'    = done(h_j) u { k : S(k, l_k - 1) and item k's last word == w }
//     partial' = max { q : k outside done', 1 <= q < l_k, S(k, q - 1), item k's word q - 1 == w }
// worked out once per row and exception word, never per entry.
//
// One workgroup of 1024 threads per commit.
//   1. wave j forms done(h_j) and the S(k, q) of its hypothesis: lane p holds gen[j, p] and its three successors (shuffles), one
//      ballot per item; the last three words are wave-uniform readlanes.  16 + 4 bits and the progress per slot go to LDS.
//   2. every running row is streamed once with fira_beam_select's loop into the thread's TopList of bank D_j (workgroup-uniform,
//      chosen outside the loop); an entry whose word is in X is kept apart: a copy slot's entry (a thread owns one slot) aside,
//      the at most 4 generator entries re-read by threads 0 .. 3 after the loop (4 bytes each).
//   3. - 5. beam_require.hip's: the carried candidates, the two phases, the written order.
// Plain vector stores, no atomics on global memory.
#include <limits.h>
#include "engine.h"
#include "decode_row.h"

namespace fira {

constexpr int PH_MAX = 4;                       // items per commit, words per item, and words per commit
constexpr int PH_BANKS = PH_MAX + 1;
constexpr int PH_EOS = 1;                       // <eos> (config.EOS)
constexpr int PH_NONE = INT_MIN;                // no word

// The thread's lists, one per bank (beam_require.hip's BankLists): indexed through unrolled chains, so they stay in registers.
template <int NB>
struct PhraseBanks {
    TopList<NB, Cand> top[PH_BANKS];
    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int c = 0; c < PH_BANKS; ++c) top[c].clear();
    }
    __device__ __forceinline__ void offer(int bank, const Cand& cd) {
#pragma unroll
        for (int c = 0; c < PH_BANKS; ++c)
            if (c == bank) top[c].offer(cd);
    }
    __device__ __forceinline__ Cand head(int bank) const {
        Cand h = Cand::none();
#pragma unroll
        for (int c = 0; c < PH_BANKS; ++c)
            if (c == bank) h = top[c].e[0];
        return h;
    }
    __device__ __forceinline__ int pop(int idx) {
        int bank = -1;
#pragma unroll
        for (int c = 0; c < PH_BANKS; ++c)
            if (bank < 0 && top[c].e[0].i == idx) { top[c].pop(); bank = c; }
        return bank;
    }
};

// A commit's items, workgroup-uniform: w[k][q] is word q of item k (looked at below len[k] only).
struct PhraseItems {
    int len[PH_MAX], w[PH_MAX][PH_MAX], total;
    __device__ __forceinline__ void load(const int32_t* __restrict__ words, const int32_t* __restrict__ item_len,
                                         const int32_t* __restrict__ n_items, size_t b) {
        int f[PH_MAX], l[PH_MAX];
#pragma unroll
        for (int e = 0; e < PH_MAX; ++e) { f[e] = words[b * PH_MAX + e]; l[e] = item_len[b * PH_MAX + e]; }
        const int n = min(max(n_items[b], 0), PH_MAX);
        int off = 0;
#pragma unroll
        for (int k = 0; k < PH_MAX; ++k) {
            len[k] = k < n ? min(max(l[k], 0), PH_MAX - off) : 0;
#pragma unroll
            for (int q = 0; q < PH_MAX; ++q) {
                const int e = off + q;
                w[k][q] = e == 0 ? f[0] : e == 1 ? f[1] : e == 2 ? f[2] : f[3];
            }
            off += len[k];
        }
        total = off;
    }
    // sum of l_k over the set bits of `done`
    __device__ __forceinline__ int credit(int done) const {
        int s = 0;
#pragma unroll
        for (int k = 0; k < PH_MAX; ++k) s += (done >> k & 1) ? len[k] : 0;
        return s;
    }
    // partial(h) from done(h) and the bits S(k, q) at bit 4 k + q of `suf`
    __device__ __forceinline__ int partial(int done, int suf) const {
        int p = 0;
#pragma unroll
        for (int k = 0; k < PH_MAX; ++k)
#pragma unroll
            for (int q = 1; q < PH_MAX; ++q)
                if (!(done >> k & 1) && q < len[k] && (suf >> (4 * k + q) & 1)) p = max(p, q);
        return p;
    }
    // progress(h . word) from done(h) and the S(k, q) of h
    __device__ __forceinline__ int progress_after(int word, int done, int suf) const {
        int nd = done;
#pragma unroll
        for (int k = 0; k < PH_MAX; ++k)
#pragma unroll
            for (int q = 0; q < PH_MAX; ++q)
                if (q == len[k] - 1 && (suf >> (4 * k + q) & 1) && w[k][q] == word) nd |= 1 << k;
        int p = 0;
#pragma unroll
        for (int k = 0; k < PH_MAX; ++k)
#pragma unroll
            for (int q = 1; q < PH_MAX; ++q)
                if (!(nd >> k & 1) && q < len[k] && (suf >> (4 * k + q - 1) & 1) && w[k][q - 1] == word) p = max(p, q);
        return min(credit(nd) + p, PH_MAX);
    }
};

template <int NB>
__global__ __launch_bounds__(DDW_NT) void beam_select_phrases_kernel(
    int beam, int T, int W, int V, int L, int S, const float* __restrict__ dist, const int32_t* __restrict__ fin,
    const int32_t* __restrict__ active, const int32_t* __restrict__ done, const int32_t* __restrict__ sou,
    const int32_t* __restrict__ sub, const int32_t* __restrict__ gen_in, const int32_t* __restrict__ len_in,
    const float* __restrict__ prob_in, const int32_t* __restrict__ words, const int32_t* __restrict__ item_len,
    const int32_t* __restrict__ n_items, int32_t* __restrict__ gen_out, int32_t* __restrict__ len_out,
    float* __restrict__ prob_out, int32_t* __restrict__ parent, int32_t* __restrict__ met_out) {
    __shared__ float smv[DDW_NT / 64];
    __shared__ int smi[DDW_NT / 64];
    __shared__ float sel_v[BEAM_MAX];
    __shared__ int sel_i[BEAM_MAX], sel_b[BEAM_MAX], act_slot[BEAM_MAX], order[BEAM_MAX], src_of[BEAM_MAX], tok_of[BEAM_MAX],
        carry_of[BEAM_MAX], done_s[BEAM_MAX], suf_s[BEAM_MAX], prog_s[BEAM_MAX];
    const int b = blockIdx.x, t = threadIdx.x, r0 = b * beam;
    PhraseItems it;
    it.load(words, item_len, n_items, (size_t)b);
    const int C = it.total;

    // 1. done(h_j), S(k, q) and progress(h_j) of the commit's hypotheses: wave j, one position per lane (T <= 64)
    if ((t >> 6) < beam) {
        const int j = t >> 6, p = t & 63;
        const int len = min(max(len_in[r0 + j], 1), T);
        const int m = len - 1;
        const int g = gen_in[(size_t)(r0 + j) * T + min(p, T - 1)];
        int g_at[PH_MAX];                                            // the words at p, p + 1, p + 2, p + 3
        g_at[0] = g;
#pragma unroll
        for (int u = 1; u < PH_MAX; ++u) g_at[u] = __shfl(g, min(p + u, 63), 64);
        // t_k: the k-th word from the end (looked at only where k <= m)
        const int t1 = __shfl(g, max(m, 0), 64), t2 = __shfl(g, max(m - 1, 0), 64), t3 = __shfl(g, max(m - 2, 0), 64);
        int dn = 0, suf = 0;
#pragma unroll
        for (int k = 0; k < PH_MAX; ++k) {
            const int l = it.len[k];
            bool at = l >= 1 && p >= 1 && p + l - 1 <= m;            // item k begins at position p
#pragma unroll
            for (int u = 0; u < PH_MAX; ++u) at = at && (u >= l || g_at[u] == it.w[k][u]);
            if (__ballot(at) != 0ull) dn |= 1 << k;
            suf |= 1 << (4 * k);
            if (m >= 1 && it.w[k][0] == t1) suf |= 2 << (4 * k);
            if (m >= 2 && it.w[k][0] == t2 && it.w[k][1] == t1) suf |= 4 << (4 * k);
            if (m >= 3 && it.w[k][0] == t3 && it.w[k][1] == t2 && it.w[k][2] == t1) suf |= 8 << (4 * k);
        }
        if (p == 0) { done_s[j] = dn; suf_s[j] = suf; prog_s[j] = min(it.credit(dn) + it.partial(dn, suf), PH_MAX); }
    }
    __syncthreads();
    if (*done) {
        pass_through_done(r0, beam, T, gen_in, len_in, prob_in, gen_out, len_out, prob_out, parent);
        if (t < beam && met_out) met_out[r0 + t] = prog_s[t];
        return;
    }
    const int n_act = active[BEAM_MAX];
    // the word of the one copy slot this thread streams: entry V + s with V + s = t (mod 1024)
    const int my_word = slot_word(sou, sub, (size_t)b, L, S, (t - V % DDW_NT + DDW_NT) % DDW_NT);

    PhraseBanks<NB> lists;
    lists.clear();
    // 2. the running rows
    int k = 0;
    for (int j = 0; j < beam; ++j) {
        if (!active[j]) continue;
        if (t == 0) act_slot[k] = j;
        if (!fin[r0 + j]) {                                          // (workgroup-uniform) a finished row is void
            const int dj = __builtin_amdgcn_readfirstlane(done_s[j]), sj = __builtin_amdgcn_readfirstlane(suf_s[j]);
            const int bj = min(it.credit(dj), PH_MAX);               // the bank of the row's ordinary entries
            const bool no_eos = __builtin_amdgcn_readfirstlane(prog_s[j]) < C;
            // the exception words of the row (flattened item positions) and their banks
            int X[PH_MAX], PX[PH_MAX];
#pragma unroll
            for (int e = 0; e < PH_MAX; ++e) X[e] = PH_NONE;
            {
                int off = 0;
#pragma unroll
                for (int kk = 0; kk < PH_MAX; ++kk) {
#pragma unroll
                    for (int q = 0; q < PH_MAX; ++q) {
                        const bool ok = q < it.len[kk] && !(dj >> kk & 1) && (sj >> (4 * kk + q) & 1);
                        const int e = off + q;
#pragma unroll
                        for (int x = 0; x < PH_MAX; ++x)
                            if (ok && x == e) X[x] = it.w[kk][q];
                    }
                    off += it.len[kk];
                }
            }
#pragma unroll
            for (int e = 0; e < PH_MAX; ++e) PX[e] = X[e] == PH_NONE ? 0 : it.progress_after(X[e], dj, sj);
            const float pj = prob_in[r0 + j];
            const float* row = dist + (size_t)(r0 + j) * W;
            Cand aside = Cand::none();                               // this thread's exception copy entry of the row
            int aside_bank = 0;
#pragma unroll
            for (int c = 0; c < PH_BANKS; ++c) {
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
                            int hit = -1;                            // the bank of an exception word
#pragma unroll
                            for (int e = 0; e < PH_MAX; ++e) hit = (X[e] != PH_NONE && X[e] == word) ? PX[e] : hit;
                            const Cand cd = {x[u] * pj, k * W + i};
                            if (no_eos && word == PH_EOS) {
                                // void
                            } else if (hit < 0) {
                                lists.top[c].offer(cd);
                            } else if (i >= V) {
                                aside = cd; aside_bank = hit;
                            }                                        // (an exception generator entry: below)
                        }
                    }
                }
            }
            if (aside.i != INT_MAX) lists.offer(aside_bank, aside);
            // the exception generator entries: thread e takes X[e] if it is a word inside the generator's range, not <eos> while
            // that is void, and not listed at a lower place (a duplicate would be offered twice)
            if (t < PH_MAX) {
                int word = X[0], bank = PX[0];
                bool first = true;
#pragma unroll
                for (int e = 1; e < PH_MAX; ++e)
                    if (t == e) { word = X[e]; bank = PX[e]; }
#pragma unroll
                for (int e = 0; e < PH_MAX; ++e) first = first && !(e < t && X[e] == word);
                if (first && word != PH_NONE && word >= 0 && word < V && !(no_eos && word == PH_EOS))
                    lists.offer(bank, {row[word] * pj, k * W + word});
            }
        }
        ++k;
    }
    // 3. the carried candidates: finished hypotheses in slot order (the -1 padding is void)
    if (t == 0) {
        int c = 0;
        for (int j = 0; j < beam; ++j)
            if (fin[r0 + j]) { order[c] = j; lists.offer(prog_s[j], {prob_in[r0 + j], n_act * W + c}); ++c; }
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
        for (int c = 0; c < PH_BANKS; ++c)
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
        if (met_out) met_out[r0 + o] = none ? prog_s[src] : bank;
    }
    __syncthreads();
    write_hypotheses(r0, beam, T, src_of, tok_of, carry_of, gen_in, len_in, gen_out);
}

}  // namespace fira

extern "C" int fira_beam_select_phrases(void* stream, const fira_dims* d, int B, int n_beam, const float* dist,
                                        const int32_t* finished, const int32_t* active, const int32_t* done, const int32_t* sou,
                                        const int32_t* sub_token, const int32_t* gen_in, const int32_t* len_in,
                                        const float* prob_in, int32_t* gen_out, int32_t* len_out, float* prob_out,
                                        int32_t* parent, const int32_t* words, const int32_t* item_len, const int32_t* n_items,
                                        int32_t* met_out) {
    using namespace fira;
    FIRA_REQUIRE(d, "fira_beam_select_phrases: null dims");
    FIRA_REQUIRE(B > 0, "fira_beam_select_phrases: B = %d must be positive", B);
    FIRA_REQUIRE(n_beam >= 2 && n_beam <= BEAM_MAX, "fira_beam_select_phrases: n_beam = %d outside 2..%d", n_beam, BEAM_MAX);
    FIRA_REQUIRE(d->tar_len >= 1 && d->tar_len <= ROW_MAX_T, "fira_beam_select_phrases: tar_len = %d outside 1..%d", d->tar_len,
                 ROW_MAX_T);
    FIRA_REQUIRE(d->vocab > BEAM_MAX && d->vocab <= ROW_MAX_V && d->sou_len >= 0 && d->sub_len >= 0 &&
                     d->sou_len + d->sub_len <= ROW_MAX_SLOTS,
                 "fira_beam_select_phrases: vocabulary %d / %d memory slots outside %d..%d / 0..%d", d->vocab,
                 d->sou_len + d->sub_len, BEAM_MAX + 1, ROW_MAX_V, ROW_MAX_SLOTS);
    FIRA_REQUIRE(dist && finished && active && done && sou && sub_token && gen_in && len_in && prob_in && gen_out && len_out &&
                     prob_out && parent && words && item_len && n_items,
                 "fira_beam_select_phrases: null pointer (met_out alone may be NULL)");
    const int S = d->sub_len, L = d->sou_len, W = d->vocab + L + S;
#define FIRA_PH_LAUNCH(NB)                                                                                                     \
    hipLaunchKernelGGL((beam_select_phrases_kernel<NB>), dim3(B), dim3(DDW_NT), 0, (hipStream_t)stream, n_beam, d->tar_len, W, \
                       d->vocab, L, S, dist, finished, active, done, sou, sub_token, gen_in, len_in, prob_in, words, item_len,  \
                       n_items, gen_out, len_out, prob_out, parent, met_out)
    if (n_beam <= 4) FIRA_PH_LAUNCH(4);
    else FIRA_PH_LAUNCH(BEAM_MAX);
#undef FIRA_PH_LAUNCH
    FIRA_CHECK_LAUNCH("fira_beam_select_phrases");
    return 0;
}
