// Beam selection under a length-normalised key, in diverse beam groups (include/fira_hip.h).
//
// fira_beam_select_scored is fira_beam_select (beam.hip) with another ranking key.  The state is the same -- gen, length, raw
// probability, double-buffered -- because a hypothesis's key is a function of its (prob, length):
//     key(p, m) = ln(p) * inv_lp[m],   inv_lp[m] = 1 / ((5 + m) / 6)^alpha   (GNMT; fp32 table of the caller),   ln 0 = -inf
// with m the words emitted: length - 1 (<start> is not counted, <eos> is).  Candidates of a step, per commit:
//     running   entry i of running slot j:  p = fp32(dist[j, i] * prob[j])  (the product fira_beam_select forms),  m = len_j
//     carried   a finished hypothesis:      p = prob[j],  m = len_j - 1      (fixed from the moment it finished)
//     void      the entries of a finished hypothesis's row and the padding of the carried list (the two -1 of fira_beam_select)
// Total order: void last, then penalised key descending, then p descending, then the flattened index of fira_beam_select
// ascending (running slots in slot order, then the carried list).  ln is monotone, so at alpha = 0 with one group this is
// (p descending, index ascending): gen / len / prob / parent are then fira_beam_select's bit for bit.
// Groups: the n_beam slots are n_groups groups of k consecutive slots, handled in ascending order.  Group g takes the k best
// among the candidates of ITS OWN slots and writes them to its slots, best first.  The penalised key of a running candidate is
// key - diversity * c, c = the number of picks made earlier in this step, for this commit, by groups < g that EXTENDED a
// hypothesis with the same WORD (multiplicity counts); the word of entry i is the id it resolves to: i below V, the sou /
// sub_token id of its copy slot above -- so the copy head cannot route around the penalty.  Carried candidates are never
// penalised and count for nothing.  The penalty affects the selection only: prob_out is the raw product and key_out the
// unpenalised key(prob_out, len_out - 1).
//
// One workgroup of 1024 threads per commit; the groups are phases inside it.  Per group:
//   1. every running row of the group is streamed once (four loads in flight, nothing behind a branch) into a thread-local
//      TopList (decode_row.h) of the NB best products of the row.  No logarithm is paid per element: within a row all entries
//      share prob[j] and m, so the order by product is the order by unpenalised key.
//   2. the list entries of the row -- best first -- get their key in fp64 (ln of an fp32 product is then strictly monotone in
//      it: two fp32 neighbours are 6e-8 apart in ln, the fp64 logarithm errs by 1e-14) and their penalty count, and are offered
//      to the thread's list of the group.  The walk stops at the first entry whose UNPENALISED key does not enter that list:
//      every later entry of the row ranks below it, penalised or not.
//   3. thread 0 offers the carried candidates; k rounds of a block-wide arg-max pop the winners; k threads resolve them.
//   4. the words the group appended join the LDS list of penalised words (at most n_beam - k words ever get compared).
// No penalised entry is lost to the product-ordered list: a thread owns the entries i = t (mod 1024) of a row, among them at
// most ONE copy slot (sou_len + sub_len <= 1024) and at most n_beam - k generator entries of penalised words (one per earlier
// pick), so at most n_beam - k + 1 of its entries are penalised.  The list holds NB >= k + (n_beam - k + 1) entries (NB >= k with
// one group, where nothing is penalised): the thread's k best unpenalised entries are always on it, and a penalised entry that
// is not on it has k + 1 unpenalised entries of higher product -- hence of higher penalised key -- above it.  The same count
// gives each thread its slot's word once per commit (slot_word): a list entry at or above V is that slot.
// Void candidates are never offered: a group with r running and k - r finished slots has r * W + (k - r) >= k others.
// Plain vector stores, no atomics on global memory.
#include <float.h>
#include <limits.h>
#include <math.h>
#include "engine.h"
#include "decode_row.h"

namespace fira {

constexpr int BS_NT = DDW_NT;

// A candidate of a group: penalised key descending, then Cand's order.
struct KeyCand {
    double k; float p; int i;
    static __device__ __forceinline__ KeyCand none() { return {-INFINITY, -2.0f, INT_MAX}; }        // below every candidate
    __device__ __forceinline__ bool before(const KeyCand& o) const { return k > o.k || (k == o.k && better(p, i, o.p, o.i)); }
};
__device__ __forceinline__ double bs_key(float p, float inv) { return p > 0.0f ? log((double)p) * (double)inv : -INFINITY; }

// NB: length of the per-row product list; KN >= k: length of the thread's list of the group
template <int NB, int KN>
__global__ __launch_bounds__(BS_NT) void beam_select_scored_kernel(
    int beam, int n_groups, int T, int W, int V, int L, int S, float diversity, const float* __restrict__ dist,
    const int32_t* __restrict__ fin, const int32_t* __restrict__ active, const int32_t* __restrict__ done,
    const int32_t* __restrict__ sou, const int32_t* __restrict__ sub, const int32_t* __restrict__ gen_in,
    const int32_t* __restrict__ len_in, const float* __restrict__ prob_in, const float* __restrict__ inv_lp,
    int32_t* __restrict__ gen_out, int32_t* __restrict__ len_out, float* __restrict__ prob_out, int32_t* __restrict__ parent,
    float* __restrict__ key_out) {
    __shared__ double smk[BS_NT / 64];
    __shared__ float smp[BS_NT / 64];
    __shared__ int smi[BS_NT / 64];
    __shared__ float sel_p[BEAM_MAX];
    __shared__ int sel_i[BEAM_MAX], order[BEAM_MAX], src_of[BEAM_MAX], tok_of[BEAM_MAX], carry_of[BEAM_MAX],
        pen_w[BEAM_MAX];
    __shared__ int s_npen;
    const int b = blockIdx.x, t = threadIdx.x, r0 = b * beam, k = beam / n_groups;
    if (*done) {
        pass_through_done(r0, beam, T, gen_in, len_in, prob_in, gen_out, len_out, prob_out, parent);
        if (t < beam && key_out) key_out[r0 + t] = (float)bs_key(prob_in[r0 + t], inv_lp[min(max(len_in[r0 + t] - 1, 0), T)]);
        return;
    }
    // the word of the one copy slot this thread streams: entry V + s with V + s = t (mod 1024)
    const int my_word = slot_word(sou, sub, (size_t)b, L, S, (t - V % BS_NT + BS_NT) % BS_NT);
    const double lam = (double)diversity;
    if (t == 0) s_npen = 0;

    TopList<KN, KeyCand> group;

    for (int g = 0; g < n_groups; ++g) {
        const int j0 = g * k;
        group.clear();
        __syncthreads();                                             // the words of the groups before are listed
        const int npen = s_npen;
        for (int jj = 0; jj < k; ++jj) {
            const int j = j0 + jj;
            if (!active[j] || fin[r0 + j]) continue;                 // (workgroup-uniform) not running: carried below, or void
            const float pj = prob_in[r0 + j];
            const float inv = inv_lp[min(max(len_in[r0 + j], 0), T)];
            const float* row = dist + (size_t)(r0 + j) * W;
            TopList<NB, Cand> top;
            top.clear();
            for (int w0 = t; w0 < W; w0 += 4 * BS_NT) {              // four loads in flight per trip
                float x[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) x[u] = row[min(w0 + u * BS_NT, W - 1)];
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (w0 + u * BS_NT < W) top.offer({x[u] * pj, w0 + u * BS_NT});
            }
            bool live = true;
#pragma unroll
            for (int q = 0; q < NB; ++q) {
                const Cand c = top.e[q];
                if (live && c.i != INT_MAX) {
                    const double uk = bs_key(c.v, inv);
                    const int idx = jj * W + c.i;
                    if (!group.admits({uk, c.v, idx})) {
                        live = false;                                // the rest of the row ranks below this entry
                    } else {
                        const int word = c.i < V ? c.i : my_word;
                        int n_pen = 0;
                        for (int n = 0; n < npen; ++n) n_pen += pen_w[n] == word;
                        group.offer({uk - lam * (double)n_pen, c.v, idx});
                    }
                }
            }
        }
        if (t == 0) {                                                // the group's finished hypotheses, slot order
            int c = 0;
            for (int jj = 0; jj < k; ++jj)
                if (fin[r0 + j0 + jj]) {
                    order[c] = j0 + jj;
                    const float p = prob_in[r0 + j0 + jj];
                    group.offer({bs_key(p, inv_lp[min(max(len_in[r0 + j0 + jj] - 1, 0), T)]), p, k * W + c});
                    ++c;
                }
            for (int q = c; q < k; ++q) order[q] = j0;
        }
        // k rounds of a block-wide arg-max over the list heads; the owner of the winner pops it
        for (int round = 0; round < k; ++round) {
            KeyCand c = group.e[0];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const KeyCand oc = {__shfl_xor(c.k, o, 64), __shfl_xor(c.p, o, 64), __shfl_xor(c.i, o, 64)};
                if (oc.before(c)) c = oc;
            }
            __syncthreads();
            if ((t & 63) == 0) { smk[t >> 6] = c.k; smp[t >> 6] = c.p; smi[t >> 6] = c.i; }
            __syncthreads();
            c = {smk[0], smp[0], smi[0]};
#pragma unroll
            for (int q = 1; q < BS_NT / 64; ++q) {
                const KeyCand oc = {smk[q], smp[q], smi[q]};
                if (oc.before(c)) c = oc;
            }
            if (t == 0) { sel_p[j0 + round] = c.p; sel_i[j0 + round] = c.i; }
            if (group.e[0].i == c.i) group.pop();
        }
        __syncthreads();
        if (t < 64) {                                                // (wave-uniform) lanes 0 .. k - 1 resolve the group's picks
            bool extended = false;
            int nt = 0;
            if (t < k) {
                const int o = j0 + t;
                const int idx = sel_i[o];
                const bool none = idx == INT_MAX;                    // fewer than k candidates: fira_beam_select's -1 padding
                const int which = none ? k : idx / W, w = none ? 0 : idx - which * W;
                const int carry = which >= k;
                const int src = carry ? order[min(w, k - 1)] : j0 + which;
                nt = entry_word(w, sou, sub, (size_t)b, V, L, S);
                src_of[o] = src; tok_of[o] = nt; carry_of[o] = carry;
                const int sl = len_in[r0 + src];
                const int lo = carry ? sl : sl + 1;
                const float p = none ? -1.0f : sel_p[o];
                len_out[r0 + o] = lo;
                prob_out[r0 + o] = p;
                parent[r0 + o] = r0 + src;
                if (key_out) key_out[r0 + o] = (float)bs_key(p, inv_lp[min(max(lo - 1, 0), T)]);
                extended = !carry;
            }
            const unsigned long long m = __ballot(extended);
            if (extended) pen_w[npen + __popcll(m & ((1ull << t) - 1ull))] = nt;
            if (t == 0) s_npen = npen + __popcll(m);
        }
    }
    __syncthreads();
    write_hypotheses(r0, beam, T, src_of, tok_of, carry_of, gen_in, len_in, gen_out);
}

}  // namespace fira

extern "C" int fira_beam_select_scored(void* stream, const fira_dims* d, int B, int n_beam, const float* dist,
                                       const int32_t* finished, const int32_t* active, const int32_t* done, const int32_t* sou,
                                       const int32_t* sub_token, const int32_t* gen_in, const int32_t* len_in,
                                       const float* prob_in, int32_t* gen_out, int32_t* len_out, float* prob_out,
                                       int32_t* parent, const float* inv_lp, int n_groups, float diversity, float* key_out) {
    using namespace fira;
    FIRA_REQUIRE(d, "fira_beam_select_scored: null dims");
    FIRA_REQUIRE(B > 0, "fira_beam_select_scored: B = %d must be positive", B);
    FIRA_REQUIRE(n_beam >= 2 && n_beam <= BEAM_MAX, "fira_beam_select_scored: n_beam = %d outside 2..%d", n_beam, BEAM_MAX);
    FIRA_REQUIRE(n_groups >= 1 && n_beam % n_groups == 0, "fira_beam_select_scored: n_groups = %d must be >= 1 and divide n_beam = %d",
                 n_groups, n_beam);
    FIRA_REQUIRE(diversity >= 0.0f && diversity <= FLT_MAX, "fira_beam_select_scored: diversity = %g must be finite and >= 0",
                 (double)diversity);
    FIRA_REQUIRE(d->tar_len >= 1 && d->tar_len <= ROW_MAX_T, "fira_beam_select_scored: tar_len = %d outside 1..%d (inv_lp has tar_len + 1 entries)",
                 d->tar_len, ROW_MAX_T);
    FIRA_REQUIRE(d->vocab > BEAM_MAX && d->sou_len >= 0 && d->sub_len >= 0 && d->sou_len + d->sub_len <= ROW_MAX_SLOTS,
                 "fira_beam_select_scored: vocabulary %d / %d memory slots outside %d.. / 0..%d", d->vocab, d->sou_len + d->sub_len,
                 BEAM_MAX + 1, ROW_MAX_SLOTS);
    FIRA_REQUIRE(dist && finished && active && done && sou && sub_token && gen_in && len_in && prob_in && gen_out && len_out &&
                     prob_out && parent && inv_lp,
                 "fira_beam_select_scored: null pointer (key_out alone may be NULL)");
    const int S = d->sub_len, L = d->sou_len, W = d->vocab + L + S, k = n_beam / n_groups;
    const int need = n_groups == 1 ? n_beam : n_beam + 1;            // entries of a row one thread must keep (see the top)
#define FIRA_BS_LAUNCH(NB, KN)                                                                                                  \
    hipLaunchKernelGGL((beam_select_scored_kernel<NB, KN>), dim3(B), dim3(BS_NT), 0, (hipStream_t)stream, n_beam, n_groups,     \
                       d->tar_len, W, d->vocab, L, S, diversity, dist, finished, active, done, sou, sub_token, gen_in, len_in,  \
                       prob_in, inv_lp, gen_out, len_out, prob_out, parent, key_out)
    if (need <= 4) FIRA_BS_LAUNCH(4, 4);
    else if (need <= 8 && k <= 4) FIRA_BS_LAUNCH(8, 4);
    else if (need <= 8) FIRA_BS_LAUNCH(8, 8);
    else FIRA_BS_LAUNCH(9, 4);                                       // n_beam 8 in groups: k <= 4
#undef FIRA_BS_LAUNCH
    FIRA_CHECK_LAUNCH("fira_beam_select_scored");
    return 0;
}
