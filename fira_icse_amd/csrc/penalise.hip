// Soft word penalties and biases on the decode step's output distribution: presence / frequency penalties, a per-word bias.
//
// fira_penalise_dist edits dist [R, W] (W = V + L + S: generator ids, diff positions, sub-token positions) in place, last in the
// edit chain (after fira_merge_dist, fira_force_dist, fira_constrain_dist) and before the selection.  It is the soft sibling of
// fira_constrain_dist, with its geometry and its definitions: that kernel sets the entries of a blocked WORD to 0, this one
// multiplies the entries of a word by a factor.  Row r of commit b = r / rows_per_commit holds the hypothesis gen[r, 0 .. len),
// len = clamp(length[r], 1, T), m = len - 1 words after <start>; a row whose last id is <eos> is finished and is not touched.
// For an unfinished row, with c(w) = the number of positions p in 1 .. m with gen[r, p] == w:
//     dist[i] <- fl32(dist[i] * count_factor[c(w(i))])       for every entry i with c(w(i)) > 0, then
//     dist[i] <- fl32(dist[i] * bias_factor[b, q])           for every entry i with w(i) == bias_id[b, q], the first such q below
//                                                            min(max(n_bias[b], 0), 16), once
// two fp32 multiplications that round separately, in that order.  w(i) is what the selection kernels resolve entry i to
// (constrain.hip), so a word is reached through its generator entry AND through every copy slot that carries it; <eos> is no
// exception.  Every other element keeps its bits; nothing is renormalised.  A bias id outside [0, V) is ignored.
//
// One workgroup of 1024 threads per row:
//   1. every thread requests the source id (slot_word) and the value of "its" copy slot (L + S <= 1024: one slot per thread, index
//      clamped, nothing behind a branch) and, with best_id, clears the LDS bitmap of W bits.  Wave 0 reads the hypothesis with
//      lane p on position p (T <= 64) and the commit's bias list with lane q on pair q (requested before the hypothesis is
//      looked at), counts every position's word over the wave (m readlanes), and writes ONE list to LDS: the distinct emitted
//      words (the lane of a word's first position is its leader) with f1 = count_factor[c] and f2 = the bias factor of the word if
//      it is biased too, else 1; then the biased words that were not emitted, with f1 = 1.  At most 63 + 16 words, pairwise
//      distinct -- so no two threads below ever read-modify-write one address, and one phase serves both edits.
//      (x * 1.0f == x bit for bit, so the absent factor is spelled 1.)
//   2. thread k below the list's length owns word k: it requests the generator entry (index clamped), multiplies twice and
//      stores, if the word is inside [0, V).  The thread of a slot compares its source id against the list (LDS reads at a
//      wave-uniform address) and multiplies and stores its own value on a hit.  Plain vector stores, no atomics on global memory.
//   3. with best_id / best_p: the arg-max of the row AS STORED (ArgMax), without reading back the stores of step 2: the touched
//      entries are marked in the bitmap (LDS atomics) and offered by the threads that hold their new values; one
//      stream_row_marked pass over the row skips the marked entries.
// Without best_id the row is read at the copy slots (4 (L + S) bytes, requested at entry so that the round trip runs under the
// list's construction) and at the touched generator entries only.  A finished row has an empty list: nothing is stored, and its
// best is the arg-max of the row as it is.
#include "decode_row.h"

namespace fira {

constexpr int PEN_MAX_BIAS = 16;
constexpr int PEN_MAX_LIST = ROW_MAX_T - 1 + PEN_MAX_BIAS;
constexpr int PEN_EOS = 1;                      // config.EOS

__global__ __launch_bounds__(DDW_NT) void penalise_dist_kernel(int T, int V, int L, int S, int rows_per_commit,
                                                               const int32_t* __restrict__ gen,
                                                               const int32_t* __restrict__ length,
                                                               const int32_t* __restrict__ sou,
                                                               const int32_t* __restrict__ sub,
                                                               const float* __restrict__ count_factor,
                                                               const int32_t* __restrict__ bias_id,
                                                               const float* __restrict__ bias_factor,
                                                               const int32_t* __restrict__ n_bias,
                                                               float* __restrict__ dist, int32_t* __restrict__ best_id,
                                                               float* __restrict__ best_p) {
    __shared__ uint32_t s_bm[bitmap_words(ROW_MAX_V + ROW_MAX_SLOTS)];
    __shared__ int32_t s_w[PEN_MAX_LIST];
    __shared__ float s_f1[PEN_MAX_LIST], s_f2[PEN_MAX_LIST];
    __shared__ int s_n;
    __shared__ float smf[DDW_NT / 64];
    __shared__ int smi[DDW_NT / 64];
    const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const size_t b = (size_t)(r / rows_per_commit);
    const int NS = L + S, W = V + NS;
    float* row = dist + (size_t)r * W;

    // ---- 1. requests (unconditional, indices clamped); the bitmap cleared; wave 0 builds the list
    const float p = NS > 0 ? row[V + min(tid, NS - 1)] : 0.0f;
    const int src = slot_word(sou, sub, b, L, S, tid);
    if (best_id)
        for (int w = tid; w <= (W + 31) / 32; w += DDW_NT) s_bm[w] = 0;
    if (tid < 64) {                                        // wave-uniform: all of wave 0
        const int q16 = lane & (PEN_MAX_BIAS - 1);
        const int bid = bias_id[b * PEN_MAX_BIAS + q16];
        const float bfac = bias_factor[b * PEN_MAX_BIAS + q16];
        const int nb = min(max(n_bias[b], 0), PEN_MAX_BIAS);
        const int len = min(max(length[r], 1), T);
        const int m = len - 1;                             // words after <start>
        const int h = gen[(size_t)r * T + min(lane, T - 1)];
        const bool finished = __shfl(h, m, 64) == PEN_EOS;
        const bool pos = !finished && lane >= 1 && lane <= m;
        int cnt = 0;
        bool lead = pos;                                   // the first position of its word
        for (int k = 1; k <= m; ++k) {                     // (wave-uniform trip count)
            const bool same = __shfl(h, k, 64) == h;
            cnt += same ? 1 : 0;
            lead = lead && !(same && k < lane);
        }
        const float cf = count_factor[min(max(cnt, 1), T - 1)];      // (c <= m <= T - 1; entry 0 is never read)
        bool bok = !finished && lane < nb && bid >= 0 && bid < V;
        float f2 = 1.0f;
        bool biased = false;
        for (int q = 0; q < PEN_MAX_BIAS; ++q) {           // pair q against every leader; a later pair of the same id is dropped
            const int id_q = __shfl(bid, q, 64);
            const float f_q = __shfl(bfac, q, 64);
            const bool ok_q = __shfl((int)bok, q, 64) != 0;
            if (ok_q && lane > q && bid == id_q) bok = false;
            if (ok_q && lead && !biased && h == id_q) { f2 = f_q; biased = true; }
        }
        bool alone = bok;                                  // a biased word that was not emitted
        for (int q = 0; q < PEN_MAX_BIAS; ++q) {
            const int id_q = __shfl(bid, q, 64);
            if (__ballot(lead && h == id_q) != 0ull && lane == q) alone = false;
        }
        const uint64_t lead_m = __ballot(lead), alone_m = __ballot(alone);
        const uint64_t below = (1ull << lane) - 1ull;
        const int n_lead = __builtin_popcountll(lead_m);
        if (lead) {
            const int k = __builtin_popcountll(lead_m & below);
            s_w[k] = h; s_f1[k] = cf; s_f2[k] = f2;
        }
        if (alone) {
            const int k = n_lead + __builtin_popcountll(alone_m & below);
            s_w[k] = bid; s_f1[k] = 1.0f; s_f2[k] = bfac;
        }
        if (lane == 0) s_n = n_lead + __builtin_popcountll(alone_m);
    }
    __syncthreads();
    const int n = s_n;
    if (n == 0 && !best_id) return;                        // (workgroup-uniform) nothing to edit, nothing to report

    // ---- 2. the edits: the generator entry of list word tid, the thread's own slot on a hit
    bool own = false, hit = false;
    int w = 0;
    float g_new = 0.0f, p_new = 0.0f;
    if ((tid & ~63) < n) {                                 // (wave-uniform) this wave owns at least one list word
        const int k = min(tid, n - 1);
        w = s_w[k];
        own = tid < n && w >= 0 && w < V;                  // a word outside [0, V) is never used as an index
        w = own ? w : 0;
        const float g = row[w];
        g_new = g * s_f1[k];
        g_new = g_new * s_f2[k];
        if (own) row[w] = g_new;
    }
    if ((tid & ~63) < NS && n > 0) {                       // (wave-uniform) this wave owns at least one slot
        int at = -1;
        for (int q = 0; q < n; ++q) at = s_w[q] == src ? q : at;     // (the list's words are distinct: at most one hit)
        hit = tid < NS && at >= 0;
        const int k = max(at, 0);
        p_new = p * s_f1[k];
        p_new = p_new * s_f2[k];
        if (hit) row[V + tid] = p_new;
    }
    if (!best_id) return;                                  // (workgroup-uniform)

    // ---- 3. arg-max of the stored row: the touched entries from their threads, the rest streamed
    if (own) atomicOr(&s_bm[w >> 5], 1u << (w & 31));
    if (hit) atomicOr(&s_bm[(V + tid) >> 5], 1u << ((V + tid) & 31));
    __syncthreads();
    ArgMax best;
    if (own) best.offer(g_new, w);
    if (hit) best.offer(p_new, V + tid);
    stream_row_marked(row, W, tid, s_bm, [&](float v, int i, unsigned marked) {
        if (!marked) best.offer(v, i);
    });
    best.reduce(smf, smi);
    best.report(best_id, best_p, r);
}

}  // namespace fira

extern "C" int fira_penalise_dist(void* stream, const fira_dims* d, int R, int rows_per_commit, const int32_t* gen,
                                  const int32_t* length, const int32_t* sou, const int32_t* sub_token, const float* count_factor,
                                  const int32_t* bias_id, const float* bias_factor, const int32_t* n_bias, float* dist,
                                  int32_t* best_id, float* best_p) {
    using namespace fira;
    if (int e = require_row_geometry(d, rows_per_commit, R, best_id, best_p, "fira_penalise_dist")) return e;
    FIRA_REQUIRE(d->tar_len >= 2 && d->tar_len <= ROW_MAX_T, "fira_penalise_dist: tar_len = %d outside 2..%d (one lane per position)",
                 d->tar_len, ROW_MAX_T);
    if (R == 0) return 0;
    FIRA_REQUIRE(gen && length && sou && sub_token && dist, "fira_penalise_dist: null pointer (gen, length, sou, sub_token or dist)");
    FIRA_REQUIRE(count_factor, "fira_penalise_dist: null pointer (count_factor)");
    FIRA_REQUIRE(bias_id && bias_factor && n_bias, "fira_penalise_dist: null pointer (bias_id, bias_factor or n_bias)");
    hipLaunchKernelGGL(penalise_dist_kernel, dim3(R), dim3(DDW_NT), 0, (hipStream_t)stream, d->tar_len, d->vocab, d->sou_len,
                       d->sub_len, rows_per_commit, gen, length, sou, sub_token, count_factor, bias_id, bias_factor, n_bias, dist,
                       best_id, best_p);
    FIRA_CHECK_LAUNCH("fira_penalise_dist");
    return 0;
}
