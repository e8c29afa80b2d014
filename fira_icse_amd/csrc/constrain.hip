// Search constraints on the decode step's output distribution: no-repeat n-gram, minimum length, banned words.
//
// fira_constrain_dist edits dist [R, W] (W = V + L + S: generator ids, diff positions, sub-token positions) in place between
// fira_decode_step and the selection (fira_beam_select / fira_greedy_advance): every entry whose WORD is blocked for the row's
// hypothesis becomes exactly 0.0f, every other element keeps its bits, nothing is renormalised (the search ranks products of
// probabilities: a zero loses to every positive candidate and the ratios among the others are what they were).  The word of
// entry i is what the selection kernels resolve it to: i below V, sou[b, i - V] below V + L, sub_token[b, i - V - L] above -- so
// a blocked word is blocked through its generator id AND through every copy slot that carries it (score.hip's p_word notion).
//
// One workgroup of 1024 threads per row:
//   1. every thread requests the source id of "its" memory slot (L + S <= 1024: one slot per thread, index clamped, nothing
//      behind a branch) and clears the LDS bitmap of W bits; wave 0 reads the hypothesis with lane p on position p (T <= 64) and
//      finds the blocked positions with ballots: with E_k = ballot(h_q == h_{m+1-k}) -- position q carries the k-th word from the
//      end -- position p completes a repeat of the last n - 1 words iff bit p - k of E_k is set for every k in 1 .. n - 1:
//          M = AND_k (E_k << k), restricted to p in [n, m]
//      (p <= m keeps the tail from matching itself as a completed n-gram: its "next word" would be position m + 1).  The words at
//      the set positions, the banned ids inside [0, V) and <eos> while m < min_length go to an LDS list (<= 63 + 32 + 1 words).
//   2. the list marks the bitmap: the generator bit of each word, and the bit of each slot whose source id is in the list
//      (each thread compares its one id against the list: LDS reads at a wave-uniform address).  LDS atomics only.
//   3. with best_id / best_p: one stream_row_marked pass over the row that takes a set bit as the value 0, into an ArgMax.
//   4. the stores: a thread walks "its" bitmap word and stores one 0.0f per set bit -- plain vector stores, no read of the row.
//      Without best_id the row is never read at all: the call costs the bitmap, not the 100 KB of the row.
// A finished row (last id <eos>) has an empty list: nothing is stored and its best is the arg-max of the row as it is.
#include "decode_row.h"

namespace fira {

constexpr int CON_MAX_BAN = 32;
constexpr int CON_MAX_BLK = ROW_MAX_T - 1 + CON_MAX_BAN + 1;
constexpr int CON_EOS = 1;                      // config.EOS

__global__ __launch_bounds__(DDW_NT) void constrain_dist_kernel(int T, int V, int L, int S, int rows_per_commit,
                                                                const int32_t* __restrict__ gen,
                                                                const int32_t* __restrict__ length,
                                                                const int32_t* __restrict__ sou,
                                                                const int32_t* __restrict__ sub, int no_repeat, int min_length,
                                                                const int32_t* __restrict__ banned, int n_banned,
                                                                float* __restrict__ dist, int32_t* __restrict__ best_id,
                                                                float* __restrict__ best_p) {
    __shared__ uint32_t s_bm[bitmap_words(ROW_MAX_V + ROW_MAX_SLOTS)];
    __shared__ int32_t s_blk[CON_MAX_BLK];
    __shared__ int s_nblk;
    __shared__ float smf[DDW_NT / 64];
    __shared__ int smi[DDW_NT / 64];
    const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const size_t b = (size_t)(r / rows_per_commit);
    const int W = V + L + S;
    const int n_words = (W + 31) / 32;

    // ---- 1. requests (unconditional, indices clamped); the bitmap cleared; wave 0 finds the blocked words
    const int src = slot_word(sou, sub, b, L, S, tid);
    for (int w = tid; w <= n_words; w += DDW_NT) s_bm[w] = 0;
    if (tid < 64) {                                        // wave-uniform: all of wave 0
        const int len = min(max(length[r], 1), T);
        const int m = len - 1;                             // words after <start>
        const int h = gen[(size_t)r * T + min(lane, T - 1)];
        const int last = __shfl(h, m, 64);
        const bool finished = last == CON_EOS;
        uint64_t M = 0;
        if (!finished && no_repeat >= 1 && m >= no_repeat) {
            M = ~0ull;
            for (int k = 1; k < no_repeat; ++k) {          // (wave-uniform trip count)
                const int tail = __shfl(h, m + 1 - k, 64); // the k-th word from the end; m + 1 - k >= 2
                M &= __ballot(h == tail) << k;
            }
            const uint64_t upto_m = m >= 63 ? ~0ull : (1ull << (m + 1)) - 1ull;
            M &= upto_m & ~((1ull << no_repeat) - 1ull);   // p in [n, m]; n <= m <= 63
        }
        const int n_rep = __builtin_popcountll(M);
        if ((M >> lane) & 1) s_blk[__builtin_popcountll(M & ((1ull << lane) - 1ull))] = h;
        int ban = lane < n_banned ? banned[lane] : -1;     // (n_banned <= 32 < 64)
        const bool ban_ok = !finished && ban >= 0 && ban < V;
        const uint64_t ban_m = __ballot(ban_ok);
        if (ban_ok) s_blk[n_rep + __builtin_popcountll(ban_m & ((1ull << lane) - 1ull))] = ban;
        int n = n_rep + __builtin_popcountll(ban_m);
        const bool short_yet = !finished && m < min_length;
        if (lane == 0) {
            if (short_yet) s_blk[n] = CON_EOS;
            s_nblk = n + (short_yet ? 1 : 0);
        }
    }
    __syncthreads();
    const int nblk = s_nblk;
    if (nblk == 0 && !best_id) return;                     // (workgroup-uniform) nothing to edit, nothing to report

    // ---- 2. mark: generator bits of the list, slot bits by comparison
    if (nblk > 0) {
        if (tid < nblk) {
            const int w = s_blk[tid];
            if (w >= 0 && w < V) atomicOr(&s_bm[w >> 5], 1u << (w & 31));
        }
        if (tid < L + S) {
            bool hit = false;
            for (int q = 0; q < nblk; ++q) hit |= s_blk[q] == src;
            if (hit) atomicOr(&s_bm[(V + tid) >> 5], 1u << ((V + tid) & 31));
        }
        __syncthreads();
    }

    float* row = dist + (size_t)r * W;
    // ---- 3. arg-max of the edited row
    if (best_id) {
        ArgMax best;
        stream_row_marked(row, W, tid, s_bm, [&](float v, int i, unsigned blocked) { best.offer(blocked ? 0.0f : v, i); });
        best.reduce(smf, smi);
        best.report(best_id, best_p, r);
    }

    // ---- 4. the stores: one 0.0f per set bit (bits exist only below W)
    if (nblk > 0)
        for (int w = tid; w < n_words; w += DDW_NT) {
            uint32_t bits = s_bm[w];
            while (bits) {
                const int i = w * 32 + __builtin_ctz(bits);
                bits &= bits - 1;
                row[i] = 0.0f;
            }
        }
}

}  // namespace fira

extern "C" int fira_constrain_dist(void* stream, const fira_dims* d, int R, int rows_per_commit, const int32_t* gen,
                                   const int32_t* length, const int32_t* sou, const int32_t* sub_token, int no_repeat_ngram,
                                   int min_length, const int32_t* banned, int n_banned, float* dist, int32_t* best_id,
                                   float* best_p) {
    using namespace fira;
    if (int e = require_row_geometry(d, rows_per_commit, R, best_id, best_p, "fira_constrain_dist")) return e;
    FIRA_REQUIRE(d->tar_len >= 2 && d->tar_len <= ROW_MAX_T, "fira_constrain_dist: tar_len = %d outside 2..%d (one lane per position)",
                 d->tar_len, ROW_MAX_T);
    FIRA_REQUIRE(no_repeat_ngram >= 0 && no_repeat_ngram <= d->tar_len, "fira_constrain_dist: no_repeat_ngram = %d outside 0..tar_len = %d",
                 no_repeat_ngram, d->tar_len);
    FIRA_REQUIRE(min_length >= 0 && min_length <= d->tar_len - 2, "fira_constrain_dist: min_length = %d outside 0..tar_len - 2 = %d",
                 min_length, d->tar_len - 2);
    FIRA_REQUIRE(n_banned >= 0 && n_banned <= CON_MAX_BAN, "fira_constrain_dist: n_banned = %d outside 0..%d", n_banned, CON_MAX_BAN);
    FIRA_REQUIRE(n_banned == 0 || banned, "fira_constrain_dist: n_banned = %d without a banned array", n_banned);
    if (R == 0) return 0;
    FIRA_REQUIRE(gen && length && sou && sub_token && dist, "fira_constrain_dist: null pointer (gen, length, sou, sub_token or dist)");
    hipLaunchKernelGGL(constrain_dist_kernel, dim3(R), dim3(DDW_NT), 0, (hipStream_t)stream, d->tar_len, d->vocab, d->sou_len,
                       d->sub_len, rows_per_commit, gen, length, sou, sub_token, no_repeat_ngram, min_length, banned, n_banned, dist,
                       best_id, best_p);
    FIRA_CHECK_LAUNCH("fira_constrain_dist");
    return 0;
}
