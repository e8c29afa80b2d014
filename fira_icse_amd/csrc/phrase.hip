// Banned phrases on the decode step's output distribution: the word that would complete a listed n-gram is blocked.
//
// fira_ban_phrases_dist edits dist [R, W] (W = V + L + S: generator ids, diff positions, sub-token positions) in place, a link of
// the edit chain after fira_constrain_dist and before fira_penalise_dist.  It is no_repeat_ngram's mechanism (constrain.hip) with
// the n-grams GIVEN instead of taken from the hypothesis, and it has that kernel's geometry and definitions.  Row r of commit
// b = r / rows_per_commit holds the hypothesis gen[r, 0 .. len), len = clamp(length[r], 1, T), m = len - 1 words after <start>; a
// row whose last id is <eos> is finished and is not touched.  Commit b lists n = clamp(n_phrases[b], 0, 8) phrases; phrase q is
// the words phrase[b, q, 0 .. l) with l = phrase_len[b, q]; a phrase with l outside 2..4 is ignored.  For an unfinished row:
//     phrase (w_1 .. w_l) blocks w_l  iff  m >= l - 1 and (h_{m-l+2} .. h_m) == (w_1 .. w_{l-1})
// and every entry whose WORD is blocked -- the generator id and every copy slot that carries it -- becomes exactly 0.0f.  Every
// other element keeps its bits; nothing is renormalised.  Prefix words are part of gen, so they count as emitted.
//
// One workgroup of 1024 threads per row:
//   1. every thread requests the source id of "its" memory slot (L + S <= 1024, index clamped, nothing behind a branch) and clears
//      the LDS bitmap of W bits.  Wave 0 reads the hypothesis with lane p on position p (T <= 64) and the commit's list with lane q
//      on phrase q mod 8 (16 bytes of words and the length, requested before the hypothesis is looked at).  The last three words
//      t_1, t_2, t_3 of the hypothesis are wave-uniform (readlanes); lane q compares its phrase's first l - 1 words with them and a
//      ballot compacts the blocked last words into an LDS list of at most 8 entries (two phrases may block one word: the list
//      then holds it twice, and the bitmap takes it once).
//   2. the list marks the bitmap: the generator bit of each word, the bit of each slot whose source id is in the list.  LDS atomics.
//   3. with best_id / best_p: one stream_row_marked pass that takes a set bit as the value 0, into an ArgMax.
//   4. the stores: one 0.0f per set bit -- plain vector stores, no read of the row.  Without best_id the row is never read.
#include "decode_row.h"

namespace fira {

constexpr int PHR_MAX = 8;                      // phrases per commit
constexpr int PHR_LEN = 4;                      // words per phrase
constexpr int PHR_EOS = 1;                      // config.EOS

__global__ __launch_bounds__(DDW_NT) void ban_phrases_dist_kernel(int T, int V, int L, int S, int rows_per_commit,
                                                                  const int32_t* __restrict__ gen,
                                                                  const int32_t* __restrict__ length,
                                                                  const int32_t* __restrict__ sou,
                                                                  const int32_t* __restrict__ sub,
                                                                  const int32_t* __restrict__ phrase,
                                                                  const int32_t* __restrict__ phrase_len,
                                                                  const int32_t* __restrict__ n_phrases,
                                                                  float* __restrict__ dist, int32_t* __restrict__ best_id,
                                                                  float* __restrict__ best_p) {
    __shared__ uint32_t s_bm[bitmap_words(ROW_MAX_V + ROW_MAX_SLOTS)];
    __shared__ int32_t s_blk[PHR_MAX];
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
        const int q = lane & (PHR_MAX - 1);
        const size_t pq = b * PHR_MAX + q;
        int w[PHR_LEN];
#pragma unroll
        for (int u = 0; u < PHR_LEN; ++u) w[u] = phrase[pq * PHR_LEN + u];
        const int l = phrase_len[pq];
        const int n = min(max(n_phrases[b], 0), PHR_MAX);
        const int len = min(max(length[r], 1), T);
        const int m = len - 1;                             // words after <start>
        const int h = gen[(size_t)r * T + min(lane, T - 1)];
        const bool finished = __shfl(h, m, 64) == PHR_EOS;
        // t_k: the k-th word from the end, position m + 1 - k (looked at only where k <= l - 1 <= m: a word, never <start>)
        const int t1 = __shfl(h, max(m, 0), 64), t2 = __shfl(h, max(m - 1, 0), 64), t3 = __shfl(h, max(m - 2, 0), 64);
        bool hit = !finished && lane < n && l >= 2 && l <= PHR_LEN && m >= l - 1;
        // (w_{l-1}, w_{l-2}, w_{l-3}) against (t_1, t_2, t_3)
        const int a1 = l == 2 ? w[0] : l == 3 ? w[1] : w[2];
        const int a2 = l == 3 ? w[0] : w[1];
        hit = hit && a1 == t1 && (l < 3 || a2 == t2) && (l < 4 || w[0] == t3);
        const int last = l == 2 ? w[1] : l == 3 ? w[2] : w[3];
        const uint64_t hit_m = __ballot(hit);
        if (hit) s_blk[__builtin_popcountll(hit_m & ((1ull << lane) - 1ull))] = last;
        if (lane == 0) s_nblk = __builtin_popcountll(hit_m);
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

extern "C" int fira_ban_phrases_dist(void* stream, const fira_dims* d, int R, int rows_per_commit, const int32_t* gen,
                                     const int32_t* length, const int32_t* sou, const int32_t* sub_token, const int32_t* phrase,
                                     const int32_t* phrase_len, const int32_t* n_phrases, float* dist, int32_t* best_id,
                                     float* best_p) {
    using namespace fira;
    if (int e = require_row_geometry(d, rows_per_commit, R, best_id, best_p, "fira_ban_phrases_dist")) return e;
    FIRA_REQUIRE(d->tar_len >= 2 && d->tar_len <= ROW_MAX_T, "fira_ban_phrases_dist: tar_len = %d outside 2..%d (one lane per position)",
                 d->tar_len, ROW_MAX_T);
    if (R == 0) return 0;
    FIRA_REQUIRE(gen && length && sou && sub_token && dist, "fira_ban_phrases_dist: null pointer (gen, length, sou, sub_token or dist)");
    FIRA_REQUIRE(phrase && phrase_len && n_phrases, "fira_ban_phrases_dist: null pointer (phrase, phrase_len or n_phrases)");
    hipLaunchKernelGGL(ban_phrases_dist_kernel, dim3(R), dim3(DDW_NT), 0, (hipStream_t)stream, d->tar_len, d->vocab, d->sou_len,
                       d->sub_len, rows_per_commit, gen, length, sou, sub_token, phrase, phrase_len, n_phrases, dist, best_id,
                       best_p);
    FIRA_CHECK_LAUNCH("fira_ban_phrases_dist");
    return 0;
}
