// Per-commit word sets on the decode step's output distribution: allow, deny, boost and ground, each a vocabulary-sized bit set.
//
// fira_wordset_dist edits dist [R, W] (W = V + L + S: generator ids, diff positions, sub-token positions) in place, a link of
// the edit chain after fira_template_dist and before fira_penalise_dist, with fira_constrain_dist's geometry and definitions
// (DESIGN.md section 6zd).  Row r of commit b = r / rows_per_commit; len = clamp(length[r], 1, T); a row whose last id is <eos>
// is finished and is not touched.  The sets, each NULL ("not given") or [B, ceil(V / 32)] uint32, bit w % 32 of word w / 32 for
// id w, the bits at or past V ignored:
//     allow    only these words (and <eos>) may be written
//     deny     these words may not
//     ground   these words may be written only if a VALID copy slot of the commit carries them
//     boost    these words are multiplied by boost_factor[b]
// in(S, w): S is given, 0 <= w < V and the bit is set.  carried(b, w): some slot j of commit b with bit j of slot_valid[b] set has
// the source id w.  For an unfinished row the word w is blocked iff
//     allow is given and w != <eos> and !in(allow, w),   or   in(deny, w),   or   in(ground, w) and !carried(b, w)
// and every entry i with w(i) blocked -- the generator id and every copy slot that carries the word -- becomes exactly +0.0f;
// every entry that is not blocked with in(boost, w(i)) becomes fl32(dist[i] * boost_factor[b]), one multiplication, once; every
// other element keeps its bits; nothing is renormalised.  An id outside [0, V) is in no set: blocked under allow, otherwise
// left alone, never an index.
//
// One workgroup of 1024 threads per row:
//   1. every thread reads the row's state (length, last id: the same few addresses for the whole workgroup).  A finished row
//      ends here when no arg-max is asked for; with best_id it takes one stream_row_marked pass with clear marks.
//   2. every thread requests the source id of "its" slot (slot_word: L + S <= 1024) and the slot's valid bit; the two bitmaps of
//      W bits (blocked, boosted) and, with ground, the carried set of V bits are cleared.  The carried set is an LDS bit-or of
//      the valid slots' ids: no extra launch, no global buffer.
//   3. the generator bits: a thread owns one 32-id word (V <= 25 600: 800 words), reads that word of each given set -- four
//      coalesced dword loads -- and the carried word from LDS, and forms blocked and boosted for 32 ids at once.
//   4. the slot bits: a slot's verdict is its source id's generator bit (read from LDS, then a barrier, then LDS atomics: the last
//      generator word also holds the first slots); a source id outside [0, V) is blocked iff allow is given.
//   5. with best_id / best_p: one stream_row_marked pass that takes a blocked entry as 0 and a boosted entry as its product,
//      into an ArgMax -- before any store (the reduction's barriers lie between).
//   6. the boosted entries: read, one multiplication, a 4-byte store, by the thread that owns the bitmap word.
//   7. the zeros, cut at the row's 16-byte boundaries (RowSplit): a vector whose four bits are set is one 16-byte store; a vector
//      with a free entry, and the elements before the first and after the last boundary, take 4-byte stores.  No read.
// Without best_id an allowed and unboosted entry is neither read nor written: the row is stores of zeros plus the reads of the
// boosted entries.  Boosted and blocked entries are disjoint, and every entry has one owner: no two threads write one address.
#include "decode_row.h"

namespace fira {

constexpr int WST_EOS = 1;                      // config.EOS
constexpr int WST_GEN_WORDS = (ROW_MAX_V + 31) / 32;

__global__ __launch_bounds__(DDW_NT) void wordset_dist_kernel(int T, int V, int L, int S, int rows_per_commit,
                                                              const int32_t* __restrict__ gen,
                                                              const int32_t* __restrict__ length,
                                                              const int32_t* __restrict__ sou,
                                                              const int32_t* __restrict__ sub,
                                                              const uint32_t* __restrict__ allow,
                                                              const uint32_t* __restrict__ deny,
                                                              const uint32_t* __restrict__ boost,
                                                              const uint32_t* __restrict__ ground,
                                                              const uint32_t* __restrict__ slot_valid,
                                                              const float* __restrict__ boost_factor,
                                                              float* __restrict__ dist, int32_t* __restrict__ best_id,
                                                              float* __restrict__ best_p) {
    __shared__ uint32_t s_bm[bitmap_words(ROW_MAX_V + ROW_MAX_SLOTS)];     // blocked entries
    __shared__ uint32_t s_up[bitmap_words(ROW_MAX_V + ROW_MAX_SLOTS)];     // boosted entries
    __shared__ uint32_t s_car[WST_GEN_WORDS];                              // carried ids
    __shared__ float smf[DDW_NT / 64];
    __shared__ int smi[DDW_NT / 64];
    const int r = blockIdx.x, tid = threadIdx.x;
    const size_t b = (size_t)(r / rows_per_commit);
    const int NS = L + S, W = V + NS;
    const int n_words = (W + 31) / 32, n_gen = (V + 31) / 32, n_sv = (NS + 31) / 32;

    // ---- 1. the row's state (workgroup-uniform addresses and values)
    const int len = min(max(length[r], 1), T);
    const bool finished = gen[(size_t)r * T + (len - 1)] == WST_EOS;
    const bool zeroes = allow || deny || ground;
    const bool edits = !finished && (zeroes || boost);
    if (!edits && !best_id) return;                        // (workgroup-uniform) nothing to edit, nothing to report

    for (int w = tid; w <= n_words; w += DDW_NT) { s_bm[w] = 0; s_up[w] = 0; }
    float* row = dist + (size_t)r * W;
    if (!edits) {
        __syncthreads();
        ArgMax best;
        stream_row_marked(row, W, tid, s_bm, [&](float v, int i, unsigned) { best.offer(v, i); });
        best.reduce(smf, smi);
        best.report(best_id, best_p, r);
        return;
    }

    // ---- 2. requests (indices clamped); the carried set
    const int src = slot_word(sou, sub, b, L, S, tid);
    const bool src_in_v = src >= 0 && src < V;             // an id outside [0, V) is never used as an index
    const float fac = boost ? boost_factor[b] : 1.0f;
    if (ground) {                                          // (workgroup-uniform)
        const uint32_t sv = NS > 0 ? slot_valid[b * n_sv + min(tid >> 5, n_sv - 1)] : 0u;
        const bool valid = tid < NS && ((sv >> (tid & 31)) & 1u);
        for (int w = tid; w < n_gen; w += DDW_NT) s_car[w] = 0;
        __syncthreads();
        if (valid && src_in_v) atomicOr(&s_car[src >> 5], 1u << (src & 31));
    }
    __syncthreads();

    // ---- 3. the generator bits, 32 ids per thread
    for (int w = tid; w < n_gen; w += DDW_NT) {
        const size_t at = b * n_gen + w;
        const uint32_t a = allow ? allow[at] : 0xFFFFFFFFu;
        const uint32_t d = deny ? deny[at] : 0u;
        const uint32_t g = ground ? ground[at] & ~s_car[w] : 0u;
        const uint32_t u = boost ? boost[at] : 0u;
        const int ids = V - 32 * w;                        // ids of this word below V: the bits above are not the sets'
        const uint32_t live = ids < 32 ? (1u << ids) - 1u : 0xFFFFFFFFu;
        const uint32_t eos = w == 0 ? 1u << WST_EOS : 0u;  // <eos> is free of allow, not of deny and ground
        const uint32_t blk = ((~a & ~eos) | d | g) & live;
        const uint32_t up = u & ~blk & live;
        if (blk) atomicOr(&s_bm[w], blk);
        if (up) atomicOr(&s_up[w], up);
    }
    __syncthreads();

    // ---- 4. the slot bits: the verdict of the slot's source id
    bool s_blk = false, s_boost = false;
    if (tid < NS) {
        const int at = src_in_v ? src : 0;
        const uint32_t bw = s_bm[at >> 5], uw = s_up[at >> 5];
        s_blk = src_in_v ? (bw >> (at & 31)) & 1u : allow != nullptr;
        s_boost = src_in_v && ((uw >> (at & 31)) & 1u);
    }
    __syncthreads();
    if (s_blk) atomicOr(&s_bm[(V + tid) >> 5], 1u << ((V + tid) & 31));
    if (s_boost) atomicOr(&s_up[(V + tid) >> 5], 1u << ((V + tid) & 31));
    __syncthreads();

    // ---- 5. arg-max of the edited row, before any store
    if (best_id) {
        ArgMax best;
        stream_row_marked(row, W, tid, s_bm, [&](float v, int i, unsigned blocked) {
            const bool up = (s_up[i >> 5] >> (i & 31)) & 1u;
            const float vb = v * fac;
            best.offer(blocked ? 0.0f : (up ? vb : v), i);
        });
        best.reduce(smf, smi);                             // (its barriers order every read above before the stores below)
        best.report(best_id, best_p, r);
    }

    // ---- 6. the boosted entries: one multiplication each (bits exist only below W)
    if (boost)
        for (int w = tid; w < n_words; w += DDW_NT) {
            uint32_t bits = s_up[w];
            while (bits) {
                const int i = w * 32 + __builtin_ctz(bits);
                bits &= bits - 1;
                const float v = row[i];
                row[i] = v * fac;
            }
        }

    // ---- 7. the zeros: +0.0f wherever the blocked bit is set
    if (!zeroes) return;                                   // (workgroup-uniform)
    const RowSplit c(row, W);
    if (tid < c.head && ((s_bm[tid >> 5] >> (tid & 31)) & 1u)) row[tid] = 0.0f;
    if (tid >= DDW_NT - 4 && c.tail_of(tid) < W) {
        const int i = c.tail_of(tid);
        if ((s_bm[i >> 5] >> (i & 31)) & 1u) row[i] = 0.0f;
    }
    float4* rowv = reinterpret_cast<float4*>(row + c.head);
    for (int v = tid; v < c.nvec; v += DDW_NT) {
        const int i = c.head + 4 * v;
        const uint64_t two = ((uint64_t)s_bm[(i >> 5) + 1] << 32) | s_bm[i >> 5];
        const unsigned bits = (unsigned)(two >> (i & 31)) & 15u;
        if (bits == 15u) {
            rowv[v] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        } else if (bits) {                                 // around a free entry: 4-byte stores
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if ((bits >> u) & 1u) row[i + u] = 0.0f;
        }
    }
}

}  // namespace fira

extern "C" int fira_wordset_dist(void* stream, const fira_dims* d, int R, int rows_per_commit, const int32_t* gen,
                                 const int32_t* length, const int32_t* sou, const int32_t* sub_token, const uint32_t* allow,
                                 const uint32_t* deny, const uint32_t* boost, const uint32_t* ground, const uint32_t* slot_valid,
                                 const float* boost_factor, float* dist, int32_t* best_id, float* best_p) {
    using namespace fira;
    if (int e = require_row_geometry(d, rows_per_commit, R, best_id, best_p, "fira_wordset_dist")) return e;
    FIRA_REQUIRE(d->tar_len >= 2 && d->tar_len <= ROW_MAX_T, "fira_wordset_dist: tar_len = %d outside 2..%d", d->tar_len, ROW_MAX_T);
    if (R == 0) return 0;
    FIRA_REQUIRE(gen && length && sou && sub_token && dist, "fira_wordset_dist: null pointer (gen, length, sou, sub_token or dist)");
    FIRA_REQUIRE(!ground || slot_valid, "fira_wordset_dist: null pointer (slot_valid, which ground needs)");
    FIRA_REQUIRE(!boost || boost_factor, "fira_wordset_dist: null pointer (boost_factor, which boost needs)");
    hipLaunchKernelGGL(wordset_dist_kernel, dim3(R), dim3(DDW_NT), 0, (hipStream_t)stream, d->tar_len, d->vocab, d->sou_len,
                       d->sub_len, rows_per_commit, gen, length, sou, sub_token, allow, deny, boost, ground, slot_valid,
                       boost_factor, dist, best_id, best_p);
    FIRA_CHECK_LAUNCH("fira_wordset_dist");
    return 0;
}
