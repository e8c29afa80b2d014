// A template on the decode step's output distribution: a deterministic automaton over word classes says which words may come next.
//
// fira_template_dist edits dist [R, W] (W = V + L + S: generator ids, diff positions, sub-token positions) in place, a link of
// the edit chain after fira_ban_phrases_dist and before fira_penalise_dist, with phrase.hip's geometry and definitions (DESIGN.md
// section 6zc).  Row r of commit b = r / rows_per_commit holds the hypothesis gen[r, 0 .. len), len = clamp(length[r], 1, T),
// m = len - 1 words h_1 .. h_m after <start>; a row whose last id is <eos> is finished and is not touched.  The tables:
//     word_class[V]   the class (0 .. 31, the low five bits are used) of every vocabulary id; an id outside [0, V), in the
//                     hypothesis or in a copy slot, has class 0
//     next[32 * 32]   next[s * 32 + c]: the state after a word of class c in state s, or -1 for "no such word here"
//     need[32]        the fewest words from state s to an accepting state (0: s accepts)
//     start[B]        the start state of every commit (outside 0 .. 31: no state at all, as -1)
// For an unfinished row: s = start[b], then s = next[s][class(h_p)] for p = 1 .. m (once -1 it stays -1), left = T - 1 - len.  The
// entries of the word w are blocked iff  s == -1,  or  w == <eos> and need[s] != 0,  or  w != <eos> and, with
// s' = next[s][class(w)], s' == -1 or need[s'] > left.  A blocked entry -- the generator id and every copy slot that carries the
// word -- becomes exactly 0.0f; every other element keeps its bits; nothing is renormalised.
//
// One workgroup of 1024 threads per row:
//   1. every thread requests the source id of "its" memory slot and, from it, that word's class (two dependent round trips, both
//      unconditional with clamped indices, in flight during the walk); thread t brings next[t] into LDS (1 KB, byte loads: the
//      table has any alignment), the first 32 bring need, and the bitmap of W bits is cleared.  Wave 0 reads the hypothesis with
//      lane p on position p (T <= 64) and gathers that word's class: one round trip for the whole hypothesis, before the walk.
//   2. wave 0 walks: m dependent LDS byte reads at a wave-uniform address (the class of position p comes by readlane).  This is
//      the kernel's only serial part.  Lane c < 32 then looks up next[s][c] and need of it: a ballot is the 32-bit mask of the
//      classes still allowed; with the <eos> verdict it goes to LDS.  s == -1 is "no class allowed, <eos> blocked"; a finished row
//      is "every class allowed, <eos> free".
//      A row with every class allowed and <eos> free has nothing to edit: without best_id the workgroup returns here.
//   3. the generator bits: a thread owns one bitmap word (V <= 25 600: 800 words), reads the 32 class bytes of its ids as nine
//      aligned dwords (indices clamped to the dwords the table overlaps, shifted by the table's misalignment: no byte outside the
//      table's own dwords is read, nothing is behind a branch), and sets the bit of every id below V whose class is not allowed;
//      the <eos> bit comes from the verdict.  The slot bits come from the slot's class (or the verdict, for a slot that carries
//      <eos>).  LDS atomics, since the last generator word also holds the first slots.
//   4. with best_id / best_p: one stream_row_marked pass that takes a set bit as the value 0, into an ArgMax.
//   5. the stores: one 0.0f per set bit -- plain vector stores, no read of the row.  Without best_id the row is never read.
#include "decode_row.h"

namespace fira {

constexpr int TPL_N = 32;                       // states and classes at most; the pitch of next
constexpr int TPL_EOS = 1;                      // config.EOS

__global__ __launch_bounds__(DDW_NT) void template_dist_kernel(int T, int V, int L, int S, int rows_per_commit,
                                                               const int32_t* __restrict__ gen,
                                                               const int32_t* __restrict__ length,
                                                               const int32_t* __restrict__ sou,
                                                               const int32_t* __restrict__ sub,
                                                               const uint8_t* __restrict__ word_class,
                                                               const int8_t* __restrict__ next,
                                                               const int32_t* __restrict__ need,
                                                               const int32_t* __restrict__ start, float* __restrict__ dist,
                                                               int32_t* __restrict__ best_id, float* __restrict__ best_p) {
    __shared__ uint32_t s_bm[bitmap_words(ROW_MAX_V + ROW_MAX_SLOTS)];
    __shared__ int8_t s_next[TPL_N * TPL_N];
    __shared__ int32_t s_need[TPL_N];
    __shared__ uint32_t s_allow;
    __shared__ int s_eos_blocked;
    __shared__ float smf[DDW_NT / 64];
    __shared__ int smi[DDW_NT / 64];
    const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const size_t b = (size_t)(r / rows_per_commit);
    const int W = V + L + S;
    const int n_words = (W + 31) / 32;

    // ---- 1. requests (unconditional, indices clamped); the tables into LDS; the bitmap cleared
    const int src = slot_word(sou, sub, b, L, S, tid);
    const int src_class = src >= 0 && src < V ? word_class[min(max(src, 0), V - 1)] & (TPL_N - 1) : 0;
    s_next[tid] = next[tid];                               // DDW_NT == TPL_N * TPL_N
    if (tid < TPL_N) s_need[tid] = need[tid];
    for (int w = tid; w <= n_words; w += DDW_NT) s_bm[w] = 0;
    int h = 0, cls = 0, len = 1, s = -1;
    if (tid < 64) {                                        // wave-uniform: all of wave 0
        len = min(max(length[r], 1), T);
        s = start[b];
        h = gen[(size_t)r * T + min(lane, T - 1)];
        cls = h >= 0 && h < V ? word_class[min(max(h, 0), V - 1)] & (TPL_N - 1) : 0;
    }
    __syncthreads();

    // ---- 2. the walk and the verdicts (wave 0)
    if (tid < 64) {
        const int m = len - 1;                             // words after <start>
        const bool finished = __shfl(h, m, 64) == TPL_EOS;
        s = __builtin_amdgcn_readfirstlane(s);
        if (s < 0 || s >= TPL_N) s = -1;
        for (int p = 1; p <= m && s >= 0; ++p) {           // wave-uniform: one dependent LDS read per word
            const int c = __builtin_amdgcn_readlane(cls, p);
            s = __builtin_amdgcn_readfirstlane((int)s_next[s * TPL_N + c]);
            if (s >= TPL_N) s = -1;
        }
        const int left = T - 1 - len;                      // positions that stay free after this step's word
        int sp = s >= 0 ? (int)s_next[s * TPL_N + (lane & (TPL_N - 1))] : -1;
        if (sp >= TPL_N) sp = -1;
        const bool ok = lane < TPL_N && sp >= 0 && s_need[max(sp, 0)] <= left;
        const uint64_t allow = __ballot(ok);
        if (lane == 0) {
            s_allow = finished ? 0xFFFFFFFFu : (uint32_t)allow;
            s_eos_blocked = finished ? 0 : (s < 0 || s_need[max(s, 0)] != 0);
        }
    }
    __syncthreads();
    const uint32_t allow = s_allow;
    const int eos_blocked = s_eos_blocked;
    const bool edits = allow != 0xFFFFFFFFu || eos_blocked;
    if (!edits && !best_id) return;                        // (workgroup-uniform) nothing to edit, nothing to report

    // ---- 3. mark: a thread's own generator word from 32 class bytes; the slot bits from the slot's class
    if (edits) {
        const int n_gen_words = (V + 31) / 32;
        const uintptr_t base = (uintptr_t)word_class;
        const unsigned mis = (unsigned)(base & 3u);
        const uint32_t* wc4 = reinterpret_cast<const uint32_t*>(base - mis);
        const int last_dw = (int)((mis + (unsigned)V - 1u) >> 2);      // the last dword the table overlaps
        for (int w = tid; w < n_gen_words; w += DDW_NT) {
            uint32_t d[9];
#pragma unroll
            for (int k = 0; k < 9; ++k) d[k] = wc4[min(8 * w + k, last_dw)];
            uint32_t bits = 0;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const uint32_t four = (uint32_t)(((((uint64_t)d[k + 1]) << 32) | d[k]) >> (8 * mis));
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const unsigned c = (four >> (8 * u)) & (TPL_N - 1);
                    bits |= (((allow >> c) & 1u) ^ 1u) << (4 * k + u);
                }
            }
            const int ids = V - 32 * w;                    // ids of this word below V: the bits above are not the table's
            if (ids < 32) bits &= (1u << ids) - 1u;
            if (w == 0) bits = (bits & ~(1u << TPL_EOS)) | ((uint32_t)eos_blocked << TPL_EOS);
            if (bits) atomicOr(&s_bm[w], bits);
        }
        if (tid < L + S) {
            const bool blocked = src == TPL_EOS ? eos_blocked != 0 : !((allow >> src_class) & 1u);
            if (blocked) atomicOr(&s_bm[(V + tid) >> 5], 1u << ((V + tid) & 31));
        }
        __syncthreads();
    }

    float* row = dist + (size_t)r * W;
    // ---- 4. arg-max of the edited row
    if (best_id) {
        ArgMax best;
        stream_row_marked(row, W, tid, s_bm, [&](float v, int i, unsigned blocked) { best.offer(blocked ? 0.0f : v, i); });
        best.reduce(smf, smi);
        best.report(best_id, best_p, r);
    }

    // ---- 5. the stores: one 0.0f per set bit (bits exist only below W)
    if (edits)
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

extern "C" int fira_template_dist(void* stream, const fira_dims* d, int R, int rows_per_commit, const int32_t* gen,
                                  const int32_t* length, const int32_t* sou, const int32_t* sub_token, const uint8_t* word_class,
                                  const int8_t* next, const int32_t* need, const int32_t* start, float* dist, int32_t* best_id,
                                  float* best_p) {
    using namespace fira;
    static_assert(DDW_NT == TPL_N * TPL_N, "thread t brings next[t] into LDS");
    if (int e = require_row_geometry(d, rows_per_commit, R, best_id, best_p, "fira_template_dist")) return e;
    FIRA_REQUIRE(d->tar_len >= 2 && d->tar_len <= ROW_MAX_T, "fira_template_dist: tar_len = %d outside 2..%d (one lane per position)",
                 d->tar_len, ROW_MAX_T);
    if (R == 0) return 0;
    FIRA_REQUIRE(gen && length && sou && sub_token && dist, "fira_template_dist: null pointer (gen, length, sou, sub_token or dist)");
    FIRA_REQUIRE(word_class && next && need && start, "fira_template_dist: null pointer (word_class, next, need or start)");
    hipLaunchKernelGGL(template_dist_kernel, dim3(R), dim3(DDW_NT), 0, (hipStream_t)stream, d->tar_len, d->vocab, d->sou_len,
                       d->sub_len, rows_per_commit, gen, length, sou, sub_token, word_class, next, need, start, dist, best_id,
                       best_p);
    FIRA_CHECK_LAUNCH("fira_template_dist");
    return 0;
}
