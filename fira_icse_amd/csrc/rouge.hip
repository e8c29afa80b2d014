// ROUGE-L statistics on token ids: the length of the longest common subsequence (LCS) of a hypothesis and a reference, and the
// two lengths.  The score itself (Lin's sentence-level F-measure, beta = 1: 2 lcs / (hyp_len + ref_len)) is formed on the host by
// metrics.rouge_l_from_stats.  Which ids are the words of a message is message.h's, shared with bleu.hip: the hypothesis and
// reference of a commit are fira_dev_bleu_stats's (a hypothesis <unkm> matches nothing), a candidate's message is
// fira_mbr_bleu_stats's.  Everything is int32 and exact: no floats, no atomics, vector stores only.
//
// The LCS is the bit-vector recurrence of Allison & Dix / Hyyro.  With the positions of one message `a` as the bits of a 64-bit
// word X, all ones at the start, for every word c of the other message `b` in order:
//       U = X & M[c]                 M[c]: the positions of a that hold c
//       X = (X + U) | (X - U)        64-bit arithmetic, the carry out of bit 63 dropped
//   lcs = |a| - popcount(X & low_bits(|a|)).
// A zero bit of X at position p says "the LCS of a[0..p] and the words of b so far is one longer than that of a[0..p-1]".  Both
// the carries of X + U and the borrows of X - U run from low bits to high bits only, so the bits below |a| never depend on the
// bits at or above it -- what lanes past |a| ballot, and the carry that leaves bit 63 when |a| = 64, cannot reach the count.
//
// Mapping: a wave per pair, one lane per position of a (T <= 64 = the wave).  a[lane] stays in a VGPR for all of its pairs;
// b[lane] is one VGPR too, word t of it is a v_readlane at a wave-uniform index, and M[c] is ONE compare + ballot into an SGPR
// pair.  X, U, the add, the subtract and the or are scalar instructions on SGPR pairs: the recurrence costs no vector ALU beyond
// the compare, no LDS access and no DP table.  The LCS is symmetric, so the SHORTER message is the one that is walked.
#include "message.h"

namespace fira {

constexpr int ROUGE_CPW = 4;           // commits (= waves) per workgroup of the dev kernel
constexpr int ROUGE_WAVES = 4;         // waves per commit of the all-pairs kernel

// a_l: word `lane` of a (ANY value at lane >= a_len: those bits of M[c] are never masked off, by the argument above they cannot
// reach the count); b_l: word `lane` of b, the walked side (lanes >= b_len are never read).  Wave-uniform result.
__device__ __forceinline__ int lcs_wave(int a_l, int a_len, int b_l, int b_len) {
    uint64_t x = ~0ull;
    for (int t = 0; t < b_len; ++t) {                      // (wave-uniform trip count)
        const int c = __builtin_amdgcn_readlane(b_l, t);
        const uint64_t u = x & __builtin_amdgcn_ballot_w64(a_l == c);
        x = (x + u) | (x - u);
    }
    return a_len - __builtin_popcountll(x & low_bits(a_len));
}

// The same with the shorter message as the walked side (the lengths are wave-uniform: selects, one copy of the loop).
__device__ __forceinline__ int lcs_pair(int p_l, int p_len, int q_l, int q_len) {
    const bool walk_q = q_len <= p_len;
    return lcs_wave(walk_q ? p_l : q_l, walk_q ? p_len : q_len, walk_q ? q_l : p_l, walk_q ? q_len : p_len);
}

// ---------------------------------------------------------------- one commit of the dev pass per wave
__global__ __launch_bounds__(ROUGE_CPW * 64) void dev_rouge_l_stats_kernel(int B, int T, int V, int L, int S,
                                                                           const int32_t* __restrict__ ids,
                                                                           const int32_t* __restrict__ sou,
                                                                           const int32_t* __restrict__ sub,
                                                                           const int32_t* __restrict__ tar,
                                                                           int32_t* __restrict__ stats) {
    __shared__ int32_t s_cmp[ROUGE_CPW][BLEU_T];           // compacted hypothesis, <unkm> as the sentinel
    __shared__ int32_t s_ref[ROUGE_CPW][BLEU_T];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int b_raw = blockIdx.x * ROUGE_CPW + w;
    const bool live = b_raw < B;                           // wave-uniform; a wave past B recomputes commit B - 1, stores nothing
    const size_t b = (size_t)(live ? b_raw : B - 1);

    const DevMessage m = dev_message(b, lane, T, V, L, S, ids, sou, sub, tar);
    if (m.keep) s_cmp[w][m.pos] = m.tok == BLEU_UNK ? BLEU_UNK_CMP : m.tok;
    if (lane >= 1 && lane < m.e_ref) s_ref[w][lane - 1] = m.tv;
    __syncthreads();
    const int hyp_l = s_cmp[w][lane], ref_l = s_ref[w][lane];          // (entries at or past the lengths were never written:
                                                                       //  lcs_wave is indifferent to them on either side)
    const int lcs = lcs_pair(hyp_l, m.hyp_len, ref_l, m.ref_len);
    int out = 0;
    out = lane == 0 ? lcs : out;
    out = lane == 1 ? m.hyp_len : out;
    out = lane == 2 ? m.ref_len : out;
    if (live && lane < 4) stats[b * 4 + lane] = out;
}

// ---------------------------------------------------------------- all pairs of one commit's candidates (MBR selection)
// One workgroup of ROUGE_WAVES waves per commit.  (1) as in mbr_bleu_stats_kernel: wave w compacts candidates w, w + 4, ... into
// LDS; one barrier.  (2) lcs is symmetric, so every unordered pair is computed once and stored into both rows, each with its own
// (hyp_len, ref_len) order: candidate i takes the partners j = i + d (mod n) for d = 1 .. n / 2 -- a round-robin schedule, the
// same number of pairs for every i; for even n the distance n / 2 reaches a pair from both ends, so only its lower end takes it.
// The diagonal needs no recurrence.  Lanes 0..3 store row [i][j], lanes 4..7 row [j][i]: one store instruction per pair.
__global__ __launch_bounds__(ROUGE_WAVES * 64) void mbr_rouge_l_stats_kernel(int n, int T, const int32_t* __restrict__ tokens,
                                                                             const int32_t* __restrict__ length,
                                                                             int32_t* __restrict__ stats) {
    __shared__ int32_t s_tok[MBR_N][BLEU_T];               // compacted messages (entries past s_len: unwritten)
    __shared__ int32_t s_len[MBR_N];
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const size_t row0 = (size_t)blockIdx.x * n;            // first candidate row of this commit

    for (int c = w; c < n; c += ROUGE_WAVES) {             // (wave-uniform trip count)
        const CandMessage m = cand_message(row0 + c, lane, T, tokens, length);
        if (m.keep) s_tok[c][m.pos] = m.tok;
        if (lane == 0) s_len[c] = m.len;
    }
    __syncthreads();

    const int k = lane & 3;                                // column of the stats row this lane stores
    for (int i = w; i < n; i += ROUGE_WAVES) {
        const int len_i = __builtin_amdgcn_readfirstlane(s_len[i]);     // (wave-uniform, and provably so)
        const int tok_i = s_tok[i][lane];
        if (lane < 4) {                                    // the diagonal: lcs == hyp_len == ref_len
            stats[((row0 + i) * n + i) * 4 + lane] = lane < 3 ? len_i : 0;
        }
        for (int d = 1; 2 * d <= n; ++d) {
            if (2 * d == n && i >= d) break;               // (wave-uniform) the pair at distance n / 2 belongs to its lower end
            const int j = i + d < n ? i + d : i + d - n;
            const int len_j = __builtin_amdgcn_readfirstlane(s_len[j]);
            const int tok_j = s_tok[j][lane];
            const int lcs = lcs_pair(tok_i, len_i, tok_j, len_j);
            const bool fwd = lane < 4;                     // lanes 0..3: row [i][j]; lanes 4..7: row [j][i]
            const int hyp = fwd ? i : j, ref = fwd ? j : i;
            int out = 0;
            out = k == 0 ? lcs : out;
            out = k == 1 ? (fwd ? len_i : len_j) : out;
            out = k == 2 ? (fwd ? len_j : len_i) : out;
            if (lane < 8) stats[((row0 + hyp) * n + ref) * 4 + k] = out;
        }
    }
}

}  // namespace fira

extern "C" int fira_dev_rouge_l_stats(void* stream, int B, int T, int V, int L, int S, const int32_t* ids, const int32_t* sou,
                                      const int32_t* sub_token, const int32_t* tar, int32_t* stats) {
    using namespace fira;
    FIRA_REQUIRE(B >= 0, "fira_dev_rouge_l_stats: B = %d is negative", B);
    FIRA_REQUIRE(T >= 1 && T <= BLEU_T, "fira_dev_rouge_l_stats: T = %d outside 1..%d (one lane per position)", T, BLEU_T);
    FIRA_REQUIRE(V > BLEU_UNK && L >= 1 && S >= 1, "fira_dev_rouge_l_stats: V = %d, L = %d, S = %d (need V >= 4, L >= 1, S >= 1)",
                 V, L, S);
    FIRA_REQUIRE((int64_t)V + L + S <= 0x7fffffff, "fira_dev_rouge_l_stats: V + L + S overflows int32");
    if (B == 0) return 0;
    FIRA_REQUIRE(ids && sou && sub_token && tar && stats, "fira_dev_rouge_l_stats: null pointer");
    hipLaunchKernelGGL(dev_rouge_l_stats_kernel, dim3(cdiv(B, ROUGE_CPW)), dim3(ROUGE_CPW * 64), 0, (hipStream_t)stream, B, T, V,
                       L, S, ids, sou, sub_token, tar, stats);
    FIRA_CHECK_LAUNCH("fira_dev_rouge_l_stats");
    return 0;
}

extern "C" int fira_mbr_rouge_l_stats(void* stream, int B, int n, int T, const int32_t* tokens, const int32_t* length,
                                      int32_t* stats) {
    using namespace fira;
    FIRA_REQUIRE(B >= 0, "fira_mbr_rouge_l_stats: B = %d is negative", B);
    FIRA_REQUIRE(n >= 1 && n <= MBR_N, "fira_mbr_rouge_l_stats: n = %d outside 1..%d (candidates per commit)", n, MBR_N);
    FIRA_REQUIRE(T >= 1 && T <= BLEU_T, "fira_mbr_rouge_l_stats: T = %d outside 1..%d (one lane per position)", T, BLEU_T);
    if (B == 0) return 0;
    FIRA_REQUIRE(tokens && length && stats, "fira_mbr_rouge_l_stats: null pointer (tokens, length or stats)");
    hipLaunchKernelGGL(mbr_rouge_l_stats_kernel, dim3(B), dim3(ROUGE_WAVES * 64), 0, (hipStream_t)stream, n, T, tokens, length,
                       stats);
    FIRA_CHECK_LAUNCH("fira_mbr_rouge_l_stats");
    return 0;
}
