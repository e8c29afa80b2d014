// Sentence-BLEU statistics of the dev pass, on token ids (reference run_model.py:138-177: dev() scores every valid commit with
// NLTK sentence_bleu, method 2).  Per commit the kernel does what the host loop does on strings:
//   hypothesis  the raw output row of fira_forward_dev up to (not including) its first raw id == <eos> (all T without one), every
//               id resolved as text.resolve_copy does (>= V + L: sub_token[id - V - L]; >= V: sou[id - V]; the index clamped, so
//               that an id outside [0, V + L + S) cannot read out of range), every resolved <pad> dropped (the host's
//               replace("<pad>", "") + split()); a resolved <eos> / <start> stays a word, as on the host;
//   reference   tar[1 : first <eos> in tar] (a row without <eos> -- the host raises there -- counts to T);
//   <unkm>      the host writes the hypothesis' <unkm> as an emoji and leaves the reference's alone, so the two never match:
//               the hypothesis is COMPARED with a sentinel in its place and WRITTEN (hyp) with the real id;
//   counts      for n = 1..4: cnt = number of hypothesis n-grams, num = sum over the DISTINCT hypothesis n-grams of
//               min(count in the hypothesis, count in the reference).
// Everything is int32 and exact: no floats, no atomics, vector stores only.  The score itself (logs, the brevity penalty) is
// formed on the host from these twelve integers with the very expressions of metrics.sentence_bleu_method2.
//
// One wave per commit, BLEU_CPW commits per workgroup; T <= 64, so lane i owns hypothesis position i.
//   1. lane t requests ids[t], tar[t] (index clamped to T - 1, dropped by a select) and BOTH copy sources at clamped indices --
//      no load sits behind a divergent branch; ballots give the first <eos>, the kept lanes and their compacted positions.
//   2. the compacted hypothesis (real and compare form) and the reference go to LDS.
//   3. lane i builds two 64-bit masks: Eh[i] bit j = hyp[i] == hyp[j], Er[i] bit j = hyp[i] == ref[j] (64 + 64 LDS reads at a
//      wave-uniform address: broadcasts).  Bits at or past the lengths and the masks of lanes past hyp_len are 0.
//   4. the n-gram at i equals the n-gram at j iff bit j + k of E[i + k] is set for every k < n:
//          M_n[i] = M_{n-1}[i] & (E[i + n - 1] >> (n - 1))
//      (a shifted mask has no bit j with j + n - 1 past the length, which is exactly "position j starts an n-gram").  The masks
//      of the neighbouring lanes come through LDS.  Lane i contributes min(popc(Mh_n), popc(Mr_n)) if it starts an n-gram and
//      no lower position holds the same one (Mh_n has no bit below i); the wave sum is the integer form of common.h's DPP tree.
//
// What the hypothesis, the reference and a candidate's message ARE (steps 1 below) is message.h's, shared with rouge.hip.
#include "message.h"

namespace fira {

constexpr int BLEU_CPW = 4;            // commits (= waves) per workgroup

__device__ __forceinline__ int wave_sum_i32(int v) {
    v += __builtin_amdgcn_update_dpp(v, v, DPP_XOR1, 0xf, 0xf, false);
    v += __builtin_amdgcn_update_dpp(v, v, DPP_XOR2, 0xf, 0xf, false);
    v += __builtin_amdgcn_update_dpp(v, v, DPP_HALF_MIRROR, 0xf, 0xf, false);
    v += __builtin_amdgcn_update_dpp(v, v, DPP_MIRROR, 0xf, 0xf, false);
    v += __builtin_amdgcn_update_dpp(0, v, DPP_BCAST15, 0xa, 0xf, false);      // rows 1, 3 += lane 15 of the row before
    v += __builtin_amdgcn_update_dpp(0, v, DPP_BCAST31, 0xc, 0xf, false);      // rows 2, 3 += lane 31
    return __builtin_amdgcn_readlane(v, 63);
}

__global__ __launch_bounds__(BLEU_CPW * 64) void dev_bleu_stats_kernel(int B, int T, int V, int L, int S,
                                                                       const int32_t* __restrict__ ids,
                                                                       const int32_t* __restrict__ sou,
                                                                       const int32_t* __restrict__ sub,
                                                                       const int32_t* __restrict__ tar,
                                                                       int32_t* __restrict__ hyp, int32_t* __restrict__ stats) {
    __shared__ int32_t s_real[BLEU_CPW][BLEU_T];           // compacted hypothesis, real ids
    __shared__ int32_t s_cmp[BLEU_CPW][BLEU_T];            // compacted hypothesis, <unkm> as the sentinel
    __shared__ int32_t s_ref[BLEU_CPW][BLEU_T];
    __shared__ uint64_t s_eh[BLEU_CPW][BLEU_T + 4];        // + 4: lane i reads entries i .. i + 3
    __shared__ uint64_t s_er[BLEU_CPW][BLEU_T + 4];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int b_raw = blockIdx.x * BLEU_CPW + w;
    const bool live = b_raw < B;                           // wave-uniform; a wave past B recomputes commit B - 1, stores nothing
    const size_t b = (size_t)(live ? b_raw : B - 1);
    const bool in_t = lane < T;

    // ---- 1. requests (all unconditional, indices clamped), then the selects: message.h
    const DevMessage m = dev_message(b, lane, T, V, L, S, ids, sou, sub, tar);
    const int tok = m.tok, tv = m.tv, hyp_len = m.hyp_len, pos = m.pos, e_ref = m.e_ref, ref_len = m.ref_len;
    const bool keep = m.keep;
    const uint64_t below = low_bits(lane);

    // ---- 2. compacted hypothesis and reference into LDS
    if (keep) {
        s_real[w][pos] = tok;
        s_cmp[w][pos] = tok == BLEU_UNK ? BLEU_UNK_CMP : tok;
    }
    if (lane >= 1 && lane < e_ref) s_ref[w][lane - 1] = tv;
    if (lane < 4) { s_eh[w][BLEU_T + lane] = 0; s_er[w][BLEU_T + lane] = 0; }
    __syncthreads();

    const bool in_h = lane < hyp_len;
    const int cmp_l = s_cmp[w][lane], real_l = s_real[w][lane];       // (entries at or past hyp_len were never written:
    const int mine = in_h ? cmp_l : -1;                                //  dropped by the selects)
    const int real = in_h ? real_l : -1;
    if (live && in_t) hyp[b * T + lane] = real;

    // ---- 3. equality masks of position `lane` against every hypothesis / reference position
    uint64_t eh = 0, er = 0;
#pragma unroll 8
    for (int j = 0; j < BLEU_T; ++j) {
        eh |= (uint64_t)(s_cmp[w][j] == mine) << j;
        er |= (uint64_t)(s_ref[w][j] == mine) << j;
    }
    eh = in_h ? eh & low_bits(hyp_len) : 0;                // (also drops what unwritten LDS entries compared as)
    er = in_h ? er & low_bits(ref_len) : 0;
    s_eh[w][lane] = eh;
    s_er[w][lane] = er;
    __syncthreads();

    // ---- 4. n-gram masks, clipped counts, wave sums
    uint64_t mh = ~0ull, mr = ~0ull;
    int num[4], cnt[4];
#pragma unroll
    for (int n = 1; n <= 4; ++n) {
        mh &= s_eh[w][lane + n - 1] >> (n - 1);
        mr &= s_er[w][lane + n - 1] >> (n - 1);
        const bool starts = lane + n <= hyp_len;           // position `lane` starts an n-gram
        const bool first = (mh & below) == 0;              // ... and no lower position holds the same one
        const int ch = __builtin_popcountll(mh), cr = __builtin_popcountll(mr);
        num[n - 1] = wave_sum_i32(starts && first ? (ch < cr ? ch : cr) : 0);
        cnt[n - 1] = hyp_len >= n ? hyp_len - n + 1 : 0;
    }

    // ---- stats row: num[4], cnt[4], hyp_len, ref_len, 0, 0 (lanes 0..11, one vector store each)
    int out = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        out = lane == k ? num[k] : out;
        out = lane == 4 + k ? cnt[k] : out;
    }
    out = lane == 8 ? hyp_len : out;
    out = lane == 9 ? ref_len : out;
    if (live && lane < 12) stats[b * 12 + lane] = out;
}

// ---------------------------------------------------------------- all pairs of one commit's candidates (MBR selection)
// fira_mbr_bleu_stats: the statistics above for every ordered pair (hypothesis i, reference j) of the n candidate messages of a
// commit.  The message of a candidate is its row's ids at positions 1 .. min(length, T) - 1 with every <pad> / <eos> / <start>
// dropped wherever it stands (text.detokenize's string replacement); <unkm> is an ordinary word (both sides print the same
// emoji).  One workgroup of MBR_WAVES waves per commit:
//   1. wave w compacts candidates w, w + MBR_WAVES, ... into LDS (one row load and one length load per candidate, indices
//      clamped, nothing behind a branch; a ballot gives the kept lanes and their positions).  One barrier.
//   2. wave w owns hypotheses w, w + MBR_WAVES, ...: per hypothesis it builds Eh, the three neighbour masks (wave shuffles; no
//      LDS round trip, so no barrier inside the loops), the first-occurrence flags and popc(Mh_n) ONCE, then per reference j
//      only Er (64 LDS reads at a wave-uniform address) and Mr_n, four wave sums, and one 12-lane store.
// A reference is read from LDS, not from HBM n times.  Lengths, not sentinels, bound every mask, so any int32 is a word.
constexpr int MBR_WAVES = 4;

__device__ __forceinline__ uint64_t shfl_up_mask(uint64_t m, int lane, int k) {      // m of lane + k, >> k; 0 past the wave
    const int lo = __shfl((int)(uint32_t)m, lane + k), hi = __shfl((int)(uint32_t)(m >> 32), lane + k);
    const uint64_t v = ((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo;
    return lane + k < 64 ? v >> k : 0;
}

__device__ __forceinline__ uint64_t equal_mask(const int32_t* __restrict__ row, int mine) {      // bit t = row[t] == mine
    uint32_t lo = 0, hi = 0;
#pragma unroll
    for (int t = 0; t < 32; ++t) {
        lo |= (uint32_t)(row[t] == mine) << t;
        hi |= (uint32_t)(row[32 + t] == mine) << t;
    }
    return ((uint64_t)hi << 32) | lo;
}

__global__ __launch_bounds__(MBR_WAVES * 64) void mbr_bleu_stats_kernel(int n, int T, const int32_t* __restrict__ tokens,
                                                                        const int32_t* __restrict__ length,
                                                                        int32_t* __restrict__ stats) {
    __shared__ __attribute__((aligned(16))) int32_t s_tok[MBR_N][BLEU_T];      // compacted messages (entries past s_len: unwritten)
    __shared__ int32_t s_len[MBR_N];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const size_t row0 = (size_t)blockIdx.x * n;                                // first candidate row of this commit
    const uint64_t below = low_bits(lane);

    // ---- 1. compact the commit's candidates into LDS (message.h)
    for (int c = w; c < n; c += MBR_WAVES) {                                   // (wave-uniform trip count)
        const CandMessage m = cand_message(row0 + c, lane, T, tokens, length);
        if (m.keep) s_tok[c][m.pos] = m.tok;
        if (lane == 0) s_len[c] = m.len;
    }
    __syncthreads();

    // ---- 2. every hypothesis of this wave against every candidate
    for (int i = w; i < n; i += MBR_WAVES) {
        const int hyp_len = s_len[i];
        const bool in_h = lane < hyp_len;
        const int tok_l = s_tok[i][lane];                                      // (unwritten past hyp_len: dropped by the select
        const int mine = in_h ? tok_l : -1;                                    //  and by in_h on the masks)
        const uint64_t eh = in_h ? equal_mask(s_tok[i], mine) & low_bits(hyp_len) : 0;
        uint64_t mh = ~0ull;
        int ch[4], cnt[4];
        bool take[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            mh &= k == 0 ? eh : shfl_up_mask(eh, lane, k);
            ch[k] = __builtin_popcountll(mh);
            take[k] = lane + k + 1 <= hyp_len && (mh & below) == 0;            // starts a (k+1)-gram, first occurrence of it
            cnt[k] = hyp_len > k ? hyp_len - k : 0;
        }
        for (int j = 0; j < n; ++j) {
            const int ref_len = s_len[j];
            const uint64_t er = in_h ? equal_mask(s_tok[j], mine) & low_bits(ref_len) : 0;
            uint64_t mr = ~0ull;
            int out = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                mr &= k == 0 ? er : shfl_up_mask(er, lane, k);
                const int cr = __builtin_popcountll(mr);
                const int num = wave_sum_i32(take[k] ? (ch[k] < cr ? ch[k] : cr) : 0);
                out = lane == k ? num : out;
                out = lane == 4 + k ? cnt[k] : out;
            }
            out = lane == 8 ? hyp_len : out;
            out = lane == 9 ? ref_len : out;
            if (lane < 12) stats[((row0 + i) * n + j) * 12 + lane] = out;
        }
    }
}

}  // namespace fira

extern "C" int fira_dev_bleu_stats(void* stream, int B, int T, int V, int L, int S, const int32_t* ids, const int32_t* sou,
                                   const int32_t* sub_token, const int32_t* tar, int32_t* hyp, int32_t* stats) {
    using namespace fira;
    FIRA_REQUIRE(B >= 0, "fira_dev_bleu_stats: B = %d is negative", B);
    FIRA_REQUIRE(T >= 1 && T <= BLEU_T, "fira_dev_bleu_stats: T = %d outside 1..%d (one lane per position)", T, BLEU_T);
    FIRA_REQUIRE(V > BLEU_UNK && L >= 1 && S >= 1, "fira_dev_bleu_stats: V = %d, L = %d, S = %d (need V >= 4, L >= 1, S >= 1)",
                 V, L, S);
    FIRA_REQUIRE((int64_t)V + L + S <= 0x7fffffff, "fira_dev_bleu_stats: V + L + S overflows int32");
    if (B == 0) return 0;
    FIRA_REQUIRE(ids && sou && sub_token && tar && hyp && stats, "fira_dev_bleu_stats: null pointer");
    hipLaunchKernelGGL(dev_bleu_stats_kernel, dim3(cdiv(B, BLEU_CPW)), dim3(BLEU_CPW * 64), 0, (hipStream_t)stream, B, T, V, L, S,
                       ids, sou, sub_token, tar, hyp, stats);
    FIRA_CHECK_LAUNCH("fira_dev_bleu_stats");
    return 0;
}

extern "C" int fira_mbr_bleu_stats(void* stream, int B, int n, int T, const int32_t* tokens, const int32_t* length,
                                   int32_t* stats) {
    using namespace fira;
    FIRA_REQUIRE(B >= 0, "fira_mbr_bleu_stats: B = %d is negative", B);
    FIRA_REQUIRE(n >= 1 && n <= MBR_N, "fira_mbr_bleu_stats: n = %d outside 1..%d (candidates per commit)", n, MBR_N);
    FIRA_REQUIRE(T >= 1 && T <= BLEU_T, "fira_mbr_bleu_stats: T = %d outside 1..%d (one lane per position)", T, BLEU_T);
    if (B == 0) return 0;
    FIRA_REQUIRE(tokens && length && stats, "fira_mbr_bleu_stats: null pointer (tokens, length or stats)");
    hipLaunchKernelGGL(mbr_bleu_stats_kernel, dim3(B), dim3(MBR_WAVES * 64), 0, (hipStream_t)stream, n, T, tokens, length, stats);
    FIRA_CHECK_LAUNCH("fira_mbr_bleu_stats");
    return 0;
}
