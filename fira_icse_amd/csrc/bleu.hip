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
#include "common.h"

namespace fira {

constexpr int BLEU_CPW = 4;            // commits (= waves) per workgroup
constexpr int BLEU_T = 64;             // positions a wave covers
constexpr int BLEU_PAD = 0, BLEU_EOS = 1, BLEU_UNK = 3;      // config.PAD / EOS / UNK
constexpr int BLEU_UNK_CMP = -2;       // what a hypothesis <unkm> is compared as: no vocabulary id, not the -1 fill of hyp

__device__ __forceinline__ int wave_sum_i32(int v) {
    v += __builtin_amdgcn_update_dpp(v, v, DPP_XOR1, 0xf, 0xf, false);
    v += __builtin_amdgcn_update_dpp(v, v, DPP_XOR2, 0xf, 0xf, false);
    v += __builtin_amdgcn_update_dpp(v, v, DPP_HALF_MIRROR, 0xf, 0xf, false);
    v += __builtin_amdgcn_update_dpp(v, v, DPP_MIRROR, 0xf, 0xf, false);
    v += __builtin_amdgcn_update_dpp(0, v, DPP_BCAST15, 0xa, 0xf, false);      // rows 1, 3 += lane 15 of the row before
    v += __builtin_amdgcn_update_dpp(0, v, DPP_BCAST31, 0xc, 0xf, false);      // rows 2, 3 += lane 31
    return __builtin_amdgcn_readlane(v, 63);
}

__device__ __forceinline__ uint64_t low_bits(int n) { return n >= 64 ? ~0ull : (1ull << n) - 1ull; }      // n in [0, 64]
__device__ __forceinline__ int clampi(int x, int lo, int hi) { return x < lo ? lo : (x > hi ? hi : x); }

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
    const int tc = in_t ? lane : T - 1;

    // ---- 1. requests (all unconditional, indices clamped), then the selects
    const int raw = ids[b * T + tc];
    const int tv = tar[b * T + tc];
    const int rc = clampi(raw, 0, V + L + S - 1);
    int from_sou = sou[b * L + clampi(rc - V, 0, L - 1)];
    int from_sub = sub[b * S + clampi(rc - V - L, 0, S - 1)];
    // (the compiler otherwise sinks each of the two loads under the test of its select: a divergent branch with a full vmcnt
    //  wait inside; both requests are in flight together this way)
    asm volatile("" : "+v"(from_sou), "+v"(from_sub));
    const int tok = raw >= V + L ? from_sub : (raw >= V ? from_sou : raw);

    const uint64_t below = low_bits(lane);
    const uint64_t eos_h = __ballot(in_t && raw == BLEU_EOS);
    const int n_raw = eos_h ? __builtin_ctzll(eos_h) : T;              // raw positions ahead of the first raw <eos>
    const bool keep = lane < n_raw && tok != BLEU_PAD;
    const uint64_t keep_m = __ballot(keep);
    const int hyp_len = __builtin_popcountll(keep_m);
    const int pos = __builtin_popcountll(keep_m & below);

    const uint64_t eos_r = __ballot(in_t && tv == BLEU_EOS);
    const int e_ref = eos_r ? __builtin_ctzll(eos_r) : T;
    const int ref_len = e_ref > 0 ? e_ref - 1 : 0;

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
