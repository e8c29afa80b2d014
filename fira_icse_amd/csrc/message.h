// The messages the text-metric kernels score (bleu.hip: sentence-BLEU statistics, rouge.hip: ROUGE-L statistics), one lane per
// position of a row of T <= 64 ids.  One definition of "which ids are the words of this row, and where do they go once the rest
// is dropped", so that the two metrics cannot drift apart on it:
//   dev_message   hypothesis and reference of a commit of the dev pass (bleu.hip has the rule and where it comes from);
//   cand_message  the message of one sampled candidate (MBR selection).
// Both only LOAD and ballot; the caller stores the kept ids where it wants them (LDS), at the compacted position `pos`.
#pragma once
#include "common.h"

namespace fira {

constexpr int BLEU_T = 64;             // positions a wave covers
constexpr int BLEU_PAD = 0, BLEU_EOS = 1, BLEU_START = 2, BLEU_UNK = 3;      // config.PAD / EOS / START / UNK
constexpr int BLEU_UNK_CMP = -2;       // what a hypothesis <unkm> is compared as: no vocabulary id, not the -1 fill of hyp
constexpr int MBR_N = 32;              // candidates per commit the LDS stage of an all-pairs kernel holds

__device__ __forceinline__ uint64_t low_bits(int n) { return n >= 64 ? ~0ull : (1ull << n) - 1ull; }      // n in [0, 64]
__device__ __forceinline__ int clampi(int x, int lo, int hi) { return x < lo ? lo : (x > hi ? hi : x); }

struct DevMessage {
    int tok;           // this lane's resolved hypothesis id (meaningful where keep)
    bool keep;         // the lane holds a hypothesis word
    int pos;           // ... which goes to this compacted position
    int hyp_len;
    int tv;            // this lane's target id: reference word lane - 1 where 1 <= lane < e_ref
    int e_ref;         // position of the first <eos> of the target (T without one)
    int ref_len;
};

// Commit b of the dev pass.  All requests unconditional, indices clamped, then the selects: no load sits behind a divergent
// branch; ballots give the first <eos>, the kept lanes and their compacted positions.
__device__ __forceinline__ DevMessage dev_message(size_t b, int lane, int T, int V, int L, int S, const int32_t* __restrict__ ids,
                                                  const int32_t* __restrict__ sou, const int32_t* __restrict__ sub,
                                                  const int32_t* __restrict__ tar) {
    DevMessage m;
    const bool in_t = lane < T;
    const int tc = in_t ? lane : T - 1;
    const int raw = ids[b * T + tc];
    m.tv = tar[b * T + tc];
    const int rc = clampi(raw, 0, V + L + S - 1);
    int from_sou = sou[b * L + clampi(rc - V, 0, L - 1)];
    int from_sub = sub[b * S + clampi(rc - V - L, 0, S - 1)];
    // (the compiler otherwise sinks each of the two loads under the test of its select: a divergent branch with a full vmcnt
    //  wait inside; both requests are in flight together this way)
    asm volatile("" : "+v"(from_sou), "+v"(from_sub));
    m.tok = raw >= V + L ? from_sub : (raw >= V ? from_sou : raw);

    const uint64_t eos_h = __ballot(in_t && raw == BLEU_EOS);
    const int n_raw = eos_h ? __builtin_ctzll(eos_h) : T;              // raw positions ahead of the first raw <eos>
    m.keep = lane < n_raw && m.tok != BLEU_PAD;
    const uint64_t keep_m = __ballot(m.keep);
    m.hyp_len = __builtin_popcountll(keep_m);
    m.pos = __builtin_popcountll(keep_m & low_bits(lane));

    const uint64_t eos_r = __ballot(in_t && m.tv == BLEU_EOS);
    m.e_ref = eos_r ? __builtin_ctzll(eos_r) : T;
    m.ref_len = m.e_ref > 0 ? m.e_ref - 1 : 0;
    return m;
}

struct CandMessage {
    int tok;
    bool keep;
    int pos;
    int len;           // words of the message
};

// One candidate row: ids at positions 1 .. min(length, T) - 1 with every <pad> / <eos> / <start> dropped wherever it stands
// (text.detokenize's string replacement).  One row load and one length load, indices clamped, nothing behind a branch.
__device__ __forceinline__ CandMessage cand_message(size_t row, int lane, int T, const int32_t* __restrict__ tokens,
                                                    const int32_t* __restrict__ length) {
    CandMessage m;
    const int tc = lane < T ? lane : T - 1;
    m.tok = tokens[row * T + tc];
    const int len = clampi(length[row], 0, T);
    m.keep = lane >= 1 && lane < len && m.tok != BLEU_PAD && m.tok != BLEU_EOS && m.tok != BLEU_START;
    const uint64_t keep_m = __ballot(m.keep);
    m.pos = __builtin_popcountll(keep_m & low_bits(lane));
    m.len = __builtin_popcountll(keep_m);
    return m;
}

}  // namespace fira
