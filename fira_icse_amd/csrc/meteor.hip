// METEOR alignment statistics on token ids: the number of matched word pairs m of a hypothesis and a reference, the number of
// chunks (maximal runs of matches that are adjacent and in order on both sides) and the two lengths.  The score itself (NLTK's
// alpha = 0.9, beta = 3, gamma = 0.5) is formed on the host by metrics.meteor_exact_from_stats.  Which ids are the words of a
// message is message.h's, shared with bleu.hip and rouge.hip: the hypothesis and reference of a commit are fira_dev_bleu_stats's
// (a hypothesis <unkm> matches nothing), a candidate's message is fira_mbr_bleu_stats's.  Everything is int32 and exact: no
// floats, no atomics, vector stores only.
//
// The alignment is NLTK's _match_enums in two stages (the project ships no stemmer and no WordNet: stage 2 runs on a table the
// caller supplies, or not at all): stage 1 pairs words of equal id, stage 2 the words still free whose ids lie in [0, V) and have
// equal classes[id].  Within a stage the sequential rule -- hypothesis positions from the last to the first, each taking the last
// free reference position of equal key -- pairs, for every key, the k-th last free occurrence on one side with the k-th last on
// the other (DESIGN.md 6j-3 has the proof).  That description names neither side, so either message may be the one that is
// walked: walking b from its last position to its first, position j takes the HIGHEST free position of a with an equal key.
//
// Mapping: a wave per pair, one lane per position of a (T <= 64 = the wave).  The key of b[j] is a v_readlane at a wave-uniform
// index, "the positions of a that hold it" ONE compare + ballot into an SGPR pair, "still free" an and with a scalar mask, "the
// highest" a scalar find-first-bit from the top; lane i keeps j as its partner.  Chunks: one exchange of the partner with lane
// + 1; a match (i, j) continues a chunk into (i + 1, j + 1) iff partner[i + 1] == partner[i] + 1.  The SHORTER message is the one
// walked, the loop runs over its words, not over T.
#include "message.h"

namespace fira {

constexpr int METEOR_CPW = 4;          // commits (= waves) per workgroup of the dev kernel
constexpr int METEOR_WAVES = 4;        // waves per commit of the all-pairs kernel

struct MeteorSide {
    int id;            // word `lane` of the message (ANY value at lane >= len: those lanes are masked off or never read)
    int cls;           // classes[id] where has (stage 2 only)
    bool has;          // lane < len and id in [0, V): the word has a class
    int len;           // wave-uniform
};

// a word of class: in range, then the table (the index is clamped FIRST, the load is unconditional; V >= 4 where classes is given)
__device__ __forceinline__ void meteor_class(MeteorSide& s, int lane, int V, const int32_t* __restrict__ classes) {
    s.has = lane < s.len && s.id >= 0 && s.id < V;
    s.cls = classes[s.has ? s.id : 0];
}

// b[j] (free) looks for the highest free position of a with its key: one step of either stage.  All of it wave-uniform but the
// compare and the select of the partner.
__device__ __forceinline__ void meteor_step(int a_key, int b_key_j, int j, int lane, uint64_t& a_free, uint64_t& b_free,
                                            int& partner, int& m) {
    const uint64_t cand = __builtin_amdgcn_ballot_w64(a_key == b_key_j) & a_free;
    if (cand) {                                            // (wave-uniform)
        const int i = 63 - __builtin_clzll(cand);
        a_free &= ~(1ull << i);
        b_free &= ~(1ull << j);
        partner = lane == i ? j : partner;
        ++m;
    }
}

// (m, chunks) of the pair, wave-uniform; `a` holds the partners, `b` is walked.  classes == nullptr: stage 1 only.
__device__ __forceinline__ void meteor_wave(const MeteorSide& a, const MeteorSide& b, int lane, bool stage2, int& m, int& chunks) {
    uint64_t a_free = low_bits(a.len), b_free = low_bits(b.len);
    int partner = -1;                                      // position of b this lane's word of a is matched with
    m = 0;
    for (int j = b.len - 1; j >= 0; --j) {                 // (wave-uniform trip count)
        meteor_step(a.id, __builtin_amdgcn_readlane(b.id, j), j, lane, a_free, b_free, partner, m);
    }
    if (stage2) {                                          // (wave-uniform)
        a_free &= __builtin_amdgcn_ballot_w64(a.has);      // a word without a class is never a candidate ...
        uint64_t todo = b_free & __builtin_amdgcn_ballot_w64(b.has);       // ... and never looks for one
        while (todo && a_free) {
            const int j = 63 - __builtin_clzll(todo);
            todo &= ~(1ull << j);
            meteor_step(a.cls, __builtin_amdgcn_readlane(b.cls, j), j, lane, a_free, b_free, partner, m);
        }
    }
    // lane 63 reads its own partner p back: p == p + 1 never holds.  A free lane has -1, and a continuation needs >= 1.
    const int next = __shfl_down(partner, 1);
    const bool continues = partner >= 0 && next == partner + 1;
    chunks = m - __builtin_popcountll(__builtin_amdgcn_ballot_w64(continues));
}

// The same with the shorter message as the walked side (the lengths are wave-uniform: selects, one copy of the loops).
__device__ __forceinline__ void meteor_pair(const MeteorSide& p, const MeteorSide& q, int lane, bool stage2, int& m, int& chunks) {
    const bool walk_q = q.len <= p.len;
    MeteorSide a, b;
    a.id = walk_q ? p.id : q.id, a.cls = walk_q ? p.cls : q.cls, a.has = walk_q ? p.has : q.has, a.len = walk_q ? p.len : q.len;
    b.id = walk_q ? q.id : p.id, b.cls = walk_q ? q.cls : p.cls, b.has = walk_q ? q.has : p.has, b.len = walk_q ? q.len : p.len;
    meteor_wave(a, b, lane, stage2, m, chunks);
}

// ---------------------------------------------------------------- one commit of the dev pass per wave
__global__ __launch_bounds__(METEOR_CPW * 64) void dev_meteor_stats_kernel(int B, int T, int V, int L, int S,
                                                                           const int32_t* __restrict__ ids,
                                                                           const int32_t* __restrict__ sou,
                                                                           const int32_t* __restrict__ sub,
                                                                           const int32_t* __restrict__ tar,
                                                                           const int32_t* __restrict__ classes,
                                                                           int32_t* __restrict__ stats) {
    __shared__ int32_t s_cmp[METEOR_CPW][BLEU_T];          // compacted hypothesis, <unkm> as the sentinel (no id: no class)
    __shared__ int32_t s_ref[METEOR_CPW][BLEU_T];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int b_raw = blockIdx.x * METEOR_CPW + w;
    const bool live = b_raw < B;                           // wave-uniform; a wave past B recomputes commit B - 1, stores nothing
    const size_t b = (size_t)(live ? b_raw : B - 1);

    const DevMessage msg = dev_message(b, lane, T, V, L, S, ids, sou, sub, tar);
    if (msg.keep) s_cmp[w][msg.pos] = msg.tok == BLEU_UNK ? BLEU_UNK_CMP : msg.tok;
    if (lane >= 1 && lane < msg.e_ref) s_ref[w][lane - 1] = msg.tv;
    __syncthreads();
    MeteorSide hyp, ref;                                   // (entries at or past the lengths were never written: see MeteorSide)
    hyp.id = s_cmp[w][lane], hyp.len = msg.hyp_len, hyp.cls = 0, hyp.has = false;
    ref.id = s_ref[w][lane], ref.len = msg.ref_len, ref.cls = 0, ref.has = false;
    const bool stage2 = classes != nullptr;                // (a kernel argument: uniform)
    if (stage2) {
        meteor_class(hyp, lane, V, classes);
        meteor_class(ref, lane, V, classes);
    }
    int m, chunks;
    meteor_pair(hyp, ref, lane, stage2, m, chunks);
    int out = msg.ref_len;
    out = lane == 0 ? m : out;
    out = lane == 1 ? chunks : out;
    out = lane == 2 ? msg.hyp_len : out;
    if (live && lane < 4) stats[b * 4 + lane] = out;
}

// ---------------------------------------------------------------- all pairs of one commit's candidates (MBR selection)
// One workgroup of METEOR_WAVES waves per commit, laid out as mbr_rouge_l_stats_kernel: (1) wave w compacts candidates w, w + 4,
// ... into LDS, with their classes; one barrier.  (2) the pairs, m and chunks do not depend on which message is the hypothesis
// (DESIGN.md 6j-3), so every unordered pair is computed once and stored into both rows, each with its own (hyp_len, ref_len)
// order: candidate i takes the partners j = i + d (mod n) for d = 1 .. n / 2; for even n the distance n / 2 reaches a pair from
// both ends, so only its lower end takes it.  The diagonal needs no alignment: every word pairs with itself, one chunk.  Lanes
// 0..3 store row [i][j], lanes 4..7 row [j][i]: one store instruction per pair.
__global__ __launch_bounds__(METEOR_WAVES * 64) void mbr_meteor_stats_kernel(int n, int T, const int32_t* __restrict__ tokens,
                                                                             const int32_t* __restrict__ length, int V,
                                                                             const int32_t* __restrict__ classes,
                                                                             int32_t* __restrict__ stats) {
    __shared__ int32_t s_tok[MBR_N][BLEU_T];               // compacted messages (entries past s_len: unwritten)
    __shared__ int32_t s_cls[MBR_N][BLEU_T];               // their classes (stage 2 only; meaningful where the id is in [0, V))
    __shared__ int32_t s_len[MBR_N];
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const size_t row0 = (size_t)blockIdx.x * n;            // first candidate row of this commit
    const bool stage2 = classes != nullptr;

    for (int c = w; c < n; c += METEOR_WAVES) {            // (wave-uniform trip count)
        const CandMessage msg = cand_message(row0 + c, lane, T, tokens, length);
        if (msg.keep) s_tok[c][msg.pos] = msg.tok;
        if (stage2) {
            const int cls = classes[msg.keep && msg.tok >= 0 && msg.tok < V ? msg.tok : 0];
            if (msg.keep) s_cls[c][msg.pos] = cls;
        }
        if (lane == 0) s_len[c] = msg.len;
    }
    __syncthreads();

    const int k = lane & 3;                                // column of the stats row this lane stores
    for (int i = w; i < n; i += METEOR_WAVES) {
        MeteorSide p;
        p.len = __builtin_amdgcn_readfirstlane(s_len[i]);  // (wave-uniform, and provably so)
        p.id = s_tok[i][lane];
        p.cls = stage2 ? s_cls[i][lane] : 0;
        p.has = stage2 && lane < p.len && p.id >= 0 && p.id < V;
        if (lane < 4) {                                    // the diagonal: (len, len > 0, len, len)
            stats[((row0 + i) * n + i) * 4 + lane] = lane == 1 ? (p.len > 0 ? 1 : 0) : p.len;
        }
        for (int d = 1; 2 * d <= n; ++d) {
            if (2 * d == n && i >= d) break;               // (wave-uniform) the pair at distance n / 2 belongs to its lower end
            const int j = i + d < n ? i + d : i + d - n;
            MeteorSide q;
            q.len = __builtin_amdgcn_readfirstlane(s_len[j]);
            q.id = s_tok[j][lane];
            q.cls = stage2 ? s_cls[j][lane] : 0;
            q.has = stage2 && lane < q.len && q.id >= 0 && q.id < V;
            int m, chunks;
            meteor_pair(p, q, lane, stage2, m, chunks);
            const bool fwd = lane < 4;                     // lanes 0..3: row [i][j]; lanes 4..7: row [j][i]
            const int hyp = fwd ? i : j, ref = fwd ? j : i;
            int out = fwd ? q.len : p.len;                 // k == 3: ref_len
            out = k == 0 ? m : out;
            out = k == 1 ? chunks : out;
            out = k == 2 ? (fwd ? p.len : q.len) : out;
            if (lane < 8) stats[((row0 + hyp) * n + ref) * 4 + k] = out;
        }
    }
}

}  // namespace fira

extern "C" int fira_dev_meteor_stats(void* stream, int B, int T, int V, int L, int S, const int32_t* ids, const int32_t* sou,
                                     const int32_t* sub_token, const int32_t* tar, const int32_t* classes, int32_t* stats) {
    using namespace fira;
    FIRA_REQUIRE(B >= 0, "fira_dev_meteor_stats: B = %d is negative", B);
    FIRA_REQUIRE(T >= 1 && T <= BLEU_T, "fira_dev_meteor_stats: T = %d outside 1..%d (one lane per position)", T, BLEU_T);
    FIRA_REQUIRE(V > BLEU_UNK && L >= 1 && S >= 1, "fira_dev_meteor_stats: V = %d, L = %d, S = %d (need V >= 4, L >= 1, S >= 1)",
                 V, L, S);
    FIRA_REQUIRE((int64_t)V + L + S <= 0x7fffffff, "fira_dev_meteor_stats: V + L + S overflows int32");
    if (B == 0) return 0;
    FIRA_REQUIRE(ids && sou && sub_token && tar && stats, "fira_dev_meteor_stats: null pointer");
    hipLaunchKernelGGL(dev_meteor_stats_kernel, dim3(cdiv(B, METEOR_CPW)), dim3(METEOR_CPW * 64), 0, (hipStream_t)stream, B, T, V,
                       L, S, ids, sou, sub_token, tar, classes, stats);
    FIRA_CHECK_LAUNCH("fira_dev_meteor_stats");
    return 0;
}

extern "C" int fira_mbr_meteor_stats(void* stream, int B, int n, int T, const int32_t* tokens, const int32_t* length, int V,
                                     const int32_t* classes, int32_t* stats) {
    using namespace fira;
    FIRA_REQUIRE(B >= 0, "fira_mbr_meteor_stats: B = %d is negative", B);
    FIRA_REQUIRE(n >= 1 && n <= MBR_N, "fira_mbr_meteor_stats: n = %d outside 1..%d (candidates per commit)", n, MBR_N);
    FIRA_REQUIRE(T >= 1 && T <= BLEU_T, "fira_mbr_meteor_stats: T = %d outside 1..%d (one lane per position)", T, BLEU_T);
    FIRA_REQUIRE(!classes || V > BLEU_UNK, "fira_mbr_meteor_stats: V = %d with a class table (need V >= 4)", V);
    if (B == 0) return 0;
    FIRA_REQUIRE(tokens && length && stats, "fira_mbr_meteor_stats: null pointer (tokens, length or stats)");
    hipLaunchKernelGGL(mbr_meteor_stats_kernel, dim3(B), dim3(METEOR_WAVES * 64), 0, (hipStream_t)stream, n, T, tokens, length, V,
                       classes, stats);
    FIRA_CHECK_LAUNCH("fira_mbr_meteor_stats");
    return 0;
}
