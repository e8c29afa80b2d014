// Search over words: the copy entries of the decode step's output distribution folded into the generator entry of their word.
//
// fira_merge_dist edits dist [R, W] (W = V + L + S: generator ids, diff positions, sub-token positions) in place between
// fira_decode_step and the selection (fira_constrain_dist, if any, then fira_beam_select / fira_greedy_advance).  The selection
// kernels resolve an entry to a vocabulary id -- i below V, sou[b, i - V] below V + L, sub_token[b, i - V - L] above -- and only
// that id reaches the hypothesis and the next step, so two entries with one id are one continuation.  Slot s in [0, L + S) has
// the source id w_s.  For every id w in [0, V) that at least one slot carries, with its slots s_1 < s_2 < ... < s_k:
//     acc        = ((p[V + s_1] + p[V + s_2]) + ...) + p[V + s_k]          (fp32, exactly this order)
//     dist[r, w] = acc + dist[r, w]                                         (the generator entry last, as score.hip's p_word)
//     dist[r, V + s_j] = 0.0f
// Every other element keeps its bits (generator entries nobody copies, slots whose id is outside [0, V)); nothing is
// renormalised.  A masked slot holds exactly 0.0f and x + 0.0f == x for x >= 0, so mem_valid is not needed.
//
// One workgroup of 1024 threads per row, one slot per thread (L + S <= 1024):
//   1. every thread requests the source id (slot_word) and the probability of "its" slot (index clamped, no branch) and puts
//      the pair in LDS (id -1 for a slot that is not folded); with best_id the bitmap of V bits is cleared.  One barrier.
//   2. every thread requests the generator entry of its id (clamped: the round trip runs under the walk), then walks the slots
//      0 .. L + S - 1 in order: 8-byte LDS reads at a wave-uniform address.  An equal id BEFORE the thread's slot means the
//      thread is not the leader of its word; an equal id AFTER it is added to acc -- the walk of a leader is p[s_1], + p[s_2], ...
//      in ascending slot order whatever the other waves do.  Waves past the last slot skip the walk.
//   3. the leader stores acc + dist[r, w] (the word's only read-modify-write: no atomics, the same bits in every run and every
//      graph replay); every thread with an id inside [0, V) stores its 0.0f.  Plain vector stores.
//   4. with best_id / best_p: the arg-max of the row AS STORED (ArgMax), without reading back the stores of step 3: the leaders
//      mark their generator entry in the bitmap (LDS atomics) and offer (merged value, w); one stream_row_marked pass over the
//      generator part skips the marked entries; a slot offers what it holds after the edit: 0.0f, or its own value where it was
//      left alone.
// Without best_id the generator part is never streamed: the call costs the slots, not the 100 KB of the row.  There is no
// finished-row case: fira_beam_select ignores finished rows and fira_greedy_advance ignores rows that are not alive.
#include "decode_row.h"

namespace fira {

__global__ __launch_bounds__(DDW_NT) void merge_dist_kernel(int V, int L, int S, int rows_per_commit,
                                                            const int32_t* __restrict__ sou, const int32_t* __restrict__ sub,
                                                            float* __restrict__ dist, int32_t* __restrict__ best_id,
                                                            float* __restrict__ best_p) {
    __shared__ int2 s_slot[ROW_MAX_SLOTS];                 // (id or -1, the bits of p)
    __shared__ uint32_t s_bm[bitmap_words(ROW_MAX_V)];
    __shared__ float smf[DDW_NT / 64];
    __shared__ int smi[DDW_NT / 64];
    const int r = blockIdx.x, tid = threadIdx.x;
    const size_t b = (size_t)(r / rows_per_commit);
    const int NS = L + S, W = V + NS;
    float* row = dist + (size_t)r * W;

    // ---- 1. requests (unconditional, indices clamped); (id, p) to LDS; the bitmap cleared
    const float p = NS > 0 ? row[V + min(tid, NS - 1)] : 0.0f;
    const int src = slot_word(sou, sub, b, L, S, tid);     // (p is requested first: all three loads in flight)
    const bool mine = tid < NS;
    const bool in = mine && src >= 0 && src < V;           // an id outside [0, V) is never used as an index
    s_slot[tid] = make_int2(in ? src : -1, __float_as_int(p));
    if (best_id)
        for (int w = tid; w <= (V + 31) / 32; w += DDW_NT) s_bm[w] = 0;
    __syncthreads();

    // ---- 2. the generator entry requested; the walk over the slots in ascending order
    const int w_idx = in ? src : 0;
    const float g = row[w_idx];                            // (first used after the walk)
    bool lead = in;
    float acc = p;
    if ((tid & ~63) < NS) {                                // (wave-uniform) this wave owns at least one slot
        const int key = in ? src : -2;                     // (-2 equals no stored id)
        for (int j = 0; j < NS; ++j) {
            const int2 e = s_slot[j];                      // wave-uniform address: a broadcast
            const bool same = e.x == key;
            lead = lead && !(same && j < tid);
            if (same && j > tid) acc = acc + __int_as_float(e.y);
        }
    }

    // ---- 3. the stores
    const float merged = acc + g;                          // the generator entry last
    if (lead) {
        row[w_idx] = merged;
        if (best_id) atomicOr(&s_bm[w_idx >> 5], 1u << (w_idx & 31));
    }
    if (in) row[V + tid] = 0.0f;
    if (!best_id) return;                                  // (workgroup-uniform)
    __syncthreads();

    // ---- 4. arg-max of the stored row: the leaders' values, the slots as they are now, the unmarked generator entries
    ArgMax best;
    if (lead) best.offer(merged, w_idx);
    if (mine) best.offer(in ? 0.0f : p, V + tid);
    stream_row_marked(row, V, tid, s_bm, [&](float v, int i, unsigned marked) {
        if (!marked) best.offer(v, i);
    });
    best.reduce(smf, smi);
    best.report(best_id, best_p, r);
}

}  // namespace fira

extern "C" int fira_merge_dist(void* stream, const fira_dims* d, int R, int rows_per_commit, const int32_t* sou,
                               const int32_t* sub_token, float* dist, int32_t* best_id, float* best_p) {
    using namespace fira;
    if (int e = require_row_geometry(d, rows_per_commit, R, best_id, best_p, "fira_merge_dist")) return e;
    if (R == 0) return 0;
    FIRA_REQUIRE(sou && sub_token && dist, "fira_merge_dist: null pointer (sou, sub_token or dist)");
    hipLaunchKernelGGL(merge_dist_kernel, dim3(R), dim3(DDW_NT), 0, (hipStream_t)stream, d->vocab, d->sou_len, d->sub_len,
                       rows_per_commit, sou, sub_token, dist, best_id, best_p);
    FIRA_CHECK_LAUNCH("fira_merge_dist");
    return 0;
}
