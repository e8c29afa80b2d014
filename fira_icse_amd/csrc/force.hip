// Prefix-forced search: the decode step's output distribution cut down to the one word a given message start asks for.
//
// fira_force_dist edits dist [R, W] (W = V + L + S: generator ids, diff positions, sub-token positions) in place between
// fira_decode_step (fira_mix_dist, fira_merge_dist) and fira_constrain_dist / the selection.  It is the mirror image of
// fira_constrain_dist: that kernel zeroes the entries of the blocked words and keeps the rest, this one keeps the entries of ONE
// word and zeroes the rest.  Row r of commit b = r / rows_per_commit has emitted m = length[r] - 1 words; while m is below the
// commit's prefix_len[b] (and the row has not ended with <eos>) the row is FORCED to the word y = prefix[b, m]: every entry i
// with w(i) != y becomes exactly +0.0f, every entry with w(i) == y -- the generator entry y, if y is inside [0, V), and every
// copy slot that carries y -- keeps its bits, nothing is renormalised.  w(i) is what the selection kernels resolve entry i to
// (constrain.hip).  A row that is not forced is left alone.  prefix and prefix_len are device arrays read when the kernel runs:
// one captured graph serves every prefix.
//
// One workgroup of 1024 threads per row:
//   1. every thread reads the row's state (length, last id, the commit's prefix length: the same few addresses for the whole
//      workgroup).  A row that is not forced ends here when no arg-max is asked for: two small dependent loads.
//   2. the LDS bitmap of W bits is cleared; with best_id a row that is not forced takes one stream_row_marked pass into an ArgMax
//      (the marks are all clear) and ends.
//   3. a forced row: every thread requests the source id of "its" slot (slot_word: L + S <= 1024) and marks the slot's bit where
//      the id is y; thread 0 marks the generator bit of y.  The bitmap now holds the KEPT entries.  LDS atomics only.
//   4. with best_id: the row is not read -- the holder of a kept slot offers that one value, thread 0 offers the generator entry
//      and (0.0f, the lowest index that is zeroed), which stands for every zero the stores below write.
//   5. the stores, cut at the row's 16-byte boundaries (RowSplit): a vector whose four bits are clear is one 16-byte store of
//      zeros; a vector with a kept entry, and the elements before the first and after the last boundary, take 4-byte stores.
// A forced row is written once (about 4 W bytes) and read at a handful of addresses; a free row is read once or not at all.
#include "decode_row.h"

namespace fira {

constexpr int FRC_EOS = 1;                      // config.EOS

__global__ __launch_bounds__(DDW_NT) void force_dist_kernel(int T, int V, int L, int S, int rows_per_commit,
                                                            const int32_t* __restrict__ gen,
                                                            const int32_t* __restrict__ length,
                                                            const int32_t* __restrict__ sou,
                                                            const int32_t* __restrict__ sub,
                                                            const int32_t* __restrict__ prefix,
                                                            const int32_t* __restrict__ prefix_len,
                                                            float* __restrict__ dist, int32_t* __restrict__ best_id,
                                                            float* __restrict__ best_p) {
    __shared__ uint32_t s_bm[bitmap_words(ROW_MAX_V + ROW_MAX_SLOTS)];
    __shared__ float smf[DDW_NT / 64];
    __shared__ int smi[DDW_NT / 64];
    const int r = blockIdx.x, tid = threadIdx.x;
    const size_t b = (size_t)(r / rows_per_commit);
    const int NS = L + S, W = V + NS;
    const int n_words = (W + 31) / 32;

    // ---- 1. the row's state (workgroup-uniform addresses and values)
    const int len = min(max(length[r], 1), T);
    const int n_pre = min(max(prefix_len[b], 0), T);
    const int m = len - 1;                                 // words after <start>
    const bool finished = gen[(size_t)r * T + m] == FRC_EOS;
    const bool forced = !finished && m < n_pre;
    if (!forced && !best_id) return;                       // (workgroup-uniform) nothing to edit, nothing to report

    // ---- 2. the bitmap cleared; a free row's arg-max
    for (int w = tid; w <= n_words; w += DDW_NT) s_bm[w] = 0;
    float* row = dist + (size_t)r * W;
    if (!forced) {
        __syncthreads();
        ArgMax best;
        stream_row_marked(row, W, tid, s_bm, [&](float v, int i, unsigned) { best.offer(v, i); });
        best.reduce(smf, smi);
        best.report(best_id, best_p, r);
        return;
    }

    // ---- 3. mark the kept entries: the slots that carry y, the generator entry y
    const int y = prefix[b * T + m];                       // (m < n_pre <= T)
    const int src = slot_word(sou, sub, b, L, S, tid);
    const int yg = y >= 0 && y < V ? y : -1;               // an id outside [0, V) is never used as an index
    const bool keep = tid < NS && src == y;
    __syncthreads();
    if (keep) atomicOr(&s_bm[(V + tid) >> 5], 1u << ((V + tid) & 31));
    if (tid == 0 && yg >= 0) atomicOr(&s_bm[yg >> 5], 1u << (yg & 31));

    // ---- 4. arg-max of the edited row from the kept entries alone (requested before the stores; no store touches them)
    if (best_id) {
        ArgMax best;
        const float pv = keep ? row[V + tid] : 0.0f;
        const float gv = tid == 0 && yg >= 0 ? row[yg] : 0.0f;
        if (keep) best.offer(pv, V + tid);
        if (tid == 0) {
            if (yg >= 0) best.offer(gv, yg);
            best.offer(0.0f, yg == 0 ? 1 : 0);             // the zeros: index 0, or 1 where entry 0 is the kept one (V >= 4)
        }
        best.reduce(smf, smi);                             // (its barriers also publish the bitmap)
        best.report(best_id, best_p, r);
    } else {
        __syncthreads();
    }

    // ---- 5. the stores: +0.0f wherever the bit is clear
    const RowSplit c(row, W);
    if (tid < c.head && !((s_bm[tid >> 5] >> (tid & 31)) & 1u)) row[tid] = 0.0f;
    if (tid >= DDW_NT - 4 && c.tail_of(tid) < W) {
        const int i = c.tail_of(tid);
        if (!((s_bm[i >> 5] >> (i & 31)) & 1u)) row[i] = 0.0f;
    }
    float4* rowv = reinterpret_cast<float4*>(row + c.head);
    for (int v = tid; v < c.nvec; v += DDW_NT) {
        const int i = c.head + 4 * v;
        const uint64_t two = ((uint64_t)s_bm[(i >> 5) + 1] << 32) | s_bm[i >> 5];
        const unsigned bits = (unsigned)(two >> (i & 31)) & 15u;
        if (!bits) {
            rowv[v] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        } else {                                           // around a kept entry: 4-byte stores
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (!((bits >> u) & 1u)) row[i + u] = 0.0f;
        }
    }
}

}  // namespace fira

extern "C" int fira_force_dist(void* stream, const fira_dims* d, int R, int rows_per_commit, const int32_t* gen,
                               const int32_t* length, const int32_t* sou, const int32_t* sub_token, const int32_t* prefix,
                               const int32_t* prefix_len, float* dist, int32_t* best_id, float* best_p) {
    using namespace fira;
    if (int e = require_row_geometry(d, rows_per_commit, R, best_id, best_p, "fira_force_dist")) return e;
    FIRA_REQUIRE(d->tar_len >= 2 && d->tar_len <= ROW_MAX_T, "fira_force_dist: tar_len = %d outside 2..%d", d->tar_len, ROW_MAX_T);
    if (R == 0) return 0;
    FIRA_REQUIRE(gen && length && sou && sub_token && dist, "fira_force_dist: null pointer (gen, length, sou, sub_token or dist)");
    FIRA_REQUIRE(prefix && prefix_len, "fira_force_dist: null pointer (prefix or prefix_len)");
    hipLaunchKernelGGL(force_dist_kernel, dim3(R), dim3(DDW_NT), 0, (hipStream_t)stream, d->tar_len, d->vocab, d->sou_len,
                       d->sub_len, rows_per_commit, gen, length, sou, sub_token, prefix, prefix_len, dist, best_id, best_p);
    FIRA_CHECK_LAUNCH("fira_force_dist");
    return 0;
}
