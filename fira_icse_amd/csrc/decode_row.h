// The decode-row toolkit: what the 1024-thread kernels that work on one row of the decode step's output distribution
// dist[r, 0 .. V + L + S) have in common.  A kernel that includes this header states only what it adds.
//   geometry    ROW_MAX_V / ROW_MAX_SLOTS / ROW_MAX_T, BEAM_MAX, require_row_geometry (host)
//   reductions  block16_sum, block16_min, block16_max, block16_argmax: the 16 wave partials combined in one fixed order, every
//               thread gets the result
//   the order   better(): value descending, index ascending; NaN is never better than anything.  ArgMax carries it.
//   the row     WideRow: the distribution itself (decode_dist_wide_kernel, sample_dist_kernel, score_dist_kernel) -- one
//               body, so the three kernels' rows are bit-identical by construction
//   words       slot_word (copy slot -> source id), entry_word (entry -> vocabulary id)
//   streaming   RowSplit, stream_row_marked: a row read once in 16-byte loads whatever its alignment
//   noise       noise_stream, gumbel_noise: the counter-hash Gumbel perturbation of the sampler and the stochastic beam
//   selection   TopList, pass_through_done, write_hypotheses: the two beam-select kernels' bookkeeping
#pragma once
#include <limits.h>
#include "common.h"
#include "epilogue.h"

namespace fira {

constexpr int DDW_NT = 1024, DDW_NPT = 25;
constexpr int ROW_MAX_V = DDW_NPT * DDW_NT;     // 25 600 generator entries: 25 registers of each thread
constexpr int ROW_MAX_SLOTS = DDW_NT;           // 1 024 copy slots (L + S): one per thread
constexpr int ROW_MAX_T = 64;                   // hypothesis positions: one per lane of a wave
constexpr int BEAM_MAX = 8;
constexpr float ROW_MASKED = -1e9f;             // the copy score of a slot outside the commit's memory

// The argument checks of a call that edits dist rows of `d`'s geometry, R rows, rows_per_commit of them per commit.
inline int require_best_pair(const int32_t* best_id, const float* best_p, const char* who) {
    FIRA_REQUIRE((best_id == nullptr) == (best_p == nullptr), "%s: best_id and best_p are given together or not at all", who);
    return 0;
}
inline int require_row_geometry(const fira_dims* d, int rows_per_commit, int R, const int32_t* best_id, const float* best_p,
                                const char* who) {
    FIRA_REQUIRE(d, "%s: null dims", who);
    FIRA_REQUIRE(R >= 0, "%s: R = %d is negative", who, R);
    FIRA_REQUIRE(rows_per_commit >= 1 && R % rows_per_commit == 0, "%s: rows_per_commit = %d must be >= 1 and divide R = %d", who,
                 rows_per_commit, R);
    FIRA_REQUIRE(d->vocab >= 4 && d->vocab <= ROW_MAX_V && d->sou_len >= 0 && d->sub_len >= 0 &&
                     d->sou_len + d->sub_len <= ROW_MAX_SLOTS,
                 "%s: vocabulary %d / %d memory slots outside 4..%d / 0..%d", who, d->vocab, d->sou_len + d->sub_len, ROW_MAX_V,
                 ROW_MAX_SLOTS);
    return require_best_pair(best_id, best_p, who);
}

// ---------------------------------------------------------------- the order and the block reductions
__device__ __forceinline__ bool better(float v, int i, float w, int j) { return v > w || (v == w && i < j); }
// (block16_argmax and ArgMax spell the order out under their `if`: as a call it is evaluated without the short circuit, which
// costs decode_dist_wide_kernel 12 VGPRs and makes sample_dist_kernel and score_dist_kernel spill)

__device__ __forceinline__ float block16_sum(float v, float* sm) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
    __syncthreads();
    float t = 0.f;
#pragma unroll
    for (int k = 0; k < DDW_NT / 64; ++k) t += sm[k];
    return t;
}
__device__ __forceinline__ int block16_min(int v, int* sm) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
    __syncthreads();
    int t = sm[0];
#pragma unroll
    for (int k = 1; k < DDW_NT / 64; ++k) t = min(t, sm[k]);
    return t;
}
__device__ __forceinline__ float block16_max(float v, float* sm) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
    __syncthreads();
    float t = sm[0];
#pragma unroll
    for (int k = 1; k < DDW_NT / 64; ++k) t = fmaxf(t, sm[k]);
    return t;
}
__device__ __forceinline__ void block16_argmax(float& v, int& idx, float* smv, int* smi) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(v, o, 64);
        const int oi = __shfl_xor(idx, o, 64);
        if (ov > v || (ov == v && oi < idx)) { v = ov; idx = oi; }
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) { smv[threadIdx.x >> 6] = v; smi[threadIdx.x >> 6] = idx; }
    __syncthreads();
    v = smv[0]; idx = smi[0];
#pragma unroll
    for (int k = 1; k < DDW_NT / 64; ++k)
        if (smv[k] > v || (smv[k] == v && smi[k] < idx)) { v = smv[k]; idx = smi[k]; }
}

// A running arg-max under the order; an empty one (nothing offered, or only NaN) reports entry 0.
struct ArgMax {
    float v = -INFINITY;
    int i = INT_MAX;
    __device__ __forceinline__ void offer(float w, int j) {
        if (w > v || (w == v && j < i)) { v = w; i = j; }
    }
    __device__ __forceinline__ void reduce(float* smf, int* smi) { block16_argmax(v, i, smf, smi); }
    __device__ __forceinline__ void report(int32_t* best_id, float* best_p, int r) const {     // after reduce()
        if (threadIdx.x == 0) { best_id[r] = i == INT_MAX ? 0 : i; best_p[r] = v; }
    }
};

// ---------------------------------------------------------------- the distribution row
// p over the V generator entries and the S <= 1024 copy slots of row r: the V logits requested once and kept in registers
// (entry tid + 1024 i in x[i]), one copy slot per thread, the 2-way gate LinearProb(x) either given or formed here from
// the decoder row (two 256-long dot products).  First-occurrence arg-max as torch.argmax.  logits_row, srow and mv are the
// row's own pointers; the gate is row r of gate_logits [., 2] or, where that is null, of xrow [., 256].
//     p[tid + 1024 i] = sg * x[i]      p[V + tid] = sc * ce
// The largest entry of either part has exp(0) = 1, so the row's maximum is max(sg, sc).
struct WideRow {
    float x[DDW_NPT];                           // exp(logit - max); 0 past V
    float ce;                                   // exp(copy score - max); 0 past S
    float sg, sc;                               // gate share over the softmax sum, generator / copy
    int gidx, cidx;                             // the arg-max of either part
    bool valid;                                 // this thread's slot is inside the commit's memory

    __device__ __forceinline__ void form(int V, int S, const float* __restrict__ logits_row, const float* __restrict__ srow,
                                         const int32_t* __restrict__ mv, int r, const float* __restrict__ gate_logits,
                                         const float* __restrict__ xrow, const float* __restrict__ wp,
                                         const float* __restrict__ bp, float* smf, int* smi) {
        const int tid = threadIdx.x;
        const rsrc_t rL = buf_rsrc(logits_row, (unsigned)V * 4u);
#pragma unroll
        for (int i = 0; i < DDW_NPT; ++i) x[i] = buf_load_f32(rL, (unsigned)(tid + DDW_NT * i) * 4u);   // past V: 0, replaced below
        float z0, z1;
        if (gate_logits) {
            z0 = gate_logits[2 * r]; z1 = gate_logits[2 * r + 1];
        } else {                                                   // gate = x wp^T + bp: two 256-long dot products
            const float xv = tid < FIRA_D ? xrow[(size_t)r * FIRA_D + tid] : 0.f;
            const float a0 = tid < FIRA_D ? xv * wp[tid] : 0.f, a1 = tid < FIRA_D ? xv * wp[FIRA_D + tid] : 0.f;
            z0 = block16_sum(a0, smf) + bp[0];
            z1 = block16_sum(a1, smf) + bp[1];
        }
        const float zm = fmaxf(z0, z1);
        const float e0 = expf(z0 - zm), e1 = expf(z1 - zm);
        const float g0 = e0 / (e0 + e1), g1 = e1 / (e0 + e1);
        float cmax = -INFINITY, gmax = -INFINITY;
        cidx = INT_MAX; gidx = INT_MAX;
        valid = tid < S && mv[tid] != 0;
        const float sv = tid < S ? (valid ? srow[tid] : ROW_MASKED) : -INFINITY;
        if (tid < S) { cmax = sv; cidx = tid; }
        block16_argmax(cmax, cidx, smf, smi);
        ce = tid < S ? expf(sv - cmax) : 0.f;
        const float csum = block16_sum(ce, smf);
#pragma unroll
        for (int i = 0; i < DDW_NPT; ++i) {                      // ascending index within the thread: first maximum wins
            const int j = tid + DDW_NT * i;
            x[i] = j < V ? x[i] : -INFINITY;
            if (x[i] > gmax) { gmax = x[i]; gidx = j; }
        }
        block16_argmax(gmax, gidx, smf, smi);
        float gsum = 0.f;
#pragma unroll
        for (int i = 0; i < DDW_NPT; ++i) {
            x[i] = expf(x[i] - gmax);                            // exp(-inf) = 0 past V
            gsum += x[i];
        }
        gsum = block16_sum(gsum, smf);
        sg = g0 * (1.0f / gsum); sc = g1 * (1.0f / csum);
    }
    // the row to dist (the row's pointer); the generator part by buffer stores, dropped past V
    __device__ __forceinline__ void store(float* __restrict__ drow, int V, int S) const {
        const int tid = threadIdx.x;
        const rsrc_t rD = buf_rsrc(drow, (unsigned)V * 4u);
#pragma unroll
        for (int i = 0; i < DDW_NPT; ++i)
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, sg * x[i]), rD, (unsigned)(tid + DDW_NT * i) * 4u, 0, 0);
        if (tid < S) drow[V + tid] = sc * ce;
    }
    __device__ __forceinline__ int best(int V) const { return sg >= sc ? gidx : V + cidx; }
    __device__ __forceinline__ float best_p() const { return sg >= sc ? sg : sc; }
};

// ---------------------------------------------------------------- words
// The source id of copy slot `slot` of commit b: sou[b, slot] below L, sub[b, slot - L] above.  Both requests are unconditional
// with clamped indices and neither is sunk under the select (bleu.hip), so the two round trips overlap; a slot at or past
// L + S gets the last sub-token id and no fault.
__device__ __forceinline__ int slot_word(const int32_t* __restrict__ sou, const int32_t* __restrict__ sub, size_t b, int L, int S,
                                         int slot) {
    int id_sou = L > 0 ? sou[b * L + min(slot, L - 1)] : 0;
    int id_sub = S > 0 ? sub[b * S + min(max(slot - L, 0), S - 1)] : 0;
    asm volatile("" : "+v"(id_sou), "+v"(id_sub));
    return slot < L ? id_sou : id_sub;
}
// The vocabulary id entry w of a row of commit b resolves to (run_model.py:305-340): itself below V, its copy slot's id above.
__device__ __forceinline__ int entry_word(int w, const int32_t* __restrict__ sou, const int32_t* __restrict__ sub, size_t b, int V,
                                          int L, int S) {
    int nt = w;
    if (w >= V + L) nt = sub[b * S + min(w - V - L, S - 1)];
    else if (w >= V) nt = sou[b * L + (w - V)];
    return nt;
}

// ---------------------------------------------------------------- noise
// The noise stream of row j (sample or beam slot) of the commit with `key` at `step`, T = tar_len, and the Gumbel perturbation
// of entry i under it (include/fira_hip.h, fira_decode_step_sample; the numpy twin: tests/sample_ref.py).
__device__ __forceinline__ uint32_t noise_stream(uint32_t key, uint64_t seed, int j, int T, int step) {
    const uint32_t base = mix32(key ^ mix32((uint32_t)seed ^ mix32((uint32_t)(seed >> 32) + 0x632BE5ABu)));
    return mix32(base + 0x9E3779B9u * (uint32_t)(j * T + step + 1));
}
__device__ __forceinline__ float gumbel_noise(uint32_t stream, uint32_t i) {
    const uint32_t h = mix32(i ^ stream);
    // (m + 0.5) * 2^-24 with m = h >> 8; m = 2^24 - 1 rounds to 1.0 in fp32 -- clamp to the largest float below 1
    const float u = fminf(((float)(h >> 8) + 0.5f) * (1.0f / 16777216.0f), 0x1.fffffep-1f);
    return -logf(-logf(u));
}

// ---------------------------------------------------------------- streaming one row
// A row of n floats cut at its 16-byte boundaries: elements [0, head) and [tail0, n) are read one by one (thread i takes head
// element i, the LAST four threads -- they carry one vector less -- take the tail), [head, tail0) as nvec float4.
struct RowSplit {
    int head, nvec, tail0;
    __device__ __forceinline__ RowSplit(const float* row, int n) {
        head = min((int)(((16u - (unsigned)((uintptr_t)row & 15u)) & 15u) >> 2), n);
        nvec = (n - head) >> 2;
        tail0 = head + 4 * nvec;
    }
    __device__ __forceinline__ int tail_of(int tid) const { return tail0 + (tid - (DDW_NT - 4)); }   // >= n: none
};
constexpr int bitmap_words(int n) { return (n + 31) / 32 + 1; }  // + 1: a 4-bit field may straddle into the next word
// f(value, index, mark) for every element of the row, mark != 0 iff the element's bit in the LDS bitmap is set (bits exist
// below n only; the words up to n / 32 + 1 are readable).  Four 16-byte loads in flight per trip.
template <class F>
__device__ __forceinline__ void stream_row_marked(const float* row, int n, int tid, const uint32_t* bm, F f) {
    const RowSplit c(row, n);
    if (tid < c.head) f(row[tid], tid, (bm[tid >> 5] >> (tid & 31)) & 1u);
    if (tid >= DDW_NT - 4 && c.tail_of(tid) < n) {
        const int i = c.tail_of(tid);
        f(row[i], i, (bm[i >> 5] >> (i & 31)) & 1u);
    }
    const float4* rowv = reinterpret_cast<const float4*>(row + c.head);
    for (int v0 = tid; v0 < c.nvec; v0 += 4 * DDW_NT) {
        float4 x[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) x[u] = rowv[min(v0 + u * DDW_NT, c.nvec - 1)];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int v = v0 + u * DDW_NT;
            if (v < c.nvec) {
                const int i = c.head + 4 * v;
                const uint64_t two = ((uint64_t)bm[(i >> 5) + 1] << 32) | bm[i >> 5];
                const unsigned bits = (unsigned)(two >> (i & 31)) & 15u;
                f(x[u].x, i, bits & 1u);
                f(x[u].y, i + 1, bits & 2u);
                f(x[u].z, i + 2, bits & 4u);
                f(x[u].w, i + 3, bits & 8u);
            }
        }
    }
}

// ---------------------------------------------------------------- beam selection
// A candidate of fira_beam_select: (probability descending, flattened index ascending).
struct Cand {
    float v; int i;
    static __device__ __forceinline__ Cand none() { return {-INFINITY, INT_MAX}; }
    __device__ __forceinline__ bool before(const Cand& o) const { return better(v, i, o.v, o.i); }
};
// The N best candidates a thread has seen, best first.  E: none() (ranks below every candidate) and before().
template <int N, class E>
struct TopList {
    E e[N];
    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int q = 0; q < N; ++q) e[q] = E::none();
    }
    __device__ __forceinline__ bool admits(const E& c) const { return c.before(e[N - 1]); }
    __device__ __forceinline__ void offer(const E& c) {
        if (!admits(c)) return;
        e[N - 1] = c;
#pragma unroll
        for (int q = N - 1; q > 0; --q)
            if (e[q].before(e[q - 1])) { const E t = e[q]; e[q] = e[q - 1]; e[q - 1] = t; }
    }
    __device__ __forceinline__ void pop() {
#pragma unroll
        for (int q = 0; q < N - 1; ++q) e[q] = e[q + 1];
        e[N - 1] = E::none();
    }
};
// search over (*done): a commit's `beam` hypotheses from r0 on are handed on unchanged
__device__ __forceinline__ void pass_through_done(int r0, int beam, int T, const int32_t* __restrict__ gen_in,
                                                  const int32_t* __restrict__ len_in, const float* __restrict__ prob_in,
                                                  int32_t* __restrict__ gen_out, int32_t* __restrict__ len_out,
                                                  float* __restrict__ prob_out, int32_t* __restrict__ parent) {
    const int t = threadIdx.x;
    for (int x = t; x < beam * T; x += DDW_NT) gen_out[(size_t)r0 * T + x] = gen_in[(size_t)r0 * T + x];
    if (t < beam) { len_out[r0 + t] = len_in[r0 + t]; prob_out[r0 + t] = prob_in[r0 + t]; parent[r0 + t] = r0 + t; }
}
// new hypothesis c = hypothesis src_of[c], with tok_of[c] appended unless it is carried (run_model.py:305-340)
__device__ __forceinline__ void write_hypotheses(int r0, int beam, int T, const int* src_of, const int* tok_of, const int* carry_of,
                                                 const int32_t* __restrict__ gen_in, const int32_t* __restrict__ len_in,
                                                 int32_t* __restrict__ gen_out) {
    for (int x = threadIdx.x; x < beam * T; x += DDW_NT) {
        const int c = x / T, p = x - c * T;
        const int src = src_of[c];
        int g = gen_in[(size_t)(r0 + src) * T + p];
        if (!carry_of[c] && p == min(len_in[r0 + src], T - 1)) g = tok_of[c];
        gen_out[(size_t)(r0 + c) * T + p] = g;
    }
}

}  // namespace fira
