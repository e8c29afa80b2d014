// Retrieval-augmented search: the vector of a commit, its nearest stored vector, and the mix of the
// neighbour's step distribution into the input's.
//
// fira_pool_memory    u[b] = v[b] / |v[b]|,  v[b, c] = (sum over valid s of mem[b, s, c]) / n_b.  One workgroup of 256 threads per
//                     commit, one column per thread: the sum in ascending s, then -- every thread for itself, over the 256 means
//                     in LDS, in ascending c -- the sum of squares.  Every operation is one IEEE fp32 operation in a fixed order
//                     (no contraction, no tree), so a loop of np.float32 operations is the reference.  Rows with valid == 0 are
//                     never read.
// fira_nn_search      top-1 of <Q[b], store[j]> over j != exclude[b] for up to 64 queries in ONE pass over the store.  The
//                     queries sit in LDS (16 per query block, up to 4 blocks = 64 KB, 16-byte columns swizzled by the row so that
//                     the fragment reads spread over the banks); a wave takes a tile of 16 store rows straight from global memory
//                     into registers (16 x 16 bytes per lane, each instruction 64 contiguous bytes of 16 rows, the next tile
//                     requested before this one is used) and forms tile x Q^T with v_mfma_f32_16x16x4_f32: 64 k-steps per
//                     query block, an ordered fp32 fma chain per (row, query), the same chain wherever the row sits in the store
//                     -- identical rows tie exactly.  By instruction count: 4 MFMA (32 cycles each) per 16 rows x 16 queries x
//                     16 k against ~10 VALU instructions per (row, query) pair for lane-sliced FMA plus DPP butterflies; at 64
//                     queries the matrix form needs 2.5 GFLOP = 16 us of the chip's fp32 matrix rate beside 12 us of HBM time
//                     for 77 MB, the butterfly form 100-160 us of VALU issue.  (Measured, profiles/retrieve_probe.md: 103-113 us, the
//                     load side and not the matrix work bounds it; whole rows through an LDS staging tile is the form to try
//                     next.)  No [B, N] scores leave the chip: every lane keeps the
//                     best (value, index) of its query column, the lanes of a column and the waves are combined under (value
//                     descending, index ascending), and a workgroup writes one partial winner per query.  A second launch of one
//                     workgroup combines the partials in the same order.  NaN never wins (it is never greater than anything).
// fira_mix_neighbour  p[i] = a p[i] (i >= vocab),  p[w] = (a p[w]) + (b q[w]) (w < vocab), (a, b) = coef[commit] read from the
//                     device; fira_mix_dist's kernel shape (one workgroup per row, the row cut at dist's 16-byte boundaries), every
//                     multiply and add rounded on its own.
// Vector stores only, no atomics.
#include <math.h>
#include "decode_row.h"

namespace fira {

// ---------------------------------------------------------------- pool
constexpr int POOL_NT = FIRA_D;

__global__ __launch_bounds__(POOL_NT) void pool_memory_kernel(int S, const float* __restrict__ mem, const int32_t* __restrict__ valid,
                                                              float* __restrict__ out) {
#pragma clang fp contract(off)
    __shared__ float sv[FIRA_D];
    const int b = blockIdx.x, c = threadIdx.x;
    const float* m = mem + (size_t)b * S * FIRA_D;
    const int32_t* mv = valid + (size_t)b * S;
    float acc = 0.f;
    int n = 0;
    for (int s = 0; s < S; ++s) {
        if (mv[s] != 0) {                                      // (workgroup-uniform)
            acc = acc + m[(size_t)s * FIRA_D + c];
            ++n;
        }
    }
    const float v = n > 0 ? acc / (float)n : 0.f;
    sv[c] = v;
    __syncthreads();
    float ss = 0.f;
    for (int k = 0; k < FIRA_D; ++k) {
        const float t = sv[k] * sv[k];
        ss = ss + t;
    }
    const float nrm = sqrtf(ss);
    out[(size_t)b * FIRA_D + c] = nrm > 0.f ? v / nrm : 0.f;   // (n_b = 0, |v| = 0 and a NaN norm: 0)
}

// ---------------------------------------------------------------- nearest neighbour
constexpr int NN_NT = 256, NN_WAVES = NN_NT / 64, NN_TILE = 16, NN_MAX_B = 64, NN_MAX_GRID = 256;   // (one workgroup per CU: the 64-query form takes all 256 VGPRs)
typedef float nn_acc __attribute__((ext_vector_type(4)));

// float offset of 16-byte column `quad` (0..63) of query row `row` in LDS
__device__ __forceinline__ int nn_off(int row, int quad) { return row * FIRA_D + ((quad ^ (row & 15)) << 2); }

struct NnPartial { float v; int i; };

template <int QB>
__global__ __launch_bounds__(NN_NT) void nn_search_kernel(const float* __restrict__ Q, int B, const float* __restrict__ store, int N,
                                                          const int32_t* __restrict__ exclude, NnPartial* __restrict__ part) {
    extern __shared__ float4 nn_lds4[];
    float* sq = reinterpret_cast<float*>(nn_lds4);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, kq = lane >> 4;

    // the queries: row r of Q as 64 16-byte columns, rows past B zero
    for (int x = tid; x < QB * 16 * 64; x += NN_NT) {
        const int r = x >> 6, quad = x & 63;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (r < B) v = *reinterpret_cast<const float4*>(Q + (size_t)r * FIRA_D + 4 * quad);
        *reinterpret_cast<float4*>(sq + nn_off(r, quad)) = v;
    }
    int excl[QB];
#pragma unroll
    for (int qb = 0; qb < QB; ++qb) {
        const int q = qb * 16 + l15;
        excl[qb] = (exclude && q < B) ? exclude[q] : -1;
    }
    __syncthreads();

    float bv[QB];
    int bi[QB];
#pragma unroll
    for (int qb = 0; qb < QB; ++qb) { bv[qb] = -INFINITY; bi[qb] = INT_MAX; }

    const int n_tiles = (N + NN_TILE - 1) / NN_TILE;
    const int stride = gridDim.x * NN_WAVES;
    int t = blockIdx.x * NN_WAVES + wave;                      // (wave-uniform)
    // lane (l15, kq) holds columns 16 m + 4 kq .. + 3 of row 16 t + l15 in a[m]; a row past the store is row N - 1 again
    auto load = [&](int tile, float4 (&a)[16]) {
        const int row = min(tile * NN_TILE + l15, N - 1);
        const float4* p = reinterpret_cast<const float4*>(store + (size_t)row * FIRA_D) + kq;
#pragma unroll
        for (int m = 0; m < 16; ++m) a[m] = p[4 * m];
    };
    float4 a[16];
    if (t < n_tiles) load(t, a);
    while (t < n_tiles) {
        const int tn = t + stride;
        float4 an[16];
        if (tn < n_tiles) load(tn, an);
        nn_acc acc[QB];
#pragma unroll
        for (int qb = 0; qb < QB; ++qb) acc[qb] = nn_acc{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int m = 0; m < 16; ++m) {
            float4 q[QB];
#pragma unroll
            for (int qb = 0; qb < QB; ++qb) q[qb] = *reinterpret_cast<const float4*>(sq + nn_off(qb * 16 + l15, 4 * m + kq));
            // (the query blocks' accumulators in turn: a dependent MFMA has 40 cycles of latency, an independent one issues in 32)
#pragma unroll
            for (int qb = 0; qb < QB; ++qb) acc[qb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[m].x, q[qb].x, acc[qb], 0, 0, 0);
#pragma unroll
            for (int qb = 0; qb < QB; ++qb) acc[qb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[m].y, q[qb].y, acc[qb], 0, 0, 0);
#pragma unroll
            for (int qb = 0; qb < QB; ++qb) acc[qb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[m].z, q[qb].z, acc[qb], 0, 0, 0);
#pragma unroll
            for (int qb = 0; qb < QB; ++qb) acc[qb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[m].w, q[qb].w, acc[qb], 0, 0, 0);
        }
        // acc[qb][r]: row 16 t + 4 kq + r against query 16 qb + l15
#pragma unroll
        for (int qb = 0; qb < QB; ++qb) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int j = t * NN_TILE + 4 * kq + r;
                const float v = acc[qb][r];
                if (j < N && j != excl[qb] && (v > bv[qb] || (v == bv[qb] && j < bi[qb]))) { bv[qb] = v; bi[qb] = j; }
            }
        }
        if (tn < n_tiles) {
#pragma unroll
            for (int m = 0; m < 16; ++m) a[m] = an[m];
        }
        t = tn;
    }

    // the four lanes of a query column, then the waves (through the LDS the queries no longer need)
#pragma unroll
    for (int qb = 0; qb < QB; ++qb) {
#pragma unroll
        for (int o = 16; o < 64; o <<= 1) {
            const float ov = __shfl_xor(bv[qb], o, 64);
            const int oi = __shfl_xor(bi[qb], o, 64);
            if (ov > bv[qb] || (ov == bv[qb] && oi < bi[qb])) { bv[qb] = ov; bi[qb] = oi; }
        }
    }
    __syncthreads();
    NnPartial* sp = reinterpret_cast<NnPartial*>(sq);          // [NN_WAVES][QB * 16]
    if (kq == 0) {
#pragma unroll
        for (int qb = 0; qb < QB; ++qb) sp[wave * (QB * 16) + qb * 16 + l15] = NnPartial{bv[qb], bi[qb]};
    }
    __syncthreads();
    if (tid < B) {
        NnPartial best = sp[tid];
#pragma unroll
        for (int w = 1; w < NN_WAVES; ++w) {
            const NnPartial o = sp[w * (QB * 16) + tid];
            if (o.v > best.v || (o.v == best.v && o.i < best.i)) best = o;
        }
        part[(size_t)blockIdx.x * NN_MAX_B + tid] = best;
    }
}

__global__ __launch_bounds__(NN_MAX_B) void nn_reduce_kernel(const NnPartial* __restrict__ part, int G, int B,
                                                             int32_t* __restrict__ best_idx, float* __restrict__ best_sim) {
    const int q = threadIdx.x;
    if (q >= B) return;
    NnPartial best = part[q];
    for (int g = 1; g < G; ++g) {
        const NnPartial o = part[(size_t)g * NN_MAX_B + q];
        if (o.v > best.v || (o.v == best.v && o.i < best.i)) best = o;
    }
    const bool none = best.i == INT_MAX;                       // every admissible row's product was NaN
    best_idx[q] = none ? -1 : best.i;
    best_sim[q] = none ? 0.f : fminf(fmaxf(best.v, 0.f), 1.f);
}

static int nn_grid(int N) {
    const int n_tiles = (N + NN_TILE - 1) / NN_TILE;
    const int g = (n_tiles + NN_WAVES - 1) / NN_WAVES;
    return g < 1 ? 1 : (g > NN_MAX_GRID ? NN_MAX_GRID : g);
}

template <int QB>
static int nn_launch(hipStream_t s, int G, const float* Q, int B, const float* store, int N, const int32_t* exclude, NnPartial* part) {
    constexpr size_t lds = (size_t)QB * 16 * FIRA_D * sizeof(float);
    static_assert(lds <= 64 * 1024, "the queries fit the default dynamic LDS limit");
    static_assert(NN_WAVES * QB * 16 * sizeof(NnPartial) <= lds, "the wave partials reuse the queries' LDS");
    hipLaunchKernelGGL(nn_search_kernel<QB>, dim3(G), dim3(NN_NT), lds, s, Q, B, store, N, exclude, part);
    return 0;
}

// ---------------------------------------------------------------- mix
__device__ __forceinline__ float mixn_elem(float a, float b, float p, float q, bool word) {
#pragma clang fp contract(off)
    const float x = a * p;
    const float y = b * q;
    const float z = x + y;
    return word ? z : x;
}

__global__ __launch_bounds__(DDW_NT) void mix_neighbour_kernel(int V, int W, int rows_per_commit, const float* __restrict__ coef,
                                                               const float* __restrict__ q, float* dist,
                                                               int32_t* __restrict__ best_id, float* __restrict__ best_p) {
    __shared__ float smf[DDW_NT / 64];
    __shared__ int smi[DDW_NT / 64];
    const int r = blockIdx.x, tid = threadIdx.x;
    const int cb = r / rows_per_commit;
    const float ca = coef[2 * cb], cq = coef[2 * cb + 1];
    const size_t off = (size_t)r * W;
    float* prow = dist + off;
    const float* qrow = q + off;
    const RowSplit c(prow, W);
    const int head = c.head, nvec = c.nvec;
    const bool wide = ((uintptr_t)(qrow + head) & 15u) == 0;   // (workgroup-uniform)

    ArgMax best;
    auto scalar = [&](int i) {
        const float y = mixn_elem(ca, cq, prow[i], qrow[min(i, V - 1)], i < V);
        prow[i] = y;
        best.offer(y, i);
    };
    if (tid < head) scalar(tid);
    if (tid >= DDW_NT - 4 && c.tail_of(tid) < W) scalar(c.tail_of(tid));

    for (int v0 = tid; v0 < nvec; v0 += 2 * DDW_NT) {
        float4 x[2], z[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int i = head + 4 * min(v0 + u * DDW_NT, nvec - 1);           // (clamped: requested, not used, past the end)
            x[u] = *reinterpret_cast<const float4*>(prow + i);
            const float* qq = qrow + i;
            if (i >= V) z[u] = make_float4(0.f, 0.f, 0.f, 0.f);                // the input's own copy entries: q is not read
            else if (wide) z[u] = *reinterpret_cast<const float4*>(qq);
            else z[u] = make_float4(qq[0], qq[1], qq[2], qq[3]);
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int v = v0 + u * DDW_NT;
            if (v < nvec) {
                const int i = head + 4 * v;
                const float4 y = make_float4(mixn_elem(ca, cq, x[u].x, z[u].x, i < V), mixn_elem(ca, cq, x[u].y, z[u].y, i + 1 < V),
                                             mixn_elem(ca, cq, x[u].z, z[u].z, i + 2 < V), mixn_elem(ca, cq, x[u].w, z[u].w, i + 3 < V));
                *reinterpret_cast<float4*>(prow + i) = y;
                best.offer(y.x, i);
                best.offer(y.y, i + 1);
                best.offer(y.z, i + 2);
                best.offer(y.w, i + 3);
            }
        }
    }
    if (!best_id) return;                                      // (workgroup-uniform)
    best.reduce(smf, smi);
    best.report(best_id, best_p, r);
}

}  // namespace fira

extern "C" int fira_pool_memory(void* stream, const fira_dims* d, int B, const float* mem, const int32_t* mem_valid, float* out) {
    using namespace fira;
    FIRA_REQUIRE(d, "fira_pool_memory: null dims");
    FIRA_REQUIRE(d->d_model == FIRA_D, "fira_pool_memory: d_model = %d, the kernels are built for %d", d->d_model, FIRA_D);
    FIRA_REQUIRE(B >= 0, "fira_pool_memory: B = %d is negative", B);
    FIRA_REQUIRE(d->sou_len >= 0 && d->sub_len >= 0, "fira_pool_memory: negative memory length");
    if (B == 0) return 0;
    FIRA_REQUIRE(mem && mem_valid && out, "fira_pool_memory: null pointer (mem, mem_valid or out)");
    hipLaunchKernelGGL(pool_memory_kernel, dim3(B), dim3(POOL_NT), 0, (hipStream_t)stream, d->sou_len + d->sub_len, mem, mem_valid,
                       out);
    FIRA_CHECK_LAUNCH("fira_pool_memory");
    return 0;
}

extern "C" size_t fira_nn_search_scratch_bytes(int B, int N) {
    using namespace fira;
    if (B <= 0 || B > NN_MAX_B || N <= 0) return 0;
    return (size_t)nn_grid(N) * NN_MAX_B * sizeof(NnPartial);
}

extern "C" int fira_nn_search(void* stream, const float* Q, int B, const float* store, int N, const int32_t* exclude,
                              int32_t* best_idx, float* best_sim, void* scratch, size_t scratch_bytes) {
    using namespace fira;
    FIRA_REQUIRE(B > 0, "fira_nn_search: B = %d queries, at least one is needed", B);
    FIRA_REQUIRE(B <= NN_MAX_B, "fira_nn_search: B = %d queries, more than %d per call", B, NN_MAX_B);
    FIRA_REQUIRE(N > 0, "fira_nn_search: N = %d, the store is empty", N);
    FIRA_REQUIRE(!(exclude && N < 2), "fira_nn_search: exclude with a store of %d row leaves no row to return", N);
    FIRA_REQUIRE(Q && store && best_idx && best_sim && scratch, "fira_nn_search: null pointer (Q, store, best_idx, best_sim or scratch)");
    FIRA_REQUIRE(((uintptr_t)Q & 15u) == 0 && ((uintptr_t)store & 15u) == 0, "fira_nn_search: Q and store must be 16-byte aligned");
    const size_t need = fira_nn_search_scratch_bytes(B, N);
    FIRA_REQUIRE(scratch_bytes >= need, "fira_nn_search: scratch of %zu bytes, %zu needed", scratch_bytes, need);
    FIRA_REQUIRE(((uintptr_t)scratch & 7u) == 0, "fira_nn_search: scratch must be 8-byte aligned");
    const hipStream_t s = (hipStream_t)stream;
    const int G = nn_grid(N);
    NnPartial* part = (NnPartial*)scratch;
    switch ((B + 15) / 16) {
        case 1: nn_launch<1>(s, G, Q, B, store, N, exclude, part); break;
        case 2: nn_launch<2>(s, G, Q, B, store, N, exclude, part); break;
        case 3: nn_launch<3>(s, G, Q, B, store, N, exclude, part); break;
        default: nn_launch<4>(s, G, Q, B, store, N, exclude, part); break;
    }
    FIRA_CHECK_LAUNCH("fira_nn_search");
    hipLaunchKernelGGL(nn_reduce_kernel, dim3(1), dim3(NN_MAX_B), 0, s, part, G, B, best_idx, best_sim);
    FIRA_CHECK_LAUNCH("fira_nn_search (reduce)");
    return 0;
}

extern "C" int fira_mix_neighbour(void* stream, const fira_dims* d, int R, int rows_per_commit, const float* coef, const float* q,
                                  float* dist, int32_t* best_id, float* best_p) {
    using namespace fira;
    if (int e = require_row_geometry(d, rows_per_commit, R, best_id, best_p, "fira_mix_neighbour")) return e;
    if (R == 0) return 0;
    FIRA_REQUIRE(coef && q && dist, "fira_mix_neighbour: null pointer (coef, q or dist)");
    const int W = d->vocab + d->sou_len + d->sub_len;
    const size_t n = (size_t)R * W;
    FIRA_REQUIRE(q + n <= dist || dist + n <= q, "fira_mix_neighbour: q overlaps dist");
    hipLaunchKernelGGL(mix_neighbour_kernel, dim3(R), dim3(DDW_NT), 0, (hipStream_t)stream, d->vocab, W, rows_per_commit, coef, q,
                       dist, best_id, best_p);
    FIRA_CHECK_LAUNCH("fira_mix_neighbour");
    return 0;
}
