// Token-level retrieval for the search (kNN-MT): the K nearest stored decoder states of every row's
// hidden state, and the mix of the words that followed them into the row's distribution.
//
// fira_knn_search   for each of R queries the K rows of keys [N, 256] with the smallest
//                       s_j = key_sq[j] - 2 <q, key_j>
//                   under the total order (s ascending, j ascending), rows with owner[j] == exclude[r] left out; NaN never
//                   wins.  nn_search_kernel's shape (retrieve.hip): a block of up to 64 queries sits in LDS (16-byte columns
//                   swizzled by the row), a wave takes a tile of 16 key rows straight from global memory into registers with
//                   the next tile requested before this one is used, and forms tile x Q^T with v_mfma_f32_16x16x4_f32: an
//                   ordered fp32 chain per (row, query), the same chain wherever the row sits, so identical keys tie exactly.
//                   No [R, N] matrix leaves the chip.  Every wave keeps, per query, an unsorted list of its K best
//                   candidates in LDS ([wave][k][query]: the 16 lanes of a tile column read 16 consecutive entries) and in
//                   registers the list's worst entry as it last saw it: a threshold that only lags, so it lets too much
//                   through and never too little.  A candidate that beats it goes down the slow path: the four lanes of a
//                   query column take turns (wave-uniform branches, skipped when no lane of the turn has a candidate), read
//                   the list, find its worst entry under the order and replace it.  The top K of a set under a total order
//                   does not depend on the order of arrival, so nothing here depends on the schedule.  At the end the four
//                   lists of a query are merged by K rounds of "the best entry after the last one taken" and the workgroup
//                   writes one sorted [K] partial per query; a second launch (one wave per query) merges the partials the same
//                   way from LDS and writes idx and d2 = max(0, q_sq + s), q_sq in ascending column order.
//                   LDS: 16 KB per 16 queries + 4 waves x K x 8 bytes per query: 96 KB at 64 queries and K = 16, one workgroup
//                   of 256 threads per CU (the tile, its successor and the accumulators take the register file as they do in
//                   nn_search_kernel).  Bytes: the keys once per block of 64 queries (1 KB per row) + 8 bytes per row of
//                   key_sq and owner.  profiles/retrieve_probe.md found the load side, not the MFMA, to bound the top-1 scan;
//                   the same holds here with the list upkeep beside it.
// fira_mix_knn      w_k = exp(-(d2_k - d2_0) inv_T) / sum over the non-void slots; every entry of the row times (1 - lam), then
//                   dist[values[idx_k]] += lam w_k for k = 0 .. K - 1 in slot order, every multiply and add rounded on its
//                   own.  mix_neighbour_kernel's row shape: one workgroup per row, the row cut at dist's 16-byte boundaries; a
//                   thread applies the K additions to the entries it holds, so no entry is written twice.  lam == 0 and a row
//                   of void slots: nothing is written.  (lam, inv_T) are read from the device.
// Vector stores only, no atomics.
#include <math.h>
#include "decode_row.h"

namespace fira {

constexpr int KNN_NT = 256, KNN_WAVES = KNN_NT / 64, KNN_TILE = 16, KNN_QBLOCK = 64, KNN_MAX_K = 16, KNN_MAX_GRID = 256;
constexpr int KNN_MAX_N = 8388608;
typedef float knn_acc __attribute__((ext_vector_type(4)));

struct KnnCand { float s; int j; };
// the order: s ascending, j ascending; NaN is never before anything
__device__ __forceinline__ bool knn_before(float s, int j, float t, int i) { return s < t || (s == t && j < i); }

// float offset of 16-byte column `quad` (0..63) of query row `row` in LDS
__device__ __forceinline__ int knn_off(int row, int quad) { return row * FIRA_D + ((quad ^ (row & 15)) << 2); }

// Round k of a merge: the best entry of e[0 .. n) (stride `stride`) that comes after `prev` (every one, when first); none:
// the void entry.  Entries are distinct rows or void, so "after the last one taken" walks them in order.
__device__ __forceinline__ KnnCand knn_next(const KnnCand* e, int n, int stride, KnnCand prev, bool first) {
    KnnCand best{INFINITY, INT_MAX};
    for (int x = 0; x < n; ++x) {
        const KnnCand c = e[(size_t)x * stride];
        if ((first || knn_before(prev.s, prev.j, c.s, c.j)) && knn_before(c.s, c.j, best.s, best.j)) best = c;
    }
    return best;
}

template <int QB>
__global__ __launch_bounds__(KNN_NT) void knn_search_kernel(const float* __restrict__ Q, int R, const float* __restrict__ keys,
                                                            const float* __restrict__ key_sq, const int32_t* __restrict__ owner,
                                                            const int32_t* __restrict__ exclude, int N, int K,
                                                            KnnCand* __restrict__ part) {
#pragma clang fp contract(off)
    extern __shared__ float4 knn_lds4[];
    float* sq = reinterpret_cast<float*>(knn_lds4);
    constexpr int NQ = QB * 16;
    KnnCand* lists = reinterpret_cast<KnnCand*>(sq + NQ * FIRA_D);       // [KNN_WAVES][K][NQ]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, kq = lane >> 4;
    const int q0 = blockIdx.y * KNN_QBLOCK;                              // this block of queries
    const int B = min(R - q0, KNN_QBLOCK);

    for (int x = tid; x < NQ * 64; x += KNN_NT) {
        const int r = x >> 6, quad = x & 63;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (r < B) v = *reinterpret_cast<const float4*>(Q + (size_t)(q0 + r) * FIRA_D + 4 * quad);
        *reinterpret_cast<float4*>(sq + knn_off(r, quad)) = v;
    }
    for (int x = tid; x < KNN_WAVES * K * NQ; x += KNN_NT) lists[x] = KnnCand{INFINITY, INT_MAX};
    int excl[QB];
    bool live[QB];
#pragma unroll
    for (int qb = 0; qb < QB; ++qb) {
        const int q = qb * 16 + l15;
        live[qb] = q < B;
        excl[qb] = (exclude && owner && q < B) ? exclude[q0 + q] : -1;
    }
    __syncthreads();

    KnnCand* mine = lists + (size_t)wave * K * NQ;                       // entry k of query q: mine[k * NQ + q]
    float ws[QB];                                                        // the list's worst entry as this lane last saw it
    int wj[QB];
#pragma unroll
    for (int qb = 0; qb < QB; ++qb) { ws[qb] = INFINITY; wj[qb] = INT_MAX; }

    const int n_tiles = (N + KNN_TILE - 1) / KNN_TILE;
    const int stride = gridDim.x * KNN_WAVES;
    int t = blockIdx.x * KNN_WAVES + wave;                               // (wave-uniform)
    // lane (l15, kq) holds columns 16 m + 4 kq .. + 3 of row 16 t + l15 in a[m], and key_sq / owner of rows 16 t + 4 kq .. + 3
    // (the rows of its accumulators); a row past the store is row N - 1 again
    auto load = [&](int tile, float4 (&a)[16], float (&ks)[4], int (&ow)[4]) {
        const int row = min(tile * KNN_TILE + l15, N - 1);
        const float4* p = reinterpret_cast<const float4*>(keys + (size_t)row * FIRA_D) + kq;
#pragma unroll
        for (int m = 0; m < 16; ++m) a[m] = p[4 * m];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int j = min(tile * KNN_TILE + 4 * kq + r, N - 1);
            ks[r] = key_sq[j];
            ow[r] = owner ? owner[j] : -2;
        }
    };
    float4 a[16];
    float ks[4];
    int ow[4];
    if (t < n_tiles) load(t, a, ks, ow);
    while (t < n_tiles) {
        const int tn = t + stride;
        float4 an[16];
        float ksn[4];
        int own[4];
        if (tn < n_tiles) load(tn, an, ksn, own);
        knn_acc acc[QB];
#pragma unroll
        for (int qb = 0; qb < QB; ++qb) acc[qb] = knn_acc{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int m = 0; m < 16; ++m) {
            float4 q[QB];
#pragma unroll
            for (int qb = 0; qb < QB; ++qb) q[qb] = *reinterpret_cast<const float4*>(sq + knn_off(qb * 16 + l15, 4 * m + kq));
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
            float s[4];
            bool ok[4];
            bool any = false;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int j = t * KNN_TILE + 4 * kq + r;
                const float two = 2.0f * acc[qb][r];
                s[r] = ks[r] - two;
                ok[r] = live[qb] && j < N && ow[r] != excl[qb] && knn_before(s[r], j, ws[qb], wj[qb]);
                any = any || ok[r];
            }
            if (!__any(any)) continue;                                 // (wave-uniform)
            const int q = qb * 16 + l15;
#pragma unroll
            for (int turn = 0; turn < 4; ++turn) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const bool go = kq == turn && ok[r];
                    if (!__any(go)) continue;                          // (wave-uniform)
                    if (go) {
                        // the list's worst entry: the one every other entry comes before (the first void one, if any)
                        float vs = mine[q].s;
                        int vj = mine[q].j, vk = 0;
                        for (int k = 1; k < K; ++k) {
                            const KnnCand c = mine[k * NQ + q];
                            if (knn_before(vs, vj, c.s, c.j)) { vs = c.s; vj = c.j; vk = k; }
                        }
                        const int j = t * KNN_TILE + 4 * kq + r;
                        if (knn_before(s[r], j, vs, vj)) mine[vk * NQ + q] = KnnCand{s[r], j};
                    }
                    // the next turn's lanes read what this turn's wrote
                    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                }
            }
            // the threshold, for all four lanes of the column
            {
                float vs = mine[q].s;
                int vj = mine[q].j;
                for (int k = 1; k < K; ++k) {
                    const KnnCand c = mine[k * NQ + q];
                    if (knn_before(vs, vj, c.s, c.j)) { vs = c.s; vj = c.j; }
                }
                ws[qb] = vs;
                wj[qb] = vj;
            }
        }
        if (tn < n_tiles) {
#pragma unroll
            for (int m = 0; m < 16; ++m) a[m] = an[m];
#pragma unroll
            for (int r = 0; r < 4; ++r) { ks[r] = ksn[r]; ow[r] = own[r]; }
        }
        t = tn;
    }

    // the waves' lists of a query into one sorted [K] partial
    __syncthreads();
    if (tid < B) {
        KnnCand* out = part + (((size_t)blockIdx.y * gridDim.x + blockIdx.x) * KNN_QBLOCK + tid) * K;
        KnnCand prev{INFINITY, INT_MAX};
        for (int k = 0; k < K; ++k) {
            prev = knn_next(lists + tid, KNN_WAVES * K, NQ, prev, k == 0);
            out[k] = prev;
        }
    }
}

constexpr int KNN_MERGE_NT = 64;

__global__ __launch_bounds__(KNN_MERGE_NT) void knn_merge_kernel(const KnnCand* __restrict__ part, int G, int K,
                                                                 const float* __restrict__ Q, int32_t* __restrict__ idx_out,
                                                                 float* __restrict__ d2_out) {
#pragma clang fp contract(off)
    __shared__ KnnCand se[KNN_MAX_GRID * KNN_MAX_K];                     // 32 KB: the query's G partials, [G][K]
    __shared__ float sqq;
    const int r = blockIdx.x, lane = threadIdx.x;
    const int yb = r / KNN_QBLOCK, q = r % KNN_QBLOCK;
    const int n = G * K;
    for (int x = lane; x < n; x += KNN_MERGE_NT) {
        const int g = x / K, k = x - g * K;
        se[x] = part[(((size_t)yb * G + g) * KNN_QBLOCK + q) * K + k];
    }
    if (lane == 0) {
        const float* qr = Q + (size_t)r * FIRA_D;
        float ss = 0.f;
        for (int c = 0; c < FIRA_D; ++c) {
            const float p = qr[c] * qr[c];
            ss = ss + p;
        }
        sqq = ss;
    }
    __syncthreads();
    KnnCand prev{INFINITY, INT_MAX};
    for (int k = 0; k < K; ++k) {
        // every lane its share, then the lanes under the same order
        KnnCand best{INFINITY, INT_MAX};
        for (int x = lane; x < n; x += KNN_MERGE_NT) {
            const KnnCand c = se[x];
            if ((k == 0 || knn_before(prev.s, prev.j, c.s, c.j)) && knn_before(c.s, c.j, best.s, best.j)) best = c;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float os = __shfl_xor(best.s, o, 64);
            const int oj = __shfl_xor(best.j, o, 64);
            if (knn_before(os, oj, best.s, best.j)) { best.s = os; best.j = oj; }
        }
        prev = best;
        if (lane == 0) {
            const bool none = best.j == INT_MAX;
            idx_out[(size_t)r * K + k] = none ? -1 : best.j;
            const float d = sqq + best.s;
            d2_out[(size_t)r * K + k] = none ? INFINITY : fmaxf(d, 0.f);
        }
    }
}

static int knn_grid(int N) {
    const int n_tiles = (N + KNN_TILE - 1) / KNN_TILE;
    const int g = (n_tiles + KNN_WAVES - 1) / KNN_WAVES;
    return g < 1 ? 1 : (g > KNN_MAX_GRID ? KNN_MAX_GRID : g);
}

template <int QB>
static int knn_launch(hipStream_t s, int G, int YB, const float* Q, int R, const float* keys, const float* key_sq,
                      const int32_t* owner, const int32_t* exclude, int N, int K, KnnCand* part) {
    constexpr size_t lds_max = (size_t)QB * 16 * (FIRA_D * sizeof(float) + KNN_WAVES * KNN_MAX_K * sizeof(KnnCand));
    static_assert(lds_max <= 160 * 1024, "the queries and the waves' lists fit the CU's LDS");
    const size_t lds = (size_t)QB * 16 * (FIRA_D * sizeof(float) + (size_t)KNN_WAVES * K * sizeof(KnnCand));
    if (lds_max > 64 * 1024)
        if (int e = raise_dynamic_lds<knn_search_kernel<QB>>(lds_max, "fira_knn_search")) return e;
    hipLaunchKernelGGL(knn_search_kernel<QB>, dim3(G, YB), dim3(KNN_NT), lds, s, Q, R, keys, key_sq, owner, exclude, N, K, part);
    return 0;
}

// ---------------------------------------------------------------- mix
struct KnnSlots {
    int word[KNN_MAX_K];                                                 // -1: void
    float add[KNN_MAX_K];                                                // fl(lam * w_k)
};

__device__ __forceinline__ float knn_elem(float a, float p, int i, const KnnSlots& sl) {
#pragma clang fp contract(off)
    float y = a * p;
#pragma unroll
    for (int k = 0; k < KNN_MAX_K; ++k)                          // (a void slot's word is -1: no entry)
        if (sl.word[k] == i) y = y + sl.add[k];
    return y;
}

__global__ __launch_bounds__(DDW_NT) void mix_knn_kernel(int W, const int32_t* __restrict__ idx, const float* __restrict__ d2,
                                                         const int32_t* __restrict__ values, int N, int K,
                                                         const float* __restrict__ coef, float* dist,
                                                         int32_t* __restrict__ best_id, float* __restrict__ best_p) {
#pragma clang fp contract(off)
    __shared__ float smf[DDW_NT / 64];
    __shared__ int smi[DDW_NT / 64];
    const int r = blockIdx.x, tid = threadIdx.x;
    const float lam = coef[0], inv_T = coef[1];
    float* prow = dist + (size_t)r * W;
    const int32_t* ir = idx + (size_t)r * K;
    const float* dr = d2 + (size_t)r * K;

    // the slots: thread k forms slot k's word and exponential, thread 0 the sum in ascending k, then every thread takes the
    // K words and additions from LDS
    __shared__ int s_word[KNN_MAX_K];
    __shared__ float s_add[KNN_MAX_K];
    __shared__ int s_some;
    if (tid < KNN_MAX_K) {
        int word = -1;
        float ex = 0.f;
        if (tid < K) {
            const int j = ir[tid];
            if (j >= 0 && j < N) {
                word = values[j];
                const float x = (dr[tid] - dr[0]) * inv_T;
                ex = expf(-x);
            }
        }
        s_word[tid] = word;
        s_add[tid] = ex;
    }
    __syncthreads();
    if (tid == 0) {
        float sum = 0.f;
        bool some = false;
        for (int k = 0; k < KNN_MAX_K; ++k)
            if (s_word[k] >= 0) { sum = sum + s_add[k]; some = true; }
        for (int k = 0; k < KNN_MAX_K; ++k) {
            const float w = s_add[k] / sum;
            s_add[k] = s_word[k] >= 0 ? lam * w : 0.f;
        }
        s_some = some;
    }
    __syncthreads();
    KnnSlots sl;
#pragma unroll
    for (int k = 0; k < KNN_MAX_K; ++k) { sl.word[k] = s_word[k]; sl.add[k] = s_add[k]; }
    const bool edit = s_some != 0 && lam != 0.f;               // (workgroup-uniform)
    const float a = 1.0f - lam;

    const RowSplit c(prow, W);
    const int head = c.head, nvec = c.nvec;
    ArgMax best;
    auto scalar = [&](int i) {
        float y = prow[i];
        if (edit) {
            y = knn_elem(a, y, i, sl);
            prow[i] = y;
        }
        best.offer(y, i);
    };
    if (tid < head) scalar(tid);
    if (tid >= DDW_NT - 4 && c.tail_of(tid) < W) scalar(c.tail_of(tid));

    for (int v0 = tid; v0 < nvec; v0 += 2 * DDW_NT) {
        float4 x[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int i = head + 4 * min(v0 + u * DDW_NT, nvec - 1);           // (clamped: requested, not used, past the end)
            x[u] = *reinterpret_cast<const float4*>(prow + i);
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int v = v0 + u * DDW_NT;
            if (v < nvec) {
                const int i = head + 4 * v;
                float4 y = x[u];
                if (edit) {
                    y = make_float4(knn_elem(a, x[u].x, i, sl), knn_elem(a, x[u].y, i + 1, sl),
                                    knn_elem(a, x[u].z, i + 2, sl), knn_elem(a, x[u].w, i + 3, sl));
                    *reinterpret_cast<float4*>(prow + i) = y;
                }
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

static bool knn_shape_ok(int R, int N, int K) { return R >= 0 && N > 0 && N <= KNN_MAX_N && K >= 1 && K <= KNN_MAX_K; }

}  // namespace fira

extern "C" size_t fira_knn_search_scratch_bytes(int R, int N, int K) {
    using namespace fira;
    if (!knn_shape_ok(R, N, K) || R == 0) return 0;
    const size_t yb = ((size_t)R + KNN_QBLOCK - 1) / KNN_QBLOCK;
    return yb * knn_grid(N) * KNN_QBLOCK * K * sizeof(KnnCand);
}

extern "C" int fira_knn_search(void* stream, const float* Q, int R, const float* keys, const float* key_sq, const int32_t* owner,
                               const int32_t* exclude, int N, int K, int32_t* idx_out, float* d2_out, void* scratch,
                               size_t scratch_bytes) {
    using namespace fira;
    FIRA_REQUIRE(R >= 0, "fira_knn_search: R = %d is negative", R);
    FIRA_REQUIRE(N > 0, "fira_knn_search: N = %d, the store is empty", N);
    FIRA_REQUIRE(N <= KNN_MAX_N, "fira_knn_search: N = %d rows, more than %d", N, KNN_MAX_N);
    FIRA_REQUIRE(K >= 1 && K <= KNN_MAX_K, "fira_knn_search: K = %d outside 1..%d", K, KNN_MAX_K);
    FIRA_REQUIRE((long long)R * K <= INT_MAX, "fira_knn_search: R = %d queries with K = %d, too many slots", R, K);
    FIRA_REQUIRE(!(exclude && !owner), "fira_knn_search: exclude without owner (there is nothing to hold it against)");
    if (R == 0) return 0;
    FIRA_REQUIRE(Q && keys && key_sq && idx_out && d2_out && scratch,
                 "fira_knn_search: null pointer (Q, keys, key_sq, idx_out, d2_out or scratch)");
    FIRA_REQUIRE(((uintptr_t)Q & 15u) == 0 && ((uintptr_t)keys & 15u) == 0, "fira_knn_search: Q and keys must be 16-byte aligned");
    const size_t need = fira_knn_search_scratch_bytes(R, N, K);
    FIRA_REQUIRE(scratch_bytes >= need, "fira_knn_search: scratch of %zu bytes, %zu needed", scratch_bytes, need);
    FIRA_REQUIRE(((uintptr_t)scratch & 7u) == 0, "fira_knn_search: scratch must be 8-byte aligned");
    const hipStream_t s = (hipStream_t)stream;
    const int G = knn_grid(N), YB = (R + KNN_QBLOCK - 1) / KNN_QBLOCK;
    KnnCand* part = (KnnCand*)scratch;
    int e = 0;
    switch ((min(R, KNN_QBLOCK) + 15) / 16) {
        case 1: e = knn_launch<1>(s, G, YB, Q, R, keys, key_sq, owner, exclude, N, K, part); break;
        case 2: e = knn_launch<2>(s, G, YB, Q, R, keys, key_sq, owner, exclude, N, K, part); break;
        case 3: e = knn_launch<3>(s, G, YB, Q, R, keys, key_sq, owner, exclude, N, K, part); break;
        default: e = knn_launch<4>(s, G, YB, Q, R, keys, key_sq, owner, exclude, N, K, part); break;
    }
    if (e) return e;
    FIRA_CHECK_LAUNCH("fira_knn_search");
    hipLaunchKernelGGL(knn_merge_kernel, dim3(R), dim3(KNN_MERGE_NT), 0, s, part, G, K, Q, idx_out, d2_out);
    FIRA_CHECK_LAUNCH("fira_knn_search (merge)");
    return 0;
}

extern "C" int fira_mix_knn(void* stream, const fira_dims* d, int R, const int32_t* idx, const float* d2, const int32_t* values,
                            int N, int K, const float* coef, float* dist, int32_t* best_id, float* best_p) {
    using namespace fira;
    if (int e = require_row_geometry(d, 1, R, best_id, best_p, "fira_mix_knn")) return e;
    FIRA_REQUIRE(N > 0 && N <= KNN_MAX_N, "fira_mix_knn: N = %d outside 1..%d", N, KNN_MAX_N);
    FIRA_REQUIRE(K >= 1 && K <= KNN_MAX_K, "fira_mix_knn: K = %d outside 1..%d", K, KNN_MAX_K);
    if (R == 0) return 0;
    FIRA_REQUIRE(idx && d2 && values && coef && dist, "fira_mix_knn: null pointer (idx, d2, values, coef or dist)");
    FIRA_REQUIRE(((uintptr_t)dist & 3u) == 0, "fira_mix_knn: dist must be 4-byte aligned");
    const int W = d->vocab + d->sou_len + d->sub_len;
    hipLaunchKernelGGL(mix_knn_kernel, dim3(R), dim3(DDW_NT), 0, (hipStream_t)stream, W, idx, d2, values, N, K, coef, dist, best_id,
                       best_p);
    FIRA_CHECK_LAUNCH("fira_mix_knn");
    return 0;
}
