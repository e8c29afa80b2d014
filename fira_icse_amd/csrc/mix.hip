// Ensemble decoding: the step distributions of several models mixed into one.
//
// fira_mix_dist forms out [R, W] from the members' dists[m] [R, W] between the members' fira_decode_step calls and whatever the
// search does with a distribution next (fira_merge_dist, fira_constrain_dist, fira_beam_select / fira_greedy_advance).  For every
// element, in member order, every multiply and every add rounded to fp32 on its own:
//     acc = w[0] * p_0[i];   acc = acc + w[1] * p_1[i];   ...   out[i] = acc
// No fused multiply-add (the function body is compiled with contraction off and the products are separate statements: DESIGN.md
// section 7 records a bit-equality test lost to a contracted expression), no atomics, no tree: a loop of np.float32 operations
// is the reference, and every run and every graph replay gives the same bits.  Nothing is renormalised.
//
// The member pointers and the weights are HOST arrays, read at launch and passed in a by-value struct: a captured launch bakes
// them in.  The kernel is instantiated per member count, so the struct is indexed by constants only (scalar kernel-argument
// loads, no scratch) and the member loop is unrolled.
//
// One workgroup of 1024 threads per row.  The row is cut at the 16-byte boundaries of OUT (RowSplit, decode_row.h); the body
// is this kernel's own, because it reads M rows and stores: per 4-element group one 16-byte store, and one 16-byte load per
// member whose row has out's alignment phase (workgroup-uniform), four 4-byte loads otherwise.  Two groups per thread are in
// flight per trip (2 * n_members 16-byte loads).  out may be dists[0]: a thread stores only to elements it has read itself, after
// reading them.
// With best_id / best_p: every thread offers what it stores to an ArgMax (NaN never wins), which reports the arg-max of the row as
// stored.  Without them no reduction runs.
#include <math.h>
#include "decode_row.h"

namespace fira {

constexpr int MIX_MAX = 8;

struct MixArgs {
    const float* p[MIX_MAX];
    float w[MIX_MAX];
};

template <int M>
__device__ __forceinline__ float mix_elem(const MixArgs& a, const float (&x)[M]) {
#pragma clang fp contract(off)
    float acc = a.w[0] * x[0];
#pragma unroll
    for (int m = 1; m < M; ++m) {
        const float t = a.w[m] * x[m];
        acc = acc + t;
    }
    return acc;
}

template <int M>
__global__ __launch_bounds__(DDW_NT) void mix_dist_kernel(int W, MixArgs a, float* out, int32_t* __restrict__ best_id,
                                                          float* __restrict__ best_p) {
    __shared__ float smf[DDW_NT / 64];
    __shared__ int smi[DDW_NT / 64];
    const int r = blockIdx.x, tid = threadIdx.x;
    const size_t off = (size_t)r * W;
    float* orow = out + off;
    const RowSplit c(orow, W);
    const int head = c.head, nvec = c.nvec;
    const float* row[M];
    bool wide[M];
#pragma unroll
    for (int m = 0; m < M; ++m) {
        row[m] = a.p[m] + off;
        wide[m] = ((uintptr_t)(row[m] + head) & 15u) == 0;     // (workgroup-uniform)
    }

    ArgMax best;
    auto scalar = [&](int i) {
        float x[M];
#pragma unroll
        for (int m = 0; m < M; ++m) x[m] = row[m][i];
        const float y = mix_elem<M>(a, x);
        orow[i] = y;
        best.offer(y, i);
    };
    if (tid < head) scalar(tid);
    if (tid >= DDW_NT - 4 && c.tail_of(tid) < W) scalar(c.tail_of(tid));

    for (int v0 = tid; v0 < nvec; v0 += 2 * DDW_NT) {
        float4 x[2][M];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int i = head + 4 * min(v0 + u * DDW_NT, nvec - 1);           // (clamped: requested, not used, past the end)
#pragma unroll
            for (int m = 0; m < M; ++m) {
                const float* q = row[m] + i;
                if (wide[m]) x[u][m] = *reinterpret_cast<const float4*>(q);
                else x[u][m] = make_float4(q[0], q[1], q[2], q[3]);
            }
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int v = v0 + u * DDW_NT;
            if (v < nvec) {
                const int i = head + 4 * v;
                float ex[M], ey[M], ez[M], ew[M];
#pragma unroll
                for (int m = 0; m < M; ++m) { ex[m] = x[u][m].x; ey[m] = x[u][m].y; ez[m] = x[u][m].z; ew[m] = x[u][m].w; }
                const float4 y = make_float4(mix_elem<M>(a, ex), mix_elem<M>(a, ey), mix_elem<M>(a, ez), mix_elem<M>(a, ew));
                *reinterpret_cast<float4*>(orow + i) = y;
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

template <int M>
static void mix_launch(hipStream_t stream, int R, int W, const MixArgs& a, float* out, int32_t* best_id, float* best_p) {
    hipLaunchKernelGGL(mix_dist_kernel<M>, dim3(R), dim3(DDW_NT), 0, stream, W, a, out, best_id, best_p);
}

}  // namespace fira

extern "C" int fira_mix_dist(void* stream, int R, int W, int n_members, const float* const* dists, const float* weights,
                             float* out, int32_t* best_id, float* best_p) {
    using namespace fira;
    FIRA_REQUIRE(R >= 0, "fira_mix_dist: R = %d is negative", R);
    FIRA_REQUIRE(W >= 1, "fira_mix_dist: W = %d, a row has at least one element", W);
    FIRA_REQUIRE(n_members >= 2 && n_members <= MIX_MAX, "fira_mix_dist: n_members = %d outside 2..%d", n_members, MIX_MAX);
    FIRA_REQUIRE(dists && weights, "fira_mix_dist: null host array (dists or weights)");
    for (int m = 0; m < n_members; ++m)
        FIRA_REQUIRE(isfinite(weights[m]) && weights[m] >= 0.0f, "fira_mix_dist: weight %d = %g is negative or not finite", m,
                     (double)weights[m]);
    if (int e = require_best_pair(best_id, best_p, "fira_mix_dist")) return e;
    if (R == 0) return 0;
    FIRA_REQUIRE(out, "fira_mix_dist: null pointer (out)");
    const size_t n = (size_t)R * W;
    MixArgs a;
    for (int m = 0; m < MIX_MAX; ++m) {
        const int k = m < n_members ? m : 0;
        FIRA_REQUIRE(dists[k], "fira_mix_dist: null pointer (dists[%d])", k);
        a.p[m] = dists[k];
        a.w[m] = m < n_members ? weights[m] : 0.0f;
    }
    for (int m = 0; m < n_members; ++m) {
        if (m == 0 && dists[0] == out) continue;               // in place over member 0: the one aliasing the kernel allows
        FIRA_REQUIRE(dists[m] + n <= out || out + n <= dists[m], "fira_mix_dist: out overlaps dists[%d] (only out == dists[0] may alias)",
                     m);
    }
    const hipStream_t s = (hipStream_t)stream;
    switch (n_members) {
        case 2: mix_launch<2>(s, R, W, a, out, best_id, best_p); break;
        case 3: mix_launch<3>(s, R, W, a, out, best_id, best_p); break;
        case 4: mix_launch<4>(s, R, W, a, out, best_id, best_p); break;
        case 5: mix_launch<5>(s, R, W, a, out, best_id, best_p); break;
        case 6: mix_launch<6>(s, R, W, a, out, best_id, best_p); break;
        case 7: mix_launch<7>(s, R, W, a, out, best_id, best_p); break;
        default: mix_launch<8>(s, R, W, a, out, best_id, best_p); break;
    }
    FIRA_CHECK_LAUNCH("fira_mix_dist");
    return 0;
}
