// Block-wide reductions of the 1024-thread decode-row kernels: decode_dist_wide_kernel (copyhead.hip) and
// sample_dist_kernel (sample.hip).  Both kernels form the same distribution row with these helpers, so the values they
// write are bit-identical.  Every thread returns the same result: the 16 wave partials are summed in one fixed order.
#pragma once
#include "common.h"

namespace fira {

constexpr int DDW_NT = 1024, DDW_NPT = 25;
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

}  // namespace fira
