// Reductions over the 64 lanes of a wave as xor-shuffle butterflies: every lane ends up with the result, and the order of the
// additions is fixed (the same inputs give the same bits).  One definition of each.
#pragma once

#include <hip/hip_runtime.h>

namespace emd {

template <typename T>   // float, double
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v = fminf(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ int wave_or(int v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v |= __shfl_xor(v, o);
    return v;
}

}  // namespace emd
