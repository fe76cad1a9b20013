// Inclusive prefix sums over the 64 lanes of a wave by shuffles, and over the 256 threads of a workgroup through LDS.  Integers only:
// the additions are associative, so the result does not depend on the order.  One definition of each (dose.hip).
#pragma once

#include <hip/hip_runtime.h>

namespace emd {

// lane l ends up with v[0] + ... + v[l]
__device__ __forceinline__ unsigned long long wave_inclusive_scan(unsigned long long v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long u = __shfl_up(v, o, 64);
        if (lane >= o) v += u;
    }
    return v;
}

// One value per thread of a 256-thread workgroup -> the inclusive prefix sum over the threads; *total: the sum over the workgroup
// (every thread gets it).  sh: 4 words that no thread still reads from an earlier use (one barrier inside; a caller that alternates
// between two such arrays from call to call needs no barrier of its own).
__device__ __forceinline__ unsigned long long block_inclusive_scan(unsigned long long v, unsigned long long* sh,
                                                                   unsigned long long* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long s = wave_inclusive_scan(v);
    if (lane == 63) sh[wave] = s;
    __syncthreads();
    unsigned long long before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const unsigned long long t = sh[w];
        if (w < wave) before += t;
        all += t;
    }
    *total = all;
    return s + before;
}

}  // namespace emd
