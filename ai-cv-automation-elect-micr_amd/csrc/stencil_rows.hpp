// What the single-channel image operations share, one definition of each:
//   the window taps as a kernel argument, the vertical 1-D pass on a register ring    ssim.hip (the metrics), filters.hip (the
//                                                                                     classical filters)
//   wave_sum_lane0, block_sum_fixed: the fixed-order sums of doubles                  those two, wavelet.hip, harvest.hip, fft.hip
//   block_sum_thread0: one double per thread, behind a barrier of its own             harvest.hip, fft.hip
//   block_tree_sum: block_sum_fixed's tree over one double per thread                 fft.hip
// The host helpers they share (overlap, round256, tiles_of) are in emd_common.hpp, the median's selection in radix_select.hpp.
#pragma once

#include "emd_common.hpp"

namespace {

constexpr int kMaxSize = 15;   // widest window

struct Taps {
    float g[kMaxSize];
};

// Vertical 1-D pass over a strip of SH output rows of one column, without a second LDS buffer: hrow(i, v) yields the NC
// horizontally filtered values of strip row i (0 <= i < SH + S - 1); they go round a ring of S rows held in registers
// (the row loop is unrolled S times, so every ring index is a compile-time constant), and orow(o, v) receives output row o.
template <int S, int SH, int NC, class HFn, class OFn>
__device__ __forceinline__ void roll_rows(const Taps& taps, HFn&& hrow, OFn&& orow) {
    constexpr int NR = SH + S - 1;
    float ring[S][NC];
    for (int base = 0; base < NR; base += S) {
#pragma unroll
        for (int j = 0; j < S; ++j) {
            const int i = base + j;
            if (i < NR) {
                hrow(i, ring[j]);
                if (i >= S - 1) {
                    float v[NC];
#pragma unroll
                    for (int c = 0; c < NC; ++c) v[c] = 0.f;
#pragma unroll
                    for (int k = 0; k < S; ++k) {
#pragma unroll
                        for (int c = 0; c < NC; ++c) v[c] = fmaf(taps.g[k], ring[(j + 1 + k) % S][c], v[c]);
                    }
                    orow(i - (S - 1), v);
                }
            }
        }
    }
}

// Sum of one double per lane over the wave, in a fixed order; the result is valid in lane 0 only (emd::wave_sum is the butterfly).
__device__ __forceinline__ double wave_sum_lane0(double v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// Sum of one double per thread over the 256 threads of a workgroup: lanes, then the four waves, in a fixed order.  Valid in
// thread 0.  sh: 4 doubles, not otherwise in use between two calls' barriers.
__device__ __forceinline__ double block_sum_thread0(double v, double* sh) {
    v = wave_sum_lane0(v);
    __syncthreads();   // sh may still be read from the previous call
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

// Sum of one double per thread over the 256 threads of a workgroup as a binary tree in LDS, in a fixed order (every thread returns
// it).  sh: 256 doubles.
__device__ double block_tree_sum(double s, double* sh) {
    const int tid = threadIdx.x;
    __syncthreads();   // sh may still be read from the previous call
    sh[tid] = s;
    __syncthreads();
    for (int off = 128; off >= 1; off >>= 1) {
        if (tid < off) sh[tid] += sh[tid + off];
        __syncthreads();
    }
    return sh[0];
}

// Sum of p[0], p[stride], ..., p[(n - 1) * stride] by the 256 threads of a workgroup, in a fixed order (every thread returns it).
__device__ double block_sum_fixed(const double* __restrict__ p, int n, int stride, double* sh) {
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) s += p[(long)i * stride];
    return block_tree_sum(s, sh);
}

}  // namespace
