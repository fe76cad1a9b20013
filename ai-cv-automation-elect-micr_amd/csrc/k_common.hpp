// What the graph K training kernels share (k_train.hip: the unpaired step, sampler and fused form; k_pair.hip: the paired step
// and the pair maker): launch constants, theta's layout helpers, the per-tap device helpers, the block reductions and the
// reduce + Adam step.
#pragma once

#include <cmath>

#include "emd_common.hpp"
#include "f4_math.hpp"
#include "wave_reduce.hpp"

namespace {

using namespace emd;

constexpr float kLog2e = 1.4426950408889634f;
constexpr int kThreads = 256, kWaves = kThreads / 64, kPx = 4, kChunk = kThreads * kPx;
constexpr int kMaxNsym = (EMD_K_MAX_WIDTH / 2 + 1) * (EMD_K_MAX_WIDTH / 2 + 2) / 2;
constexpr int kMaxScal = (2 * EMD_K_MAX_DEPTH - 1) * kMaxNsym + EMD_K_MAX_DEPTH - 1;
constexpr int kMaxGrid = 1024;          // workgroups of k_grad_kernel (partial slabs)
constexpr int kUpdThreads = 1024;

inline int nsym_of(int width) { return (width / 2 + 1) * (width / 2 + 2) / 2; }
inline int nscal_of(int width, int depth) { return (2 * depth - 1) * nsym_of(width) + depth - 1; }

__device__ __forceinline__ float sigm(float z) {
    return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-kLog2e * z));
}

// class of tap (i, j) of a width-w map: the creation index of (max(|i-o|,|j-o|), min(..)) in make_layer's order
__device__ __forceinline__ int tap_class(int i, int j, int o) {
    const int a = abs(i - o), b = abs(j - o);
    const int hi = a > b ? a : b, lo = a > b ? b : a;
    return hi * (hi + 1) / 2 + lo;
}

// The reduce + Adam step shared by emd_k_train_step_f32 and emd_k_train_pair_step_f32 (one workgroup of kUpdThreads).  R threads
// per scalar share the partial slabs (strided), then a fixed-order tree in LDS.
// kSqrt = true adds the paired trainer's rule (noise_removal_kernels_duplicate.py:433): with sqrt_above_1 set and the mean squared
// error L > 1 the loss is sqrt(L) and every gradient is divided by 2 sqrt(L).  L exists only here, after the partials are summed,
// so the factor is applied here and the batch is never walked twice.  kSqrt = false is the unpaired arithmetic, unchanged.
template <bool kSqrt>
__device__ __forceinline__ void k_update_body(const float* __restrict__ partial, int nwg, int R, int width, int depth, long npix,
                                              float* __restrict__ theta, float* __restrict__ adam_m, float* __restrict__ adam_v,
                                              int* __restrict__ step, double lr0, long total_steps, float beta1, float beta2,
                                              float eps, int update, int sqrt_above_1, float* __restrict__ grad_out,
                                              float* __restrict__ loss_out, float* __restrict__ params_out) {
    __shared__ double red[kUpdThreads];
    __shared__ double sums[kMaxScal + 1];
    __shared__ float th[kMaxScal];
    const int tid = threadIdx.x;
    const int o = width >> 1, nsym = (o + 1) * (o + 2) / 2, ww = width * width;
    const int nscal = (2 * depth - 1) * nsym + depth - 1, n1 = nscal + 1;
    const int t = update ? step[0] + 1 : 0;   // 1-based step of this update
    const int per = kUpdThreads / R, part = tid % R;
    for (int base = 0; base < n1; base += per) {
        const int i = base + tid / R;
        double s = 0.0;
        if (i < n1)
            for (int w = part; w < nwg; w += R) s += (double)partial[(long)w * n1 + i];
        red[tid] = s;
        __syncthreads();
        for (int h = R >> 1; h; h >>= 1) {
            if (part < h) red[tid] += red[tid + h];
            __syncthreads();
        }
        if (part == 0 && i < n1) sums[i] = red[tid];
        __syncthreads();
    }
    // TF AdamOptimizer: lr_t = lr sqrt(1 - beta2^t) / (1 - beta1^t), lr the float32 placeholder value (:665-669)
    float lr_t = 0.f;
    if (update) {
        const float lr = (float)(lr0 * (1.0 - (double)t / (double)(total_steps + 1)));
        lr_t = (float)((double)lr * sqrt(1.0 - pow((double)beta2, (double)t)) / (1.0 - pow((double)beta1, (double)t)));
    }
    double root = 0.0;   // sqrt(L) where the sqrt rule applies, else 0
    if (kSqrt) {
        const double L = sums[nscal] / (double)npix;
        if (sqrt_above_1 && L > 1.0) root = sqrt(L);
    }
    for (int i = tid; i < n1; i += kUpdThreads) {
        if (i == nscal) {
            if (loss_out) loss_out[0] = kSqrt && root != 0.0 ? (float)root : (float)(sums[i] / (double)npix);
            continue;
        }
        const float g = kSqrt && root != 0.0 ? (float)(sums[i] / (double)npix / root) : (float)(sums[i] * 2.0 / (double)npix);
        if (grad_out) grad_out[i] = g;
        float p = theta[i];
        if (update) {   // adam_kernel's arithmetic (gan_train.hip)
            const float mi = beta1 * adam_m[i] + (1.f - beta1) * g;
            const float vi = beta2 * adam_v[i] + (1.f - beta2) * g * g;
            adam_m[i] = mi;
            adam_v[i] = vi;
            p -= lr_t * mi / (sqrtf(vi) + eps);
            theta[i] = p;
        }
        th[i] = p;
    }
    __syncthreads();
    if (params_out) {   // [wmaps D][w*w] | [bmaps D][w*w] (bmaps[0] = 0) | s [D] (s[0] = 1)
        const int offB = depth * nsym - nsym, offS = (2 * depth - 1) * nsym - 1;
        const int n = 2 * depth * ww + depth;
        for (int k = tid; k < n; k += kUpdThreads) {
            float val;
            if (k < 2 * depth * ww) {
                const int l = (k / ww) % depth, tap = k % ww;
                const int c = tap_class(tap / width, tap % width, o);
                if (k < depth * ww) val = th[l * nsym + c];
                else val = l ? th[offB + l * nsym + c] : 0.f;
            } else {
                const int l = k - 2 * depth * ww;
                val = l ? th[offS + l] : 1.f;
            }
            params_out[k] = val;
        }
    }
    if (update && tid == 0) step[0] = t;
}

// ---- block reductions of a kThreads workgroup (fixed order) and the integer draw
__device__ __forceinline__ float block_reduce_min(float v, float* sh) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v = fminf(v, __shfl_xor(v, o));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return fminf(fminf(sh[0], sh[1]), fminf(sh[2], sh[3]));
}
__device__ __forceinline__ float block_reduce_max(float v, float* sh) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return fmaxf(fmaxf(sh[0], sh[1]), fmaxf(sh[2], sh[3]));
}
__device__ __forceinline__ double block_reduce_sum(double v, double* sh) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

__device__ __forceinline__ unsigned draw_below(unsigned r, unsigned n) {   // floor(n * r / 2^32): 0 .. n-1
    return (unsigned)(((unsigned long long)r * n) >> 32);
}

}  // namespace
