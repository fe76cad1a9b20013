// float4 arithmetic and the small index / gradient helpers of the element-wise (HBM-bound, fp32) kernels: one definition of each.
#pragma once

#include <hip/hip_runtime.h>

namespace emd {

__device__ __forceinline__ float4 f4zero() { return make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ __forceinline__ float4 fma4(float4 a, float4 b, float4 c) {
    return make_float4(fmaf(a.x, b.x, c.x), fmaf(a.y, b.y, c.y), fmaf(a.z, b.z, c.z), fmaf(a.w, b.w, c.w));
}
__device__ __forceinline__ float4 fma4s(float4 a, float s, float4 c) {
    return make_float4(fmaf(a.x, s, c.x), fmaf(a.y, s, c.y), fmaf(a.z, s, c.z), fmaf(a.w, s, c.w));
}
__device__ __forceinline__ float4 add4(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ __forceinline__ float4 relu4(float4 a) { return make_float4(fmaxf(a.x, 0.f), fmaxf(a.y, 0.f), fmaxf(a.z, 0.f), fmaxf(a.w, 0.f)); }
// relu (hi = +inf) or relu6 (hi = 6), in the order affine_relu6_kernel (dw_misc.hip) applies them: the PRE forms produce its bits
__device__ __forceinline__ float4 clamp4(float4 a, float hi) {
    return make_float4(fminf(fmaxf(a.x, 0.f), hi), fminf(fmaxf(a.y, 0.f), hi), fminf(fmaxf(a.z, 0.f), hi), fminf(fmaxf(a.w, 0.f), hi));
}

// dy masked by the activation that followed, z = the activation's input
__device__ __forceinline__ float grad_mask(float dy, float z, int mask) {
    if (mask == 1) return (z > 0.f && z < 6.f) ? dy : 0.f;   // tf.nn.relu6 (Relu6Grad: 0 < z < 6)
    if (mask == 2) return (z > 0.f && z <= 1.f) ? dy : 0.f;  // relu6 then tf.clip_by_value(., 0, 1) (passes on [0,1])
    if (mask == 3) return z > 0.f ? dy : 0.2f * dy;           // tf.nn.leaky_relu, alpha 0.2 (graph G)
    if (mask == 4) return z > 0.f ? dy : 0.f;                 // tf.nn.relu (ReluGrad: z > 0; graph S)
    return dy;
}

// tf.pad(mode="REFLECT"): index -1 -> 1, n -> n-2 (the border sample is not repeated)
__device__ __forceinline__ int reflect(int i, int n) {
    i = i < 0 ? -i : i;
    return i >= n ? 2 * n - 2 - i : i;
}

}  // namespace emd
