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

// tf.image.resize_images (bilinear, align_corners = False, legacy sampling src = dst * (in / out)): the one copy of its index arithmetic
// and of its interpolation step.  resize_bilinear_kernel (dw_misc.hip) and the kernels that form an upsampled tensor in registers instead
// of reading it (dw3x3_s1_roll_up, gemm_conv_kernel's UP epilogue) call these, x first inside a source row and then y: the same bits.
// The fused multiply-adds are written out: the compiler formed them in resize_bilinear_kernel from `f - i0` and `a + (b - a) * l`
// (the weight is o * s - i0 with the product unrounded; the index is the floor of the rounded product), and whether it forms them
// must not depend on the kernel the expression is inlined into.
__device__ __forceinline__ void resize_src(int o, float s, int n_in, int& i0, int& i1, float& l) {
    const float f = (float)o * s;
    i0 = (int)floorf(f);
    i1 = min(i0 + 1, n_in - 1);
    l = fmaf(s, (float)o, -(float)i0);
}
__device__ __forceinline__ float lerpf(float a, float b, float l) { return fmaf(l, b - a, a); }
__device__ __forceinline__ float4 lerp4(float4 a, float4 b, float l) {
    return make_float4(lerpf(a.x, b.x, l), lerpf(a.y, b.y, l), lerpf(a.z, b.z, l), lerpf(a.w, b.w, l));
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
