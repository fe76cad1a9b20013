// Graph S training (see include/emdenoise.h, emd_s_head_bwd_f32 / emd_s_mse_loss_f32 / emd_relu_mask_bwd_f32).
//
// The reference's loss (misc_py/autoencoder.py:177-188) is tf.losses.mean_squared_error(imgs, outputs): L = sum (out - x)^2 / N over
// the B*H*W pixels, the target being the input crop itself.  The last two layers of the apply graph (apply_autoencoders.py:160-184)
// are  a = relu(conv2d_transpose(.) + bias)  [B,H,W,64]  and  out = conv2d(a, w, 3x3 SAME, no bias)  [B,H,W,1].  Their reverse pass:
//   dout = 2 (out - x) / N                                  (formed in registers, never written)
//   dW[t][c]  = sum_q a[q][c] dout[q - off_t]               (off_t = (ky-1, kx-1); dout is zero outside the image)
//   da[q][c]  = [a[q][c] > 0] sum_t dout[q - off_t] w[t][c] (ReluGrad; written once, may overwrite a)
//   dbias[c]  = sum_q da[q][c]                              (the transposed conv's bias)
// s_head_bwd_kernel: one workgroup per 8 x 32 tile of one image.  dout of the tile and its one-pixel halo goes to LDS; every thread
// owns one channel quad and walks the tile's pixels, reading a once and writing da once, and keeps its nine weight-gradient and one
// bias sums in registers.  They are reduced over the workgroup's pixel lanes in a fixed order into a per-workgroup slab (with the
// tile's sum of (out - x)^2); s_head_reduce1/2_kernel sum the slabs in a fixed order in double, in two levels.  No atomics: the same inputs give the
// same bits.
#include "emd_common.hpp"
#include "f4_math.hpp"

namespace {

using namespace emd;

constexpr int kTH = 8, kTW = 32, kThreads = 256;
constexpr int kHaloW = kTW + 2, kHalo = (kTH + 2) * kHaloW;

// slab of one workgroup: [9][C] weight-gradient sums, [C] bias sums, then the sum of (out - x)^2; stride slab_stride(C) floats
__host__ __device__ inline int slab_stride(int C) { return 10 * C + 4; }

template <int CG>
__global__ __launch_bounds__(kThreads) void s_head_bwd_kernel(const float* __restrict__ out, const float* __restrict__ x,
                                                              const float* a, int lda, const float* __restrict__ w9, float* da, int ldo,
                                                              int H, int W, float gscale, float* __restrict__ slabs) {
    constexpr int PL = kThreads / CG;   // pixel lanes
    constexpr int C = 4 * CG;
    __shared__ float e_s[kHalo];
    __shared__ float4 red[kThreads];
    __shared__ double red_d[kThreads / 64];
    const int tid = threadIdx.x, cg = tid % CG, pl = tid / CG;
    const int b = blockIdx.z, y0 = blockIdx.y * kTH, x0 = blockIdx.x * kTW;
    const long img = (long)b * H * W;

    // dout over the tile and its halo; the tile's own pixels give the loss partial
    float sq = 0.f;
    for (int k = tid; k < kHalo; k += kThreads) {
        const int i = k / kHaloW, j = k - i * kHaloW;
        const int gy = y0 + i - 1, gx = x0 + j - 1;
        float e = 0.f;
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
            const long p = img + (long)gy * W + gx;
            e = out[p] - x[p];
            if (i >= 1 && i <= kTH && j >= 1 && j <= kTW) sq = fmaf(e, e, sq);
        }
        e_s[k] = gscale * e;
    }
    float4 w[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) w[t] = *reinterpret_cast<const float4*>(w9 + t * C + 4 * cg);
    __syncthreads();

    float4 acc[9], accb = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int t = 0; t < 9; ++t) acc[t] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int p = pl; p < kTH * kTW; p += PL) {
        const int i = p / kTW, j = p - i * kTW;
        const int gy = y0 + i, gx = x0 + j;
        if (gy >= H || gx >= W) continue;
        const long q = img + (long)gy * W + gx;
        const float4 av = *reinterpret_cast<const float4*>(a + q * lda + 4 * cg);
        float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const float g = e_s[(i + 2 - ky) * kHaloW + (j + 2 - kx)];   // dout[q - (ky-1, kx-1)]
                s = fma4s(w[ky * 3 + kx], g, s);
                acc[ky * 3 + kx] = fma4s(av, g, acc[ky * 3 + kx]);
            }
        const float4 d = make_float4(av.x > 0.f ? s.x : 0.f, av.y > 0.f ? s.y : 0.f, av.z > 0.f ? s.z : 0.f, av.w > 0.f ? s.w : 0.f);
        accb = add4(accb, d);
        *reinterpret_cast<float4*>(da + q * ldo + 4 * cg) = d;
    }

    float* slab = slabs + ((long)(blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * slab_stride(C);
#pragma unroll
    for (int t = 0; t < 10; ++t) {
        red[tid] = t < 9 ? acc[t] : accb;
        __syncthreads();
        if (pl == 0) {
            float4 s = red[cg];
            for (int l = 1; l < PL; ++l) s = add4(s, red[l * CG + cg]);
            *reinterpret_cast<float4*>(slab + t * C + 4 * cg) = s;
        }
        __syncthreads();
    }
    double sd = (double)sq;
#pragma unroll
    for (int o = 32; o; o >>= 1) sd += __shfl_xor(sd, o);
    if ((tid & 63) == 0) red_d[tid >> 6] = sd;
    __syncthreads();
    if (tid == 0) {
        double s = 0.0;
        for (int k = 0; k < kThreads / 64; ++k) s += red_d[k];
        slab[10 * C] = (float)s;
    }
}

// Two-level fixed-order reduce of the slabs (deterministic).  Stage 1: workgroup (column block, chunk) = 32 columns x 8 slab lanes
// over the chunk's slabs -> one double per (chunk, column).  Stage 2: the chunks of every column in order; columns [0, 9C) += into
// dw9, [9C, 10C) += into dbias (if given), column 10C / n -> loss_out.
__global__ __launch_bounds__(kThreads) void s_head_reduce1_kernel(const float* __restrict__ slabs, int nslab, int per_chunk, int C,
                                                                  double* __restrict__ part_out) {
    __shared__ double part[8][32];
    const int col_l = threadIdx.x & 31, lane = threadIdx.x >> 5;
    const int col = blockIdx.x * 32 + col_l, ncol = 10 * C + 1, stride = slab_stride(C);
    const int k0 = blockIdx.y * per_chunk, k1 = min(nslab, k0 + per_chunk);
    double s = 0.0;
    if (col < ncol)
        for (int k = k0 + lane; k < k1; k += 8) s += (double)slabs[(long)k * stride + col];
    part[lane][col_l] = s;
    __syncthreads();
    if (lane == 0 && col < ncol) {
        double t = part[0][col_l];
        for (int l = 1; l < 8; ++l) t += part[l][col_l];
        part_out[(long)blockIdx.y * ncol + col] = t;
    }
}

__global__ __launch_bounds__(kThreads) void s_head_reduce2_kernel(const double* __restrict__ part, int nchunk, int C, long n,
                                                                  float* __restrict__ dw9, float* __restrict__ dbias,
                                                                  float* __restrict__ loss_out) {
    const int col = blockIdx.x * kThreads + threadIdx.x, ncol = 10 * C + 1;
    if (col >= ncol) return;
    double t = 0.0;
    for (int k = 0; k < nchunk; ++k) t += part[(long)k * ncol + col];
    if (col < 9 * C)
        dw9[col] += (float)t;
    else if (col < 10 * C) {
        if (dbias) dbias[col - 9 * C] += (float)t;
    } else if (loss_out)
        loss_out[0] = (float)(t / (double)n);
}

// the composed route's loss: per-block double sums of (out - x)^2, then one final block; dout = gscale (out - x)
__global__ __launch_bounds__(kThreads) void s_sqdiff_kernel(const float* __restrict__ out, const float* __restrict__ x, long n, float gscale,
                                                            float* __restrict__ dout, double* __restrict__ part) {
    __shared__ double red_d[kThreads / 64];
    double s = 0.0;
    for (long i = (long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long)gridDim.x * kThreads) {
        const float e = out[i] - x[i];
        s += (double)(e * e);
        if (dout) dout[i] = gscale * e;
    }
#pragma unroll
    for (int o = 32; o; o >>= 1) s += __shfl_xor(s, o);
    if ((threadIdx.x & 63) == 0) red_d[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int k = 0; k < kThreads / 64; ++k) t += red_d[k];
        part[blockIdx.x] = t;
    }
}

__global__ void s_sqdiff_final(const double* __restrict__ part, int nblk, long n, float* __restrict__ loss_out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double s = 0.0;
    for (int k = 0; k < nblk; ++k) s += part[k];
    loss_out[0] = (float)(s / (double)n);
}

// dr = [a > 0] g, float4 over the flat [npix][C] tensors (pitches C)
__global__ __launch_bounds__(kThreads) void relu_mask_bwd_kernel(const float4* __restrict__ a, const float4* g, float4* dr, long n4) {
    const long i = (long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n4) return;
    const float4 av = a[i], gv = g[i];
    dr[i] = make_float4(av.x > 0.f ? gv.x : 0.f, av.y > 0.f ? gv.y : 0.f, av.z > 0.f ? gv.z : 0.f, av.w > 0.f ? gv.w : 0.f);
}

template <int CG>
void launch_head(dim3 grid, hipStream_t st, const float* out, const float* x, const float* a, int lda, const float* w9, float* da, int ldo,
                 int H, int W, float gscale, float* slabs) {
    hipLaunchKernelGGL(s_head_bwd_kernel<CG>, grid, dim3(kThreads), 0, st, out, x, a, lda, w9, da, ldo, H, W, gscale, slabs);
}

long head_slabs(int B, int H, int W) { return (long)B * ((H + kTH - 1) / kTH) * ((W + kTW - 1) / kTW); }
constexpr long kSlabsPerChunk = 64;
long head_chunks(long nslab) { return (nslab + kSlabsPerChunk - 1) / kSlabsPerChunk; }
size_t head_slab_bytes(int B, int H, int W, int C) { return ((size_t)head_slabs(B, H, W) * slab_stride(C) * sizeof(float) + 15) & ~(size_t)15; }

}  // namespace

extern "C" size_t emd_s_head_bwd_workspace_bytes(int B, int H, int W, int C) {
    if (B < 1 || H < 1 || W < 1 || C < 4) return 0;
    return head_slab_bytes(B, H, W, C) + (size_t)head_chunks(head_slabs(B, H, W)) * (10 * C + 1) * sizeof(double);
}

extern "C" int emd_s_head_bwd_f32(const float* out, const float* x, const float* a, int lda, const float* w9, int B, int H, int W, int C,
                                  float* da, int ldo, float* dw9, float* dbias, float* loss_out, void* workspace, size_t workspace_bytes,
                                  emd_stream_t stream) {
    EMD_REQUIRE(out && x && a && w9 && da && dw9 && workspace, EMD_E_INVALID, "emd_s_head_bwd_f32: null pointer");
    EMD_REQUIRE(B >= 1 && B <= 65535 && H >= 1 && W >= 1 && (H + kTH - 1) / kTH <= 65535, EMD_E_INVALID, "emd_s_head_bwd_f32: bad shape");
    EMD_REQUIRE(C == 4 || C == 8 || C == 16 || C == 32 || C == 64 || C == 128 || C == 256, EMD_E_UNSUPPORTED,
                "emd_s_head_bwd_f32: C must be a power of two, 4..256");
    EMD_REQUIRE(lda % 4 == 0 && ldo % 4 == 0 && lda >= C && ldo >= C && emd::aligned16(a) && emd::aligned16(da) && emd::aligned16(w9),
                EMD_E_ALIGN, "emd_s_head_bwd_f32: pitches multiples of 4 and >= C, 16-byte aligned a / da / w9");
    EMD_REQUIRE(da == a ? ldo == lda : true, EMD_E_INVALID, "emd_s_head_bwd_f32: in place needs ldo == lda");
    EMD_REQUIRE(workspace_bytes >= emd_s_head_bwd_workspace_bytes(B, H, W, C), EMD_E_INVALID, "emd_s_head_bwd_f32: workspace too small");
    EMD_REQUIRE(head_slabs(B, H, W) <= 0x7fffffffL && head_chunks(head_slabs(B, H, W)) <= 65535, EMD_E_UNSUPPORTED,
                "emd_s_head_bwd_f32: too many tiles");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const long n = (long)B * H * W;
    const float gscale = (float)(2.0 / (double)n);
    const dim3 grid((W + kTW - 1) / kTW, (H + kTH - 1) / kTH, B);
    float* slabs = static_cast<float*>(workspace);
    switch (C / 4) {
        case 1: launch_head<1>(grid, st, out, x, a, lda, w9, da, ldo, H, W, gscale, slabs); break;
        case 2: launch_head<2>(grid, st, out, x, a, lda, w9, da, ldo, H, W, gscale, slabs); break;
        case 4: launch_head<4>(grid, st, out, x, a, lda, w9, da, ldo, H, W, gscale, slabs); break;
        case 8: launch_head<8>(grid, st, out, x, a, lda, w9, da, ldo, H, W, gscale, slabs); break;
        case 16: launch_head<16>(grid, st, out, x, a, lda, w9, da, ldo, H, W, gscale, slabs); break;
        case 32: launch_head<32>(grid, st, out, x, a, lda, w9, da, ldo, H, W, gscale, slabs); break;
        default: launch_head<64>(grid, st, out, x, a, lda, w9, da, ldo, H, W, gscale, slabs); break;
    }
    const int ncol = 10 * C + 1;
    const long nslab = head_slabs(B, H, W), nchunk = head_chunks(nslab);
    double* part = reinterpret_cast<double*>(static_cast<char*>(workspace) + head_slab_bytes(B, H, W, C));
    hipLaunchKernelGGL(s_head_reduce1_kernel, dim3((ncol + 31) / 32, (unsigned)nchunk), dim3(kThreads), 0, st, slabs, (int)nslab,
                       (int)kSlabsPerChunk, C, part);
    hipLaunchKernelGGL(s_head_reduce2_kernel, dim3((ncol + kThreads - 1) / kThreads), dim3(kThreads), 0, st, part, (int)nchunk, C, n, dw9,
                       dbias, loss_out);
    return emd::check_launch("s_head_bwd_kernel");
}

extern "C" size_t emd_s_mse_loss_workspace_bytes(void) { return 1024 * sizeof(double); }

extern "C" int emd_s_mse_loss_f32(const float* out, const float* x, long n, float* loss_out, float* dout, void* workspace,
                                  emd_stream_t stream) {
    EMD_REQUIRE(out && x && loss_out && workspace, EMD_E_INVALID, "emd_s_mse_loss_f32: null pointer");
    EMD_REQUIRE(n >= 1, EMD_E_INVALID, "emd_s_mse_loss_f32: empty input");
    hipStream_t st = static_cast<hipStream_t>(stream);
    long nblk = (n + kThreads * 16 - 1) / (kThreads * 16);
    if (nblk > 1024) nblk = 1024;
    double* part = static_cast<double*>(workspace);
    hipLaunchKernelGGL(s_sqdiff_kernel, dim3((unsigned)nblk), dim3(kThreads), 0, st, out, x, n, (float)(2.0 / (double)n), dout, part);
    hipLaunchKernelGGL(s_sqdiff_final, dim3(1), dim3(64), 0, st, part, (int)nblk, n, loss_out);
    return emd::check_launch("s_mse_loss");
}

extern "C" int emd_relu_mask_bwd_f32(const float* a, const float* g, float* dr, long n, emd_stream_t stream) {
    EMD_REQUIRE(a && g && dr, EMD_E_INVALID, "emd_relu_mask_bwd_f32: null pointer");
    EMD_REQUIRE(n >= 0 && n % 4 == 0 && emd::aligned16(a) && emd::aligned16(g) && emd::aligned16(dr), EMD_E_ALIGN,
                "emd_relu_mask_bwd_f32: n a multiple of 4, 16-byte aligned tensors");
    if (n == 0) return EMD_OK;
    const long n4 = n / 4, nb = (n4 + kThreads - 1) / kThreads;
    EMD_REQUIRE(nb <= 0x7fffffffL, EMD_E_UNSUPPORTED, "emd_relu_mask_bwd_f32: too large");
    hipLaunchKernelGGL(relu_mask_bwd_kernel, dim3((unsigned)nb), dim3(kThreads), 0, static_cast<hipStream_t>(stream),
                       reinterpret_cast<const float4*>(a), reinterpret_cast<const float4*>(g), reinterpret_cast<float4*>(dr), n4);
    return emd::check_launch("relu_mask_bwd_kernel");
}
