// Graph K paired training (see include/emdenoise.h, emd_k_train_pair_step_f32 / emd_k_make_pairs_f32 / emd_s_crop_unscale_f32).
// replaces: misc_py/noise_removal_kernels_duplicate.py:406-434 (the filter over the UNPADDED patch, the interior target, the MSE
// and its sqrt rule), the gradient TensorFlow derives from it, :449 + :720-724 (Adam at beta1 = 0.5, lr = 0.01 (1 - t / 10001)),
// and misc_py/autoencoder_train-val-test.py:35-55 (the rescale of an autoencoder input / output pair and the 20 x 20 patch cut
// from both), with record_parser's finiteness rule (dup :534-548) applied where the pairs are made.
//
// k_pair_grad_kernel<D, kValid>  k_grad_kernel (k_train.hip) with a second tensor as the target.  kValid: the thread's pixel is
//   one of the (H-w+1) x (W-w+1) interior outputs, taps are read at (r + i, c + j) with no mirrored index, and the target is
//   truth[r + o][c + o].  !kValid: the REFLECT border of k_grad_kernel, output H x W, target truth[r][c].  The reference
//   assembles its output transposed (:425-428) and feeds the truth transposed (:735-736); the two cancel, so F(x) is compared
//   with truth in image orientation and there is no "reference" / "image" choice here.  Same chunking, same register / wave /
//   LDS summation order as k_grad_kernel: no atomics, bitwise reproducible.
// k_pair_update_kernel           k_update_body<true> (k_common.hpp): the fixed-order reduction, the sqrt rule, Adam, the packed block.
// k_make_pairs_kernel            one workgroup per image pair: (img - min) / (mean - min) for both, one Philox offset pair, the
//   patch of both, and 0.5 in both if either patch holds a non-finite value.
// s_crop_unscale_kernel          one workgroup per crop: Micrograph_Autoencoder.denoise_crop's inverse map, scale * pred + offset,
//   or pred * offset / mean(pred) for a flat crop.
#include <cmath>

#include "emd_common.hpp"
#include "k_common.hpp"
#include "philox.hpp"

namespace {

template <int D, bool kValid>
__global__ __launch_bounds__(kThreads) void k_pair_grad_kernel(const float* __restrict__ x, const float* __restrict__ truth, int B,
                                                               int H, int W, int width, int want_grad,
                                                               const float* __restrict__ theta, float* __restrict__ partial,
                                                               long nchunks) {
    __shared__ float th[kMaxScal];
    __shared__ float acc[kWaves][kMaxScal + 1];
    __shared__ unsigned char cls[EMD_K_MAX_WIDTH * EMD_K_MAX_WIDTH];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int o = width >> 1, ww = width * width;
    const int nsym = (o + 1) * (o + 2) / 2;
    const int nscal = (2 * D - 1) * nsym + D - 1;
    const int offB = D * nsym - nsym;           // b(l, c) = offB + l*nsym + c   (l >= 1)
    const int offS = (2 * D - 1) * nsym - 1;    // s(l)    = offS + l            (l >= 1)
    for (int i = tid; i < nscal; i += kThreads) th[i] = theta[i];
    for (int i = tid; i < kWaves * (kMaxScal + 1); i += kThreads) (&acc[0][0])[i] = 0.f;
    for (int k = tid; k < ww; k += kThreads) cls[k] = (unsigned char)tap_class(k / width, k % width, o);
    __syncthreads();

    // the compared pixels: Ho x Wo outputs per image, output (r, c) centred on input (r + ctr, c + ctr)
    const int Ho = kValid ? H - width + 1 : H, Wo = kValid ? W - width + 1 : W, ctr = kValid ? o : 0;
    const long HW = (long)H * W, HWo = (long)Ho * Wo, total = (long)B * HWo;
    float s_acc[D], loss_acc = 0.f;
#pragma unroll
    for (int l = 0; l < D; ++l) s_acc[l] = 0.f;

    // input element under tap (i, j) of output pixel (r, c): VALID rows r .. r + w - 1 are all inside the image
    auto tap_at = [&](int r, int c, int i, int j) -> long {
        if constexpr (kValid) return (long)(r + i) * W + (c + j);
        else return (long)reflect(r + i - o, H) * W + reflect(c + j - o, W);
    };

    for (long chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
        const float* img[kPx];
        int pr[kPx], pc[kPx];
        float e[kPx];
#pragma unroll
        for (int q = 0; q < kPx; ++q) {
            long idx = chunk * kChunk + q * kThreads + tid;
            const bool valid = idx < total;
            if (!valid) idx = 0;
            const long b = idx / HWo;
            const int rem = (int)(idx - b * HWo);
            pr[q] = rem / Wo;
            pc[q] = rem - pr[q] * Wo;
            img[q] = x + b * HW;
            const float tgt = truth[b * HW + (long)(pr[q] + ctr) * W + (pc[q] + ctr)];   // dup :431-432
            e[q] = valid ? -tgt : 0.f;   // becomes O - target below; invalid lanes keep zero residual
            if (!valid) pr[q] = -1;
        }
        // forward: O = sum over taps of the chain
        float out[kPx] = {};
        for (int i = 0; i < width; ++i) {
            for (int j = 0; j < width; ++j) {
                const int c = cls[i * width + j];
                float wl[D], bl[D], sl[D];
#pragma unroll
                for (int l = 0; l < D; ++l) {
                    wl[l] = th[l * nsym + c];
                    bl[l] = l ? th[offB + l * nsym + c] : 0.f;
                    sl[l] = l ? th[offS + l] : 1.f;
                }
#pragma unroll
                for (int q = 0; q < kPx; ++q) {
                    float f = wl[0] * img[q][tap_at(pr[q] < 0 ? 0 : pr[q], pc[q], i, j)];
#pragma unroll
                    for (int l = 1; l < D; ++l) f = wl[l] * (sl[l] * sigm(f + bl[l]));
                    out[q] += f;
                }
            }
        }
#pragma unroll
        for (int q = 0; q < kPx; ++q) {
            e[q] = pr[q] < 0 ? 0.f : out[q] + e[q];
            loss_acc = fmaf(e[q], e[q], loss_acc);
        }
        if (!want_grad) continue;
        // backward, per tap: dL/df_{D-1} = e (the factor 2/N, and 1 / (2 sqrt(L)) under the sqrt rule, is k_update_body's)
        for (int i = 0; i < width; ++i) {
            for (int j = 0; j < width; ++j) {
                const int c = cls[i * width + j];
                float wl[D], bl[D], sl[D], gw[D], gb[D];
#pragma unroll
                for (int l = 0; l < D; ++l) {
                    wl[l] = th[l * nsym + c];
                    bl[l] = l ? th[offB + l * nsym + c] : 0.f;
                    sl[l] = l ? th[offS + l] : 1.f;
                    gw[l] = 0.f;
                    gb[l] = 0.f;
                }
#pragma unroll
                for (int q = 0; q < kPx; ++q) {
                    const float v = img[q][tap_at(pr[q] < 0 ? 0 : pr[q], pc[q], i, j)];
                    float g[D];
                    float f = wl[0] * v;
#pragma unroll
                    for (int l = 1; l < D; ++l) {
                        g[l] = sigm(f + bl[l]);
                        f = wl[l] * (sl[l] * g[l]);
                    }
                    float d = e[q];
#pragma unroll
                    for (int l = D - 1; l >= 1; --l) {
                        const float sg = sl[l] * g[l];
                        gw[l] = fmaf(d, sg, gw[l]);
                        const float dw = d * wl[l];
                        s_acc[l] = fmaf(dw, g[l], s_acc[l]);
                        d = dw * sg * (1.f - g[l]);
                        gb[l] += d;
                    }
                    gw[0] = fmaf(d, v, gw[0]);
                }
#pragma unroll
                for (int l = 0; l < D; ++l) {
                    const float sw = wave_sum(gw[l]);
                    if (lane == 0) acc[wv][l * nsym + c] += sw;
                    if (l) {
                        const float sb = wave_sum(gb[l]);
                        if (lane == 0) acc[wv][offB + l * nsym + c] += sb;
                    }
                }
            }
        }
    }
#pragma unroll
    for (int l = 1; l < D; ++l) {
        const float v = wave_sum(s_acc[l]);
        if (lane == 0) acc[wv][offS + l] = v;
    }
    {
        const float v = wave_sum(loss_acc);
        if (lane == 0) acc[wv][nscal] = v;
    }
    __syncthreads();
    for (int i = tid; i <= nscal; i += kThreads)
        partial[(long)blockIdx.x * (nscal + 1) + i] = (acc[0][i] + acc[1][i]) + (acc[2][i] + acc[3][i]);
}

__global__ __launch_bounds__(kUpdThreads) void k_pair_update_kernel(const float* __restrict__ partial, int nwg, int R, int width,
                                                                    int depth, long npix, float* __restrict__ theta,
                                                                    float* __restrict__ adam_m, float* __restrict__ adam_v,
                                                                    int* __restrict__ step, double lr0, long total_steps,
                                                                    float beta1, float beta2, float eps, int update,
                                                                    int sqrt_above_1, float* __restrict__ grad_out,
                                                                    float* __restrict__ loss_out, float* __restrict__ params_out) {
    k_update_body<true>(partial, nwg, R, width, depth, npix, theta, adam_m, adam_v, step, lr0, total_steps, beta1, beta2, eps, update,
                        sqrt_above_1, grad_out, loss_out, params_out);
}

// ---- the pair maker (autoencoder_train-val-test.py:35-55), one workgroup per image pair
__device__ __forceinline__ int block_any(int v, int* sh) {
    __syncthreads();
    if (threadIdx.x == 0) *sh = 0;
    __syncthreads();
    if (v) *sh = 1;   // benign race: every writer stores 1
    __syncthreads();
    return *sh;
}

// (c, m) of one image: c = np.min (NaN when any pixel is), m = float32(mean accumulated in double) - c
__device__ __forceinline__ void min_mean_stats(const float* __restrict__ img, int np_, float* shf, double* shd, int* shi, float& c,
                                               float& m) {
    float mn = INFINITY;
    double s = 0.0;
    int nan = 0;
    for (int k = threadIdx.x; k < np_; k += kThreads) {
        const float v = img[k];
        mn = fminf(mn, v);
        s += (double)v;
        nan |= (v != v);
    }
    mn = block_reduce_min(mn, shf);
    s = block_reduce_sum(s, shd);
    c = block_any(nan, shi) ? NAN : mn;
    m = (float)(s / (double)np_) - c;
}

__global__ __launch_bounds__(kThreads) void k_make_pairs_kernel(const float* __restrict__ a, const float* __restrict__ b, int H,
                                                                int W, int patch, int lo, int hi, unsigned long long seed,
                                                                unsigned long long first_index, float* __restrict__ x,
                                                                float* __restrict__ t, int* __restrict__ draws) {
    __shared__ float shf[kWaves];
    __shared__ double shd[kWaves];
    __shared__ int shi;
    const int n = blockIdx.x, tid = threadIdx.x;
    const unsigned long long idx = first_index + (unsigned long long)n;
    const emd::U4 r = emd::philox4x32_10(emd::U4{(unsigned)idx, (unsigned)(idx >> 32), 0u, emd::kPhiloxTagKPair}, (unsigned)seed,
                                         (unsigned)(seed >> 32));
    const int i0 = lo + (int)draw_below(r.x, (unsigned)(hi - lo));   // np.random.randint(lo, hi): upper bound exclusive (:51-52)
    const int j0 = lo + (int)draw_below(r.y, (unsigned)(hi - lo));
    if (tid == 0 && draws) {
        draws[2 * n + 0] = i0;
        draws[2 * n + 1] = j0;
    }
    const long HW = (long)H * W;
    const float* ai = a + n * HW;
    const float* bi = b + n * HW;
    float ca, ma, cb, mb;
    min_mean_stats(ai, (int)HW, shf, shd, &shi, ca, ma);
    min_mean_stats(bi, (int)HW, shf, shd, &shi, cb, mb);
    const int pp = patch * patch;
    float* xo = x + (long)n * pp;
    float* to = t + (long)n * pp;
    int nonfinite = 0;
    for (int k = tid; k < pp; k += kThreads) {
        const int pi = k / patch, pj = k - pi * patch;
        const long src = (long)(i0 + pi) * W + (j0 + pj);
        const float va = (ai[src] - ca) / ma, vb = (bi[src] - cb) / mb;   // (img - c) / m in float32 (:38-44)
        xo[k] = va;
        to[k] = vb;
        nonfinite |= !(fabsf(va) <= 3.402823466e38f) | !(fabsf(vb) <= 3.402823466e38f);
    }
    if (block_any(nonfinite, &shi))   // dup record_parser (:544-546): both patches become 0.5; each thread rewrites what it wrote
        for (int k = tid; k < pp; k += kThreads) {
            xo[k] = 0.5f;
            to[k] = 0.5f;
        }
}

// ---- denoise_crop's inverse map (apply_autoencoders.py:376-381), one workgroup per crop
__global__ __launch_bounds__(kThreads) void s_crop_unscale_kernel(const float* __restrict__ pred, const float* __restrict__ cstats,
                                                                  int np_, float* __restrict__ out) {
    __shared__ double shd[kWaves];
    const int n = blockIdx.x, tid = threadIdx.x;
    const float off = cstats[2 * n], scale = cstats[2 * n + 1];
    const float* p = pred + (long)n * np_;
    float* o = out + (long)n * np_;
    if (scale != 0.f) {   // a NaN scale takes this branch, as `if scale:` does
        for (int k = tid; k < np_; k += kThreads) o[k] = __fadd_rn(__fmul_rn(scale, p[k]), off);   // two roundings, as numpy
        return;
    }
    double s = 0.0;   // scale == 0 for the whole workgroup: the barriers below are uniform
    for (int k = tid; k < np_; k += kThreads) s += (double)p[k];
    s = block_reduce_sum(s, shd);
    const float mean = (float)(s / (double)np_);
    for (int k = tid; k < np_; k += kThreads) o[k] = __fdiv_rn(__fmul_rn(p[k], off), mean);
}

int pair_grid_of(int B, int H, int W, int width, int pad_mode, long* nchunks, long* npix) {
    const long Ho = pad_mode == EMD_K_PAD_VALID ? H - width + 1 : H, Wo = pad_mode == EMD_K_PAD_VALID ? W - width + 1 : W;
    *npix = (long)B * Ho * Wo;
    *nchunks = (*npix + kChunk - 1) / kChunk;
    return (int)(*nchunks < kMaxGrid ? *nchunks : kMaxGrid);
}

template <int D>
void launch_pair_grad(bool valid, const float* x, const float* truth, int B, int H, int W, int width, int want_grad,
                      const float* theta, float* partial, long nchunks, int nwg, hipStream_t st) {
    if (valid)
        hipLaunchKernelGGL((k_pair_grad_kernel<D, true>), dim3(nwg), dim3(kThreads), 0, st, x, truth, B, H, W, width, want_grad, theta,
                           partial, nchunks);
    else
        hipLaunchKernelGGL((k_pair_grad_kernel<D, false>), dim3(nwg), dim3(kThreads), 0, st, x, truth, B, H, W, width, want_grad, theta,
                           partial, nchunks);
}

}  // namespace

extern "C" int emd_k_train_pair_step_f32(const float* x, const float* truth, int B, int H, int W, int width, int depth, int pad_mode,
                                         float* theta, float* adam_m, float* adam_v, int* step, double lr0, long total_steps,
                                         float beta1, float beta2, float eps, unsigned flags, float* grad_out, float* loss_out,
                                         float* params_out, void* workspace, size_t workspace_bytes, emd_stream_t stream) {
    const bool update = flags & EMD_K_TRAIN_UPDATE, no_grad = flags & EMD_K_TRAIN_LOSS_ONLY;
    const bool valid = pad_mode == EMD_K_PAD_VALID;
    EMD_REQUIRE((flags & ~(EMD_K_TRAIN_UPDATE | EMD_K_TRAIN_LOSS_ONLY | EMD_K_TRAIN_SQRT_ABOVE_1)) == 0, EMD_E_INVALID,
                "emd_k_train_pair_step_f32: unknown flag");
    EMD_REQUIRE(!(update && no_grad), EMD_E_INVALID, "emd_k_train_pair_step_f32: an update needs the gradient");
    EMD_REQUIRE(x && truth && theta && workspace, EMD_E_INVALID, "emd_k_train_pair_step_f32: null pointer");
    EMD_REQUIRE(!update || (adam_m && adam_v && step), EMD_E_INVALID, "emd_k_train_pair_step_f32: null pointer (Adam state)");
    EMD_REQUIRE(width >= 3 && (width & 1) && width <= EMD_K_MAX_WIDTH, EMD_E_INVALID,
                "emd_k_train_pair_step_f32: width must be odd, 3..15");
    EMD_REQUIRE(depth >= 1 && depth <= EMD_K_MAX_DEPTH, EMD_E_INVALID, "emd_k_train_pair_step_f32: depth must be 1..5");
    EMD_REQUIRE(B >= 1 && H >= 1 && W >= 1, EMD_E_INVALID, "emd_k_train_pair_step_f32: bad shape");
    EMD_REQUIRE((long)H * W < 0x7fffffffL, EMD_E_UNSUPPORTED, "emd_k_train_pair_step_f32: image too large");
    EMD_REQUIRE(valid || pad_mode == EMD_K_PAD_REFLECT, EMD_E_INVALID, "emd_k_train_pair_step_f32: unknown border mode");
    EMD_REQUIRE(!valid || (width <= H && width <= W), EMD_E_INVALID,
                "emd_k_train_pair_step_f32: VALID needs width <= min(H,W)");
    EMD_REQUIRE(valid || (width / 2 < H && width / 2 < W), EMD_E_INVALID,
                "emd_k_train_pair_step_f32: REFLECT padding needs width/2 < min(H,W)");
    EMD_REQUIRE(!update || (total_steps >= 1 && lr0 >= 0.0), EMD_E_INVALID, "emd_k_train_pair_step_f32: bad schedule");
    EMD_REQUIRE(workspace_bytes >= emd_k_train_workspace_bytes(B, H, W, width, depth), EMD_E_INVALID,
                "emd_k_train_pair_step_f32: workspace too small");
    hipStream_t st = static_cast<hipStream_t>(stream);
    long nchunks, npix;
    const int nwg = pair_grid_of(B, H, W, width, pad_mode, &nchunks, &npix);   // never more slabs than the H x W grid the workspace holds
    float* partial = static_cast<float*>(workspace);
    const int want_grad = no_grad ? 0 : 1;
    switch (depth) {
        case 1: launch_pair_grad<1>(valid, x, truth, B, H, W, width, want_grad, theta, partial, nchunks, nwg, st); break;
        case 2: launch_pair_grad<2>(valid, x, truth, B, H, W, width, want_grad, theta, partial, nchunks, nwg, st); break;
        case 3: launch_pair_grad<3>(valid, x, truth, B, H, W, width, want_grad, theta, partial, nchunks, nwg, st); break;
        case 4: launch_pair_grad<4>(valid, x, truth, B, H, W, width, want_grad, theta, partial, nchunks, nwg, st); break;
        default: launch_pair_grad<5>(valid, x, truth, B, H, W, width, want_grad, theta, partial, nchunks, nwg, st); break;
    }
    int rc = emd::check_launch("k_pair_grad_kernel");
    if (rc != EMD_OK) return rc;
    const int n1 = nscal_of(width, depth) + 1;
    int R = 1;
    while (R < 64 && 2 * R * n1 <= kUpdThreads) R *= 2;
    hipLaunchKernelGGL(k_pair_update_kernel, dim3(1), dim3(kUpdThreads), 0, st, static_cast<const float*>(partial), nwg, R, width, depth,
                       npix, theta, adam_m, adam_v, step, lr0, total_steps, beta1, beta2, eps, update ? 1 : 0,
                       (flags & EMD_K_TRAIN_SQRT_ABOVE_1) ? 1 : 0, no_grad ? nullptr : grad_out, loss_out, params_out);
    return emd::check_launch("k_pair_update_kernel");
}

extern "C" int emd_k_make_pairs_f32(const float* a, const float* b, int N, int H, int W, int patch, int lo, int hi,
                                    unsigned long long seed, unsigned long long first_index, float* x, float* t, int* draws_out,
                                    emd_stream_t stream) {
    EMD_REQUIRE(a && b && x && t, EMD_E_INVALID, "emd_k_make_pairs_f32: null pointer");
    EMD_REQUIRE(N >= 1 && H >= 1 && W >= 1 && patch >= 1, EMD_E_INVALID, "emd_k_make_pairs_f32: bad shape");
    EMD_REQUIRE((long)H * W < 0x7fffffffL, EMD_E_UNSUPPORTED, "emd_k_make_pairs_f32: image too large");
    EMD_REQUIRE(N <= 0x7fffffff / 2, EMD_E_UNSUPPORTED, "emd_k_make_pairs_f32: too many images");
    EMD_REQUIRE(lo >= 0 && hi > lo, EMD_E_INVALID, "emd_k_make_pairs_f32: the offset window [lo, hi) is empty");
    EMD_REQUIRE((long)hi - 1 + patch <= H && (long)hi - 1 + patch <= W, EMD_E_INVALID,
                "emd_k_make_pairs_f32: a patch at offset hi - 1 does not fit the image");
    hipLaunchKernelGGL(k_make_pairs_kernel, dim3(N), dim3(kThreads), 0, static_cast<hipStream_t>(stream), a, b, H, W, patch, lo, hi,
                       seed, first_index, x, t, draws_out);
    return emd::check_launch("k_make_pairs_kernel");
}

extern "C" int emd_s_crop_unscale_f32(const float* pred, const float* crop_stats, int N, int npix, float* out, emd_stream_t stream) {
    EMD_REQUIRE(pred && crop_stats && out, EMD_E_INVALID, "emd_s_crop_unscale_f32: null pointer");
    EMD_REQUIRE(N >= 1 && npix >= 1, EMD_E_INVALID, "emd_s_crop_unscale_f32: bad shape");
    hipLaunchKernelGGL(s_crop_unscale_kernel, dim3(N), dim3(kThreads), 0, static_cast<hipStream_t>(stream), pred, crop_stats, npix, out);
    return emd::check_launch("s_crop_unscale_kernel");
}
