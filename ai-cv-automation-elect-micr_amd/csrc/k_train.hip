// Graph K training (see include/emdenoise.h, emd_k_train_step_f32 / emd_k_sample_crops_f32).
// replaces: misc_py/noise-removal-kernels.py:409-438 (the per-pixel unrolled filter graph and its MSE loss), the gradient
// TensorFlow derives from it, :442-446 + :665-678 (one AdamOptimizer per filter, lr = lr0 (1 - t / (T + 1))), and the host
// input path :450-538 (load_image -> flip_rotate -> preprocess -> record_parser).
//
// The trainable state of one (depth, width) filter is a vector `theta` of make_layer scalars (:107-358), one per D4 class of
// tap positions, laid out as
//     w [depth][nsym]  |  b [depth-1][nsym] (b1..)  |  s [depth-1] (fully_connected scalars s1..)      nsym = (o+1)(o+2)/2
// A scalar's gradient is the SUM over the taps of its class.
//
// k_grad_kernel<D>  forward + backward, one thread per output pixel (4 pixels per thread), per tap.  The flattened [B,H,W]
//   pixel range is cut into chunks of 1024; a workgroup walks chunks blockIdx.x, + gridDim.x, ... .  Per tap the thread's
//   (2D-1) class contributions are summed over its pixels in registers, over the wave by a xor butterfly, and lane 0 adds
//   them into its wave's LDS slab; the fully_connected gradients and the squared error stay in registers to the end.  The
//   four wave slabs are added in a fixed order into the workgroup's partial slab.  No float atomics anywhere: for a given
//   shape the grid, every thread's pixels and every summation order are fixed, so a step is bitwise reproducible.
// k_update_kernel   one workgroup: the partial slabs are summed in a fixed order (double), scaled by 2/N (the loss by 1/N),
//   Adam is applied to theta with lr_t computed on the device from the step counter, and theta is expanded into the packed
//   [wmaps | bmaps | s] block of emd_kernel_denoise_f32, so the filter can be applied with no host round trip.
// k_sample_kernel   one workgroup per crop: Philox draws (image, x, y, D4 element), crop, D4, NaN/Inf -> 0, scale0to1, / mean.
// k_fused_kernel<D> the small-batch form: one workgroup per filter runs n whole steps (sample, forward/backward, reduce, Adam).
#include <cmath>

#include "emd_common.hpp"
#include "k_common.hpp"
#include "philox.hpp"

namespace {

template <int D>
__global__ __launch_bounds__(kThreads) void k_grad_kernel(const float* __restrict__ x, int B, int H, int W, int width,
                                                          int loss_mode, int want_grad, const float* __restrict__ theta,
                                                          float* __restrict__ partial, long nchunks) {
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

    const long HW = (long)H * W, total = (long)B * HW;
    float s_acc[D], loss_acc = 0.f;
#pragma unroll
    for (int l = 0; l < D; ++l) s_acc[l] = 0.f;

    for (long chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
        const float* img[kPx];
        int pr[kPx], pc[kPx];
        float e[kPx];
#pragma unroll
        for (int q = 0; q < kPx; ++q) {
            long idx = chunk * kChunk + q * kThreads + tid;
            const bool valid = idx < total;
            if (!valid) idx = 0;
            const long b = idx / HW;
            const int rem = (int)(idx - b * HW);
            pr[q] = rem / W;
            pc[q] = rem - pr[q] * W;
            img[q] = x + b * HW;
            // target: the input itself ("image"), or its transpose (the reference's loss, :421-424 + :438; H == W)
            const float tgt = loss_mode == EMD_K_LOSS_IMAGE ? img[q][rem] : img[q][(long)pc[q] * W + pr[q]];
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
                    const int rr = reflect((pr[q] < 0 ? 0 : pr[q]) + i - o, H), cc = reflect(pc[q] + j - o, W);
                    float f = wl[0] * img[q][(long)rr * W + cc];
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
        // backward, per tap: dL/df_{D-1} = e (the factor 2/N is applied by k_update_kernel)
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
                    const int rr = reflect((pr[q] < 0 ? 0 : pr[q]) + i - o, H), cc = reflect(pc[q] + j - o, W);
                    const float v = img[q][(long)rr * W + cc];
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

// One workgroup of kUpdThreads: k_update_body (k_common.hpp) without the paired trainer's sqrt rule.
__global__ __launch_bounds__(kUpdThreads) void k_update_kernel(const float* __restrict__ partial, int nwg, int R, int width,
                                                               int depth, long npix, float* __restrict__ theta,
                                                               float* __restrict__ adam_m, float* __restrict__ adam_v,
                                                               int* __restrict__ step, double lr0, long total_steps,
                                                               float beta1, float beta2, float eps, int update,
                                                               float* __restrict__ grad_out, float* __restrict__ loss_out,
                                                               float* __restrict__ params_out) {
    k_update_body<false>(partial, nwg, R, width, depth, npix, theta, adam_m, adam_v, step, lr0, total_steps, beta1, beta2, eps, update,
                         0, grad_out, loss_out, params_out);
}

// ---- the input path (:450-538) for one crop per workgroup
// S = true: graph S's input path (misc_py/autoencoder.py:190-274): its own Philox tag, a non-finite crop becomes ONES (:271-272),
// x4 (may be NULL) receives a copy of every crop in channel 0 of a [B][crop][crop][4] tensor (its other channels are not touched), and
// first_index_dev (may be NULL) holds the first crop index on the device (a replayed graph).
template <bool S>
__global__ __launch_bounds__(kThreads) void k_sample_kernel(const float* __restrict__ stack, int N, int H, int W,
                                                            float* __restrict__ crops, int crop, unsigned long long seed,
                                                            unsigned long long first_index, int* __restrict__ draws,
                                                            float* __restrict__ x4, const unsigned long long* __restrict__ first_index_dev) {
    __shared__ float shf[kWaves];
    __shared__ double shd[kWaves];
    __shared__ int bad;
    const int b = blockIdx.x, tid = threadIdx.x;
    const unsigned long long idx = (S && first_index_dev ? *first_index_dev : first_index) + (unsigned long long)b;
    constexpr unsigned tag = S ? emd::kPhiloxTagSCrop : emd::kPhiloxTagKCrop;
    const emd::U4 r = emd::philox4x32_10(emd::U4{(unsigned)idx, (unsigned)(idx >> 32), 0u, tag},
                                         (unsigned)seed, (unsigned)(seed >> 32));
    const int n = (int)draw_below(r.x, (unsigned)N);
    const int x0 = (int)draw_below(r.y, (unsigned)(H - crop));   // np.random.randint(0, H - crop): upper bound exclusive
    const int y0 = (int)draw_below(r.z, (unsigned)(W - crop));
    const int ch = (int)(r.w >> 29);                             // np.random.randint(0, 8)
    if (tid == 0) {
        bad = 0;
        if (draws) {
            draws[4 * b + 0] = n;
            draws[4 * b + 1] = x0;
            draws[4 * b + 2] = y0;
            draws[4 * b + 3] = ch;
        }
    }
    const float* src = stack + (size_t)n * H * W + (size_t)x0 * W + y0;
    float* out = crops + (size_t)b * crop * crop;
    const int np_ = crop * crop;
    // flip_rotate (:498-515), as emd_flip_rotate_f32: out[i][j] = in[si][sj]
    const bool transposing = ch == 1 || ch == 3 || ch == 6 || ch == 7;
    const bool flip_i = ch == 2 || ch == 4 || ch == 3 || ch == 7;
    const bool flip_j = ch == 2 || ch == 5 || ch == 1 || ch == 7;
    auto fetch = [&](int k) {
        const int i = k / crop, j = k - (k / crop) * crop;
        const int ro = transposing ? j : i, co = transposing ? i : j;
        const int si = flip_i ? crop - 1 - ro : ro, sj = flip_j ? crop - 1 - co : co;
        const float v = src[(size_t)si * W + sj];
        return fabsf(v) <= 3.402823466e38f ? v : 0.f;   // preprocess: NaN and +-Inf -> 0 (:519-520)
    };
    float mn = INFINITY, mx = -INFINITY;
    for (int k = tid; k < np_; k += kThreads) {
        const float v = fetch(k);
        out[k] = v;
        mn = fminf(mn, v);
        mx = fmaxf(mx, v);
    }
    mn = block_reduce_min(mn, shf);
    mx = block_reduce_max(mx, shf);
    // scale0to1 (:474-484) in float32; constant crop -> 0.5
    const float d = mx - mn;
    double s = 0.0;
    for (int k = tid; k < np_; k += kThreads) {   // each thread re-reads only what it wrote itself
        const float v = mn == mx ? 0.5f : (out[k] - mn) / d;
        out[k] = v;
        s += (double)v;
    }
    s = block_reduce_sum(s, shd);
    const float mean = (float)(s / (double)np_);   // img /= np.mean(img) (:526)
    int nonfinite = 0;
    for (int k = tid; k < np_; k += kThreads) {
        const float v = out[k] / mean;
        out[k] = v;
        nonfinite |= !(fabsf(v) <= 3.402823466e38f);
    }
    if (nonfinite) bad = 1;   // benign race: every writer stores 1
    __syncthreads();
    if (bad)   // record_parser (:534-535): a crop with any non-finite value becomes zeros (graph S: ones)
        for (int k = tid; k < np_; k += kThreads) out[k] = S ? 1.f : 0.f;
    if (S && x4)   // each thread copies only what it wrote itself
        for (int k = tid; k < np_; k += kThreads) x4[((size_t)b * np_ + k) * 4] = out[k];
}

// ---- (c) the fused small-batch form: one workgroup per filter runs `nsteps` complete steps in one launch ----------------
// Per step: the batch is sampled into LDS (one wave per crop; the arithmetic of k_sample_kernel with wave-level reductions,
// so the mean can differ from emd_k_sample_crops_f32's in the last bit) or copied from the caller's fixed batches; forward +
// backward as k_grad_kernel but over the LDS image; the kFWaves wave slabs are summed in a fixed order (double), and Adam is
// applied to theta / m / v held in LDS.  No grid-wide synchronisation: filters are independent workgroups.  LDS: the batch
// (B * crop^2 floats <= EMD_K_FUSED_MAX_PIXELS = 32 KiB) + kFWaves slabs + theta / m / v ~ 47 KiB.
constexpr int kFThreads = 512, kFWaves = kFThreads / 64, kFChunk = kFThreads * kPx;
constexpr int kMaxFusedJobs = 32;

struct FusedArgs {
    emd_k_fused_job_t job[kMaxFusedJobs];
};

// crop b of the batch drawn for crop index `idx`, by one wave, into dst[crop*crop]
__device__ void sample_crop_wave(const float* __restrict__ stack, int N, int H, int W, int crop, unsigned long long seed,
                                 unsigned long long idx, float* dst, int lane) {
    const emd::U4 r = emd::philox4x32_10(emd::U4{(unsigned)idx, (unsigned)(idx >> 32), 0u, emd::kPhiloxTagKCrop},
                                         (unsigned)seed, (unsigned)(seed >> 32));
    const int n = (int)draw_below(r.x, (unsigned)N);
    const int x0 = (int)draw_below(r.y, (unsigned)(H - crop));
    const int y0 = (int)draw_below(r.z, (unsigned)(W - crop));
    const int ch = (int)(r.w >> 29);
    const float* src = stack + (size_t)n * H * W + (size_t)x0 * W + y0;
    const bool transposing = ch == 1 || ch == 3 || ch == 6 || ch == 7;
    const bool flip_i = ch == 2 || ch == 4 || ch == 3 || ch == 7;
    const bool flip_j = ch == 2 || ch == 5 || ch == 1 || ch == 7;
    const int np_ = crop * crop;
    float mn = INFINITY, mx = -INFINITY;
    for (int k = lane; k < np_; k += 64) {
        const int i = k / crop, j = k - (k / crop) * crop;
        const int ro = transposing ? j : i, co = transposing ? i : j;
        const int si = flip_i ? crop - 1 - ro : ro, sj = flip_j ? crop - 1 - co : co;
        float v = src[(size_t)si * W + sj];
        v = fabsf(v) <= 3.402823466e38f ? v : 0.f;
        dst[k] = v;
        mn = fminf(mn, v);
        mx = fmaxf(mx, v);
    }
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        mn = fminf(mn, __shfl_xor(mn, o));
        mx = fmaxf(mx, __shfl_xor(mx, o));
    }
    const float d = mx - mn;
    double s = 0.0;
    for (int k = lane; k < np_; k += 64) {
        const float v = mn == mx ? 0.5f : (dst[k] - mn) / d;
        dst[k] = v;
        s += (double)v;
    }
    const float mean = (float)(wave_sum(s) / (double)np_);
    int bad = 0;
    for (int k = lane; k < np_; k += 64) {
        const float v = dst[k] / mean;
        dst[k] = v;
        bad |= !(fabsf(v) <= 3.402823466e38f);
    }
    if (__any(bad))
        for (int k = lane; k < np_; k += 64) dst[k] = 0.f;
}

template <int D>
__global__ __launch_bounds__(kFThreads) void k_fused_kernel(FusedArgs args, const float* __restrict__ stack, int N, int H, int W,
                                                            const float* __restrict__ batches, int nbatches, int B, int crop,
                                                            unsigned long long seed, int nsteps, int loss_mode, double lr0,
                                                            long total_steps, float beta1, float beta2, float eps) {
    __shared__ float img[EMD_K_FUSED_MAX_PIXELS];
    __shared__ float acc[kFWaves][kMaxScal + 1];
    __shared__ float th[kMaxScal], am[kMaxScal], av[kMaxScal];
    __shared__ unsigned char cls[EMD_K_MAX_WIDTH * EMD_K_MAX_WIDTH];
    const emd_k_fused_job_t job = args.job[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int width = job.width, o = width >> 1, ww = width * width;
    const int nsym = (o + 1) * (o + 2) / 2;
    const int nscal = (2 * D - 1) * nsym + D - 1;
    const int offB = D * nsym - nsym, offS = (2 * D - 1) * nsym - 1;
    const int S = crop, SS = crop * crop, npix = B * SS;
    const long nchunks = (npix + kFChunk - 1) / kFChunk;
    for (int i = tid; i < nscal; i += kFThreads) {
        th[i] = job.theta[i];
        am[i] = job.adam_m[i];
        av[i] = job.adam_v[i];
    }
    for (int k = tid; k < ww; k += kFThreads) cls[k] = (unsigned char)tap_class(k / width, k % width, o);
    const int step0 = job.step[0];

    for (int it = 0; it < nsteps; ++it) {
        const int t = step0 + it + 1;   // 1-based step of this update
        if (batches) {
            const float* src = batches + (size_t)(it % nbatches) * npix;
            for (int i = tid; i < npix; i += kFThreads) img[i] = src[i];
        } else {
            for (int b = wv; b < B; b += kFWaves)
                sample_crop_wave(stack, N, H, W, crop, seed, (unsigned long long)(t - 1) * B + b, img + b * SS, lane);
        }
        for (int i = tid; i < kFWaves * (kMaxScal + 1); i += kFThreads) (&acc[0][0])[i] = 0.f;
        __syncthreads();

        float s_acc[D], loss_acc = 0.f;
#pragma unroll
        for (int l = 0; l < D; ++l) s_acc[l] = 0.f;
        for (long chunk = 0; chunk < nchunks; ++chunk) {
            int pb[kPx], pr[kPx], pc[kPx];
            float e[kPx];
#pragma unroll
            for (int q = 0; q < kPx; ++q) {
                int idx = (int)chunk * kFChunk + q * kFThreads + tid;
                const bool valid = idx < npix;
                if (!valid) idx = 0;
                pb[q] = idx / SS;
                const int rem = idx - pb[q] * SS;
                pr[q] = rem / S;
                pc[q] = rem - pr[q] * S;
                const float tgt = loss_mode == EMD_K_LOSS_IMAGE ? img[idx] : img[pb[q] * SS + pc[q] * S + pr[q]];
                e[q] = valid ? -tgt : 0.f;
                if (!valid) pr[q] = -1;
            }
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
                        const int rr = reflect((pr[q] < 0 ? 0 : pr[q]) + i - o, S), cc = reflect(pc[q] + j - o, S);
                        float f = wl[0] * img[pb[q] * SS + rr * S + cc];
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
                        const int rr = reflect((pr[q] < 0 ? 0 : pr[q]) + i - o, S), cc = reflect(pc[q] + j - o, S);
                        const float v = img[pb[q] * SS + rr * S + cc];
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
        // fixed-order sum of the wave slabs, then TF's Adam (k_update_kernel's arithmetic)
        const float lr = (float)(lr0 * (1.0 - (double)t / (double)(total_steps + 1)));
        const float lr_t = (float)((double)lr * sqrt(1.0 - pow((double)beta2, (double)t)) / (1.0 - pow((double)beta1, (double)t)));
        for (int i = tid; i <= nscal; i += kFThreads) {
            double sum = 0.0;
            for (int w = 0; w < kFWaves; ++w) sum += (double)acc[w][i];
            if (i == nscal) {
                job.losses[it] = (float)(sum / (double)npix);
                continue;
            }
            const float g = (float)(sum * 2.0 / (double)npix);
            const float mi = beta1 * am[i] + (1.f - beta1) * g;
            const float vi = beta2 * av[i] + (1.f - beta2) * g * g;
            am[i] = mi;
            av[i] = vi;
            th[i] = th[i] - lr_t * mi / (sqrtf(vi) + eps);
        }
        __syncthreads();
    }
    for (int i = tid; i < nscal; i += kFThreads) {
        job.theta[i] = th[i];
        job.adam_m[i] = am[i];
        job.adam_v[i] = av[i];
    }
    if (job.params_out) {
        const int n = 2 * D * ww + D;
        for (int k = tid; k < n; k += kFThreads) {
            float val;
            if (k < 2 * D * ww) {
                const int l = (k / ww) % D, tap = k % ww;
                const int c = tap_class(tap / width, tap % width, o);
                if (k < D * ww) val = th[l * nsym + c];
                else val = l ? th[offB + l * nsym + c] : 0.f;
            } else {
                const int l = k - 2 * D * ww;
                val = l ? th[offS + l] : 1.f;
            }
            job.params_out[k] = val;
        }
    }
    if (tid == 0) job.step[0] = step0 + nsteps;
}

template <int D>
void launch_grad(const float* x, int B, int H, int W, int width, int loss_mode, int want_grad, const float* theta, float* partial,
                 long nchunks, int nwg, hipStream_t st) {
    hipLaunchKernelGGL(k_grad_kernel<D>, dim3(nwg), dim3(kThreads), 0, st, x, B, H, W, width, loss_mode, want_grad, theta, partial,
                       nchunks);
}

int grid_of(int B, int H, int W, long* nchunks) {
    const long total = (long)B * H * W;
    *nchunks = (total + kChunk - 1) / kChunk;
    return (int)(*nchunks < kMaxGrid ? *nchunks : kMaxGrid);
}

}  // namespace

extern "C" size_t emd_k_train_scalar_count(int width, int depth) {
    if (width < 1 || !(width & 1) || width > EMD_K_MAX_WIDTH || depth < 1 || depth > EMD_K_MAX_DEPTH) return 0;
    return (size_t)nscal_of(width, depth);
}

extern "C" size_t emd_k_train_workspace_bytes(int B, int H, int W, int width, int depth) {
    const size_t n = emd_k_train_scalar_count(width, depth);
    if (n == 0 || B < 1 || H < 1 || W < 1) return 0;
    long nchunks;
    const int nwg = grid_of(B, H, W, &nchunks);
    return (size_t)nwg * (n + 1) * sizeof(float);
}

extern "C" int emd_k_train_step_f32(const float* x, int B, int H, int W, int width, int depth, int loss_mode, float* theta,
                                    float* adam_m, float* adam_v, int* step, double lr0, long total_steps, float beta1,
                                    float beta2, float eps, unsigned flags, float* grad_out, float* loss_out, float* params_out,
                                    void* workspace, size_t workspace_bytes, emd_stream_t stream) {
    const bool update = flags & EMD_K_TRAIN_UPDATE, no_grad = flags & EMD_K_TRAIN_LOSS_ONLY;
    EMD_REQUIRE((flags & ~(EMD_K_TRAIN_UPDATE | EMD_K_TRAIN_LOSS_ONLY)) == 0, EMD_E_INVALID, "emd_k_train_step_f32: unknown flag");
    EMD_REQUIRE(!(update && no_grad), EMD_E_INVALID, "emd_k_train_step_f32: an update needs the gradient");
    EMD_REQUIRE(x && theta && workspace, EMD_E_INVALID, "emd_k_train_step_f32: null pointer");
    EMD_REQUIRE(!update || (adam_m && adam_v && step), EMD_E_INVALID, "emd_k_train_step_f32: null pointer (Adam state)");
    EMD_REQUIRE(width >= 3 && (width & 1) && width <= EMD_K_MAX_WIDTH, EMD_E_INVALID,
                "emd_k_train_step_f32: width must be odd, 3..15");
    EMD_REQUIRE(depth >= 1 && depth <= EMD_K_MAX_DEPTH, EMD_E_INVALID, "emd_k_train_step_f32: depth must be 1..5");
    EMD_REQUIRE(B >= 1 && H >= 1 && W >= 1, EMD_E_INVALID, "emd_k_train_step_f32: bad shape");
    EMD_REQUIRE((long)H * W < 0x7fffffffL, EMD_E_UNSUPPORTED, "emd_k_train_step_f32: image too large");
    EMD_REQUIRE(width / 2 < H && width / 2 < W, EMD_E_INVALID, "emd_k_train_step_f32: REFLECT padding needs width/2 < min(H,W)");
    EMD_REQUIRE(loss_mode == EMD_K_LOSS_REFERENCE || loss_mode == EMD_K_LOSS_IMAGE, EMD_E_INVALID,
                "emd_k_train_step_f32: unknown loss mode");
    EMD_REQUIRE(loss_mode != EMD_K_LOSS_REFERENCE || H == W, EMD_E_INVALID,
                "emd_k_train_step_f32: the reference loss compares the transposed output: square crops only");
    EMD_REQUIRE(!update || (total_steps >= 1 && lr0 >= 0.0), EMD_E_INVALID, "emd_k_train_step_f32: bad schedule");
    EMD_REQUIRE(workspace_bytes >= emd_k_train_workspace_bytes(B, H, W, width, depth), EMD_E_INVALID,
                "emd_k_train_step_f32: workspace too small");
    hipStream_t st = static_cast<hipStream_t>(stream);
    long nchunks;
    const int nwg = grid_of(B, H, W, &nchunks);
    float* partial = static_cast<float*>(workspace);
    const int want_grad = no_grad ? 0 : 1;
    switch (depth) {
        case 1: launch_grad<1>(x, B, H, W, width, loss_mode, want_grad, theta, partial, nchunks, nwg, st); break;
        case 2: launch_grad<2>(x, B, H, W, width, loss_mode, want_grad, theta, partial, nchunks, nwg, st); break;
        case 3: launch_grad<3>(x, B, H, W, width, loss_mode, want_grad, theta, partial, nchunks, nwg, st); break;
        case 4: launch_grad<4>(x, B, H, W, width, loss_mode, want_grad, theta, partial, nchunks, nwg, st); break;
        default: launch_grad<5>(x, B, H, W, width, loss_mode, want_grad, theta, partial, nchunks, nwg, st); break;
    }
    int rc = emd::check_launch("k_grad_kernel");
    if (rc != EMD_OK) return rc;
    const int n1 = nscal_of(width, depth) + 1;
    int R = 1;
    while (R < 64 && 2 * R * n1 <= kUpdThreads) R *= 2;
    hipLaunchKernelGGL(k_update_kernel, dim3(1), dim3(kUpdThreads), 0, st, static_cast<const float*>(partial), nwg, R, width, depth,
                       (long)B * H * W, theta, adam_m, adam_v, step, lr0, total_steps, beta1, beta2, eps, update ? 1 : 0,
                       no_grad ? nullptr : grad_out, loss_out, params_out);
    return emd::check_launch("k_update_kernel");
}

extern "C" int emd_k_sample_crops_f32(const float* stack, int N, int H, int W, float* crops, int B, int crop,
                                      unsigned long long seed, unsigned long long first_index, int* draws_out,
                                      emd_stream_t stream) {
    EMD_REQUIRE(stack && crops, EMD_E_INVALID, "emd_k_sample_crops_f32: null pointer");
    EMD_REQUIRE(N >= 1 && H >= 1 && W >= 1 && B >= 1 && crop >= 1, EMD_E_INVALID, "emd_k_sample_crops_f32: bad shape");
    EMD_REQUIRE(crop < H && crop < W, EMD_E_INVALID,
                "emd_k_sample_crops_f32: crop must be smaller than the image (randint(0, H - crop) needs H > crop)");
    EMD_REQUIRE(B <= 0x7fffffff / 4, EMD_E_UNSUPPORTED, "emd_k_sample_crops_f32: batch too large");
    hipLaunchKernelGGL(k_sample_kernel<false>, dim3(B), dim3(kThreads), 0, static_cast<hipStream_t>(stream), stack, N, H, W, crops, crop, seed,
                       first_index, draws_out, nullptr, nullptr);
    return emd::check_launch("k_sample_kernel");
}

extern "C" int emd_s_sample_crops_f32(const float* stack, int N, int H, int W, float* crops, float* x4, int B, int crop,
                                      unsigned long long seed, unsigned long long first_index,
                                      const unsigned long long* first_index_dev, int* draws_out, emd_stream_t stream) {
    EMD_REQUIRE(stack && crops, EMD_E_INVALID, "emd_s_sample_crops_f32: null pointer");
    EMD_REQUIRE(N >= 1 && H >= 1 && W >= 1 && B >= 1 && crop >= 1, EMD_E_INVALID, "emd_s_sample_crops_f32: bad shape");
    EMD_REQUIRE(crop < H && crop < W, EMD_E_INVALID,
                "emd_s_sample_crops_f32: crop must be smaller than the image (randint(0, H - crop) needs H > crop)");
    EMD_REQUIRE(B <= 0x7fffffff / 4, EMD_E_UNSUPPORTED, "emd_s_sample_crops_f32: batch too large");
    EMD_REQUIRE((long)B * crop * crop * 4 < (1L << 40), EMD_E_UNSUPPORTED, "emd_s_sample_crops_f32: batch too large");
    hipLaunchKernelGGL(k_sample_kernel<true>, dim3(B), dim3(kThreads), 0, static_cast<hipStream_t>(stream), stack, N, H, W, crops, crop, seed,
                       first_index, draws_out, x4, first_index_dev);
    return emd::check_launch("k_sample_kernel");
}

extern "C" int emd_k_train_fused_f32(const emd_k_fused_job_t* jobs, int njobs, const float* stack, int N, int H, int W,
                                     const float* batches, int nbatches, int B, int crop, unsigned long long seed, int nsteps,
                                     int loss_mode, double lr0, long total_steps, float beta1, float beta2, float eps,
                                     emd_stream_t stream) {
    EMD_REQUIRE(jobs && njobs >= 1, EMD_E_INVALID, "emd_k_train_fused_f32: null pointer or no jobs");
    EMD_REQUIRE(nsteps >= 1 && nsteps <= EMD_K_FUSED_MAX_STEPS, EMD_E_INVALID, "emd_k_train_fused_f32: nsteps must be 1..1000");
    EMD_REQUIRE(B >= 1 && crop >= 1, EMD_E_INVALID, "emd_k_train_fused_f32: bad shape");
    EMD_REQUIRE((long)B * crop * crop <= EMD_K_FUSED_MAX_PIXELS, EMD_E_UNSUPPORTED,
                "emd_k_train_fused_f32: the batch does not fit the LDS budget (B * crop^2 <= 8192)");
    EMD_REQUIRE(loss_mode == EMD_K_LOSS_REFERENCE || loss_mode == EMD_K_LOSS_IMAGE, EMD_E_INVALID,
                "emd_k_train_fused_f32: unknown loss mode");
    EMD_REQUIRE(total_steps >= 1 && lr0 >= 0.0, EMD_E_INVALID, "emd_k_train_fused_f32: bad schedule");
    if (batches) {
        EMD_REQUIRE(nbatches >= 1, EMD_E_INVALID, "emd_k_train_fused_f32: nbatches must be >= 1");
    } else {
        EMD_REQUIRE(stack, EMD_E_INVALID, "emd_k_train_fused_f32: null pointer (stack)");
        EMD_REQUIRE(N >= 1 && H >= 1 && W >= 1, EMD_E_INVALID, "emd_k_train_fused_f32: bad shape");
        EMD_REQUIRE(crop < H && crop < W, EMD_E_INVALID,
                    "emd_k_train_fused_f32: crop must be smaller than the image (randint(0, H - crop) needs H > crop)");
    }
    int count[EMD_K_MAX_DEPTH + 1] = {};
    for (int i = 0; i < njobs; ++i) {
        const emd_k_fused_job_t& j = jobs[i];
        EMD_REQUIRE(j.theta && j.adam_m && j.adam_v && j.step && j.losses, EMD_E_INVALID,
                    "emd_k_train_fused_f32: null pointer in a job");
        EMD_REQUIRE(j.width >= 3 && (j.width & 1) && j.width <= EMD_K_MAX_WIDTH, EMD_E_INVALID,
                    "emd_k_train_fused_f32: width must be odd, 3..15");
        EMD_REQUIRE(j.depth >= 1 && j.depth <= EMD_K_MAX_DEPTH, EMD_E_INVALID, "emd_k_train_fused_f32: depth must be 1..5");
        EMD_REQUIRE(j.width / 2 < crop, EMD_E_INVALID, "emd_k_train_fused_f32: REFLECT padding needs width/2 < crop");
        ++count[j.depth];
    }
    for (int d = 1; d <= EMD_K_MAX_DEPTH; ++d)
        EMD_REQUIRE(count[d] <= kMaxFusedJobs, EMD_E_UNSUPPORTED, "emd_k_train_fused_f32: more than 32 filters of one depth");
    hipStream_t st = static_cast<hipStream_t>(stream);
    for (int d = 1; d <= EMD_K_MAX_DEPTH; ++d) {   // one launch per depth present, one workgroup per filter
        if (!count[d]) continue;
        FusedArgs a = {};
        int n = 0;
        for (int i = 0; i < njobs; ++i)
            if (jobs[i].depth == d) a.job[n++] = jobs[i];
#define EMD_K_FUSED_LAUNCH(DD)                                                                                          \
    hipLaunchKernelGGL(k_fused_kernel<DD>, dim3(n), dim3(kFThreads), 0, st, a, stack, N, H, W, batches, nbatches, B, crop, \
                       seed, nsteps, loss_mode, lr0, total_steps, beta1, beta2, eps)
        switch (d) {
            case 1: EMD_K_FUSED_LAUNCH(1); break;
            case 2: EMD_K_FUSED_LAUNCH(2); break;
            case 3: EMD_K_FUSED_LAUNCH(3); break;
            case 4: EMD_K_FUSED_LAUNCH(4); break;
            default: EMD_K_FUSED_LAUNCH(5); break;
        }
#undef EMD_K_FUSED_LAUNCH
        const int rc = emd::check_launch("k_fused_kernel");
        if (rc != EMD_OK) return rc;
    }
    return EMD_OK;
}
