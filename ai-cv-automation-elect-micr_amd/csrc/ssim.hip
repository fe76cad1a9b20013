// Image-quality metrics on the device: SSIM, MS-SSIM, PSNR and the SSIM loss with its gradient.
// Restates misc_py/denoiser-multi-gpu.py:124-139 (_tf_fspecial_gauss), :142-167 (tf_ssim), :170-192 (tf_ms_ssim) and the
// loss term of _tower_fn (:775).
//
//   emd_ssim_f32                 one launch: tile of x and y (+ halo) into LDS once, horizontal 1-D pass from LDS, vertical
//                                1-D pass on a register ring, ssim / cs formed in registers and reduced; two small launches
//                                add the per-workgroup partial sums per image (one workgroup each), then the per-image
//                                means into the batch mean, in a fixed order, in double
//   emd_ssim_loss_f32            the same launch also writes the three partial-derivative planes Ga, Gb, Gc; a second
//                                kernel applies the full correlation (gather form) and adds scale * dL/dx into dout
//   emd_avgpool2x2_same_c1_f32   tf.nn.avg_pool 2x2 / 2 SAME for one channel (odd extents: the valid elements only)
//   emd_ms_ssim_f32              `level` forward launches and level - 1 pools on one stream + the final product
//   emd_psnr_f32                 squared-difference reduction per image, in double
//
// Images are single-channel and W-contiguous: a lane is a column.  No atomics anywhere: every result is bitwise
// reproducible run to run.
#include "stencil_rows.hpp"

namespace {

constexpr int kTW = 64;        // tile columns = lanes of a wave
constexpr int kWaves = 4;      // a wave owns a strip of rows of the tile
constexpr int kLW = 80;        // LDS row stride in floats: kTW + kMaxSize - 1 = 78, rounded up to whole float4s
constexpr int kFwdSH = 16;     // rows per strip: forward (two planes in LDS)
constexpr int kGradSH = 12;    // ... gradient (three planes in LDS)

constexpr float kC1 = 0.01f * 0.01f;   // (K1 L)^2, L = 1 (:144-148)
constexpr float kC2 = 0.03f * 0.03f;

// Forward: grid (tiles per image, B).  part[(b * tiles + tile) * 2 + {0, 1}] = sums of ssim_map / cs_map over the tile.
// G != NULL: the planes Ga, Gb, Gc (d map / d mu1, d E[xx], d E[xy], times neg_inv_n) at G + {0, 1, 2} * plane.
template <int S, bool VEC>
__global__ __launch_bounds__(256) void ssim_fwd_kernel(const float* __restrict__ x, const float* __restrict__ y, int H, int W, int Hm,
                                                       int Wm, int tiles_x, Taps taps, float neg_inv_n, double* __restrict__ part,
                                                       float* __restrict__ ssim_map, float* __restrict__ cs_map,
                                                       float* __restrict__ G, long plane) {
    constexpr int SH = kFwdSH, TH = kWaves * SH, IR = TH + S - 1, IC = kTW + S - 1;
    __shared__ __attribute__((aligned(16))) float xs[IR * kLW];
    __shared__ __attribute__((aligned(16))) float ys[IR * kLW];
    __shared__ double red[2 * kWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.y, tile = blockIdx.x;
    const int r0 = (tile / tiles_x) * TH, c0 = (tile % tiles_x) * kTW;
    const float* xb = x + (long)b * H * W;
    const float* yb = y + (long)b * H * W;
    if (VEC) {   // W % 4 == 0 and 16-byte aligned images: a float4 is wholly inside a row or wholly outside
        constexpr int NV = kLW / 4;
        for (int i = tid; i < IR * NV; i += 256) {
            const int r = i / NV, v = i - r * NV;
            const int gr = r0 + r, gc = c0 + 4 * v;
            float4 a = make_float4(0.f, 0.f, 0.f, 0.f), c = a;
            if (gr < H && gc < W) {
                a = *reinterpret_cast<const float4*>(xb + (long)gr * W + gc);
                c = *reinterpret_cast<const float4*>(yb + (long)gr * W + gc);
            }
            *reinterpret_cast<float4*>(&xs[r * kLW + 4 * v]) = a;
            *reinterpret_cast<float4*>(&ys[r * kLW + 4 * v]) = c;
        }
    } else {
        for (int i = tid; i < IR * IC; i += 256) {
            const int r = i / IC, c = i - r * IC;
            const int gr = r0 + r, gc = c0 + c;
            float a = 0.f, d = 0.f;
            if (gr < H && gc < W) {
                a = xb[(long)gr * W + gc];
                d = yb[(long)gr * W + gc];
            }
            xs[r * kLW + c] = a;
            ys[r * kLW + c] = d;
        }
    }
    __syncthreads();
    float sum_s = 0.f, sum_c = 0.f;
    const int rs = r0 + wave * SH;   // first map row of this wave's strip
    const int gc = c0 + lane;
    if (rs < Hm) {
        const float* xr = xs + wave * SH * kLW + lane;
        const float* yr = ys + wave * SH * kLW + lane;
        const long mbase = (long)b * Hm * Wm;
        roll_rows<S, SH, 5>(
            taps,
            [&](int i, float* v) {
                float m1 = 0.f, m2 = 0.f, xx = 0.f, yy = 0.f, xy = 0.f;
#pragma unroll
                for (int k = 0; k < S; ++k) {
                    const float a = xr[i * kLW + k], c = yr[i * kLW + k];
                    const float ga = taps.g[k] * a, gb = taps.g[k] * c;
                    m1 = fmaf(taps.g[k], a, m1);
                    m2 = fmaf(taps.g[k], c, m2);
                    xx = fmaf(ga, a, xx);
                    yy = fmaf(gb, c, yy);
                    xy = fmaf(ga, c, xy);
                }
                v[0] = m1, v[1] = m2, v[2] = xx, v[3] = yy, v[4] = xy;
            },
            [&](int o, const float* v) {
                const int gr = rs + o;
                if (gr >= Hm || gc >= Wm) return;
                const float mu1 = v[0], mu2 = v[1];
                const float mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu1_mu2 = mu1 * mu2;
                const float s1 = v[2] - mu1_sq, s2 = v[3] - mu2_sq, s12 = v[4] - mu1_mu2;
                const float A1 = 2.f * mu1_mu2 + kC1, A2 = 2.f * s12 + kC2;
                const float B1 = mu1_sq + mu2_sq + kC1, B2 = s1 + s2 + kC2;
                const float den = B1 * B2;
                const float ssim = (A1 * A2) / den;
                const float cs = A2 / B2;
                sum_s += ssim;
                sum_c += cs;
                const long idx = mbase + (long)gr * Wm + gc;
                if (ssim_map) ssim_map[idx] = ssim;
                if (cs_map) cs_map[idx] = cs;
                if (G) {
                    const float inv = 1.f / den;
                    const float ga = (2.f * mu2 * (A2 - A1) - ssim * 2.f * mu1 * (B2 - B1)) * inv;
                    const float gb = -ssim / B2;
                    const float gcc = 2.f * A1 * inv;
                    G[idx] = neg_inv_n * ga;
                    G[plane + idx] = neg_inv_n * gb;
                    G[2 * plane + idx] = neg_inv_n * gcc;
                }
            });
    }
    const double ws = wave_sum_lane0((double)sum_s), wc = wave_sum_lane0((double)sum_c);
    if (lane == 0) {
        red[2 * wave] = ws;
        red[2 * wave + 1] = wc;
    }
    __syncthreads();
    if (tid == 0) {
        double a = 0.0, c = 0.0;
        for (int w = 0; w < kWaves; ++w) {
            a += red[2 * w];
            c += red[2 * w + 1];
        }
        double* p = part + ((long)b * gridDim.x + tile) * 2;
        p[0] = a;
        p[1] = c;
    }
}

// grid (B): sums[b * NC + c] = scale * (sum over the n partial sums of component c of image b), in a fixed order
template <int NC>
__global__ __launch_bounds__(256) void image_sums_kernel(const double* __restrict__ part, int n, double scale, double* __restrict__ sums) {
    __shared__ double sh[256];
    const int b = blockIdx.x;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const double v = block_sum_fixed(part + (long)b * n * NC + c, n, NC, sh) * scale;
        if (threadIdx.x == 0) sums[(long)b * NC + c] = v;
    }
}

// One workgroup, after image_sums_kernel<2>: the batch mean of the per-image means (fixed order), and the outputs.
// means [B + 1][2] = (ssim, cs), row B the batch.  loss != NULL: loss [B + 1][2] = (mean ssim, 1 - mean ssim) instead.
// acc != NULL: acc[b * acc_stride] += acc_weight * loss_b (per_image) or acc[0] += acc_weight * loss_batch.
__global__ __launch_bounds__(256) void ssim_final_kernel(const double* __restrict__ im, int B, float* __restrict__ means,
                                                         float* __restrict__ loss, float* __restrict__ acc, int acc_stride,
                                                         float acc_weight, int per_image) {
    __shared__ double sh[256];
    const double bs = block_sum_fixed(im, B, 2, sh) / (double)B;
    const double bc = block_sum_fixed(im + 1, B, 2, sh) / (double)B;
    for (int b = threadIdx.x; b <= B; b += 256) {
        const double ms = b < B ? im[2 * b] : bs, mc = b < B ? im[2 * b + 1] : bc;
        if (means) {
            means[2 * b] = (float)ms;
            means[2 * b + 1] = (float)mc;
        }
        if (loss) {
            loss[2 * b] = (float)ms;
            loss[2 * b + 1] = (float)(1.0 - ms);
        }
        if (acc) {
            if (per_image && b < B) acc[(long)b * acc_stride] += acc_weight * (float)(1.0 - ms);
            if (!per_image && b == B) acc[0] += acc_weight * (float)(1.0 - ms);
        }
    }
}

// Gradient: grid (tiles per image over the H x W input domain, B).  dout[q] += s_b * (T[Ga] + 2 x T[Gb] + y T[Gc])(q) with T the
// full correlation: input pixel q gathers the map pixels q - (S - 1) .. q that cover it (zero outside the map).
template <int S>
__global__ __launch_bounds__(256) void ssim_grad_kernel(const float* __restrict__ G, long plane, const float* __restrict__ x,
                                                        const float* __restrict__ y, int H, int W, int Hm, int Wm, int tiles_x,
                                                        Taps taps, float scale, const float* __restrict__ scale_dev,
                                                        float* __restrict__ dout) {
    constexpr int SH = kGradSH, TH = kWaves * SH, IR = TH + S - 1, IC = kTW + S - 1;
    __shared__ float gs[3][IR * kLW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.y, tile = blockIdx.x;
    const int r0 = (tile / tiles_x) * TH, c0 = (tile % tiles_x) * kTW;
    const float* Gb = G + (long)b * Hm * Wm;
    for (int i = tid; i < IR * IC; i += 256) {
        const int r = i / IC, c = i - r * IC;
        const int mr = r0 - (S - 1) + r, mc = c0 - (S - 1) + c;
        float a = 0.f, d = 0.f, e = 0.f;
        if (mr >= 0 && mr < Hm && mc >= 0 && mc < Wm) {
            const long idx = (long)mr * Wm + mc;
            a = Gb[idx];
            d = Gb[plane + idx];
            e = Gb[2 * plane + idx];
        }
        gs[0][r * kLW + c] = a;
        gs[1][r * kLW + c] = d;
        gs[2][r * kLW + c] = e;
    }
    __syncthreads();
    const int rs = r0 + wave * SH;
    const int gc = c0 + lane;
    if (rs >= H) return;
    const float s = scale * (scale_dev ? scale_dev[b] : 1.f);
    const int off = wave * SH * kLW + lane;
    const long ibase = (long)b * H * W;
    roll_rows<S, SH, 3>(
        taps,
        [&](int i, float* v) {
            float a = 0.f, d = 0.f, e = 0.f;
#pragma unroll
            for (int k = 0; k < S; ++k) {
                a = fmaf(taps.g[k], gs[0][off + i * kLW + k], a);
                d = fmaf(taps.g[k], gs[1][off + i * kLW + k], d);
                e = fmaf(taps.g[k], gs[2][off + i * kLW + k], e);
            }
            v[0] = a, v[1] = d, v[2] = e;
        },
        [&](int o, const float* v) {
            const int gr = rs + o;
            if (gr >= H || gc >= W) return;
            const long idx = ibase + (long)gr * W + gc;
            const float g = v[0] + 2.f * x[idx] * v[1] + y[idx] * v[2];
            dout[idx] += s * g;
        });
}

// tf.nn.avg_pool [1,2,2,1] / [1,2,2,1] SAME on one channel, two tensors per launch (x1 may be NULL): [B,H,W] -> [B,ceil(H/2),ceil(W/2)]
__global__ __launch_bounds__(256) void avgpool_c1_kernel(const float* __restrict__ x0, float* __restrict__ y0, const float* __restrict__ x1,
                                                         float* __restrict__ y1, int H, int W, int Ho, int Wo, long n) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int ow = (int)(i % Wo);
    const long t = i / Wo;
    const int oh = (int)(t % Ho);
    const long b = t / Ho;
    const int h0 = 2 * oh, w0 = 2 * ow;
    const bool hw = w0 + 1 < W, hh = h0 + 1 < H;
    const float inv = 1.f / (float)((hw ? 2 : 1) * (hh ? 2 : 1));
    const long base = (b * H + h0) * W + w0;
    for (int k = 0; k < 2; ++k) {
        const float* x = k ? x1 : x0;
        float* y = k ? y1 : y0;
        if (!x) continue;
        float s = x[base];
        if (hw) s += x[base + 1];
        if (hh) {
            float s2 = x[base + W];
            if (hw) s2 += x[base + W + 1];
            s += s2;
        }
        y[i] = s * inv;
    }
}

constexpr int kMaxLevel = 5;
struct MsWeights {
    float w[kMaxLevel];
};

// value[i] = prod_{l < level-1} cs_l ^ w_l * ssim_{level-1} ^ w_{level-1} from lm [level][B + 1][2]; i < B the images, i = B the batch
__global__ void ms_ssim_combine_kernel(const float* __restrict__ lm, int B, int level, MsWeights w, float* __restrict__ value) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i > B) return;
    double v = 1.0;
    for (int l = 0; l < level - 1; ++l) v *= pow((double)lm[((long)l * (B + 1) + i) * 2 + 1], (double)w.w[l]);
    v *= pow((double)lm[((long)(level - 1) * (B + 1) + i) * 2], (double)w.w[level - 1]);
    value[i] = (float)v;   // a negative mean under a fractional power is NaN, as in the reference
}

// grid (nblk, B): part[b * nblk + k] = sum of (x - y)^2 over the k-th slice of image b
__global__ __launch_bounds__(256) void sqdiff_images_kernel(const float* __restrict__ x, const float* __restrict__ y, long npix,
                                                            double* __restrict__ part) {
    __shared__ double red[kWaves];
    const int b = blockIdx.y;
    const float* xb = x + (long)b * npix;
    const float* yb = y + (long)b * npix;
    double s = 0.0;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < npix; i += (long)gridDim.x * 256) {
        const float d = xb[i] - yb[i];
        s += (double)d * (double)d;
    }
    s = wave_sum_lane0(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) part[(long)b * gridDim.x + blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// One workgroup, after image_sums_kernel<1> (im[b] = mse of image b): out [B + 1][2] = (mse, psnr) per image, row B for the batch
// (its mse is the mean of the images')
__global__ __launch_bounds__(256) void psnr_final_kernel(const double* __restrict__ im, int B, double range_sq, float* __restrict__ out) {
    __shared__ double sh[256];
    const double bm = block_sum_fixed(im, B, 1, sh) / (double)B;
    for (int b = threadIdx.x; b <= B; b += 256) {
        const double mse = b < B ? im[b] : bm;
        out[2 * b] = (float)mse;
        out[2 * b + 1] = (float)(10.0 * log10(range_sq / mse));   // mse == 0: inf
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------------

int check_window(const char* who, const float* taps_host, int size, int H, int W, Taps* t) {
    if (!taps_host) {
        emd::set_error("%s: null pointer (taps_host)", who);
        return EMD_E_INVALID;
    }
    if (size < 3 || size > kMaxSize || size % 2 == 0) {
        emd::set_error("%s: window size must be odd, 3..%d (got %d)", who, kMaxSize, size);
        return EMD_E_INVALID;
    }
    if (H < size || W < size) {
        emd::set_error("%s: image %d x %d is smaller than the %d x %d window", who, H, W, size, size);
        return EMD_E_INVALID;
    }
    for (int k = 0; k < kMaxSize; ++k) t->g[k] = k < size ? taps_host[k] : 0.f;
    return EMD_OK;
}

bool fwd_vec_ok(const float* x, const float* y, int W) { return W % 4 == 0 && emd::aligned16(x) && emd::aligned16(y); }

size_t fwd_part_bytes(int B, int H, int W, int size) {
    const int Hm = H - size + 1, Wm = W - size + 1;
    return emd::round256((size_t)B * emd::tiles_of(Hm, kWaves * kFwdSH) * emd::tiles_of(Wm, kTW) * 2 * sizeof(double));
}
// the whole forward workspace: [per-tile partial sums] [per-image means, double [B][2]]
size_t fwd_ws_bytes(int B, int H, int W, int size) { return fwd_part_bytes(B, H, W, size) + emd::round256((size_t)B * 2 * sizeof(double)); }

template <int S>
void launch_fwd_s(bool vec, dim3 grid, hipStream_t st, const float* x, const float* y, int H, int W, int Hm, int Wm, int tiles_x,
                  const Taps& t, float neg_inv_n, double* part, float* ssim_map, float* cs_map, float* G, long plane) {
    if (vec)
        hipLaunchKernelGGL((ssim_fwd_kernel<S, true>), grid, dim3(256), 0, st, x, y, H, W, Hm, Wm, tiles_x, t, neg_inv_n, part, ssim_map,
                           cs_map, G, plane);
    else
        hipLaunchKernelGGL((ssim_fwd_kernel<S, false>), grid, dim3(256), 0, st, x, y, H, W, Hm, Wm, tiles_x, t, neg_inv_n, part, ssim_map,
                           cs_map, G, plane);
}

// the tile launch; the caller has validated everything (size odd in 3..15, H, W >= size, 1 <= B <= 65535)
int launch_fwd(const float* x, const float* y, int B, int H, int W, const Taps& t, int size, double* part, float* ssim_map,
               float* cs_map, float* G, hipStream_t st, int* tiles_out) {
    const int Hm = H - size + 1, Wm = W - size + 1;
    const int tiles_x = emd::tiles_of(Wm, kTW), tiles = tiles_x * emd::tiles_of(Hm, kWaves * kFwdSH);
    const dim3 grid((unsigned)tiles, (unsigned)B);
    const bool vec = fwd_vec_ok(x, y, W);
    const float neg_inv_n = (float)(-1.0 / ((double)Hm * Wm));
    const long plane = (long)B * Hm * Wm;
#define EMD_SSIM_CASE(SZ) \
    case SZ:              \
        launch_fwd_s<SZ>(vec, grid, st, x, y, H, W, Hm, Wm, tiles_x, t, neg_inv_n, part, ssim_map, cs_map, G, plane); \
        break;
    switch (size) {
        EMD_SSIM_CASE(3)
        EMD_SSIM_CASE(5)
        EMD_SSIM_CASE(7)
        EMD_SSIM_CASE(9)
        EMD_SSIM_CASE(11)
        EMD_SSIM_CASE(13)
        EMD_SSIM_CASE(15)
    }
#undef EMD_SSIM_CASE
    *tiles_out = tiles;
    return emd::check_launch("ssim_fwd_kernel");
}

int launch_final(const double* part, double* im, int B, int tiles, int Hm, int Wm, float* means, float* loss, float* acc, int acc_stride,
                 float acc_weight, int per_image, hipStream_t st) {
    hipLaunchKernelGGL(image_sums_kernel<2>, dim3((unsigned)B), dim3(256), 0, st, part, tiles, 1.0 / ((double)Hm * Wm), im);
    hipLaunchKernelGGL(ssim_final_kernel, dim3(1), dim3(256), 0, st, static_cast<const double*>(im), B, means, loss, acc, acc_stride,
                       acc_weight, per_image);
    return emd::check_launch("ssim_final_kernel");
}

int launch_pool(const float* x0, float* y0, const float* x1, float* y1, int B, int H, int W, hipStream_t st) {
    const int Ho = (H + 1) / 2, Wo = (W + 1) / 2;
    const long n = (long)B * Ho * Wo;
    const long nb = (n + 255) / 256;
    if (nb > 0x7fffffffL) return emd::fail(EMD_E_INVALID, "emd_avgpool2x2_same_c1_f32: tensor too large");
    hipLaunchKernelGGL(avgpool_c1_kernel, dim3((unsigned)nb), dim3(256), 0, st, x0, y0, x1, y1, H, W, Ho, Wo, n);
    return emd::check_launch("avgpool_c1_kernel");
}

const MsWeights kMsWeights = {{0.0448f, 0.2856f, 0.3001f, 0.2363f, 0.1333f}};   // :171

}  // namespace

extern "C" size_t emd_ssim_workspace_bytes(int B, int H, int W, int size) {
    if (B < 1 || size < 3 || size > kMaxSize || size % 2 == 0 || H < size || W < size) return 0;
    return fwd_ws_bytes(B, H, W, size);
}

extern "C" int emd_ssim_f32(const float* x, const float* y, int B, int H, int W, const float* taps_host, int size, float* means,
                            float* ssim_map, float* cs_map, void* workspace, size_t workspace_bytes, emd_stream_t stream) {
    EMD_REQUIRE(x && y && means && workspace, EMD_E_INVALID, "emd_ssim_f32: null pointer");
    EMD_REQUIRE(B >= 0 && B <= 65535, EMD_E_INVALID, "emd_ssim_f32: batch must be 0..65535");
    Taps t;
    int rc = check_window("emd_ssim_f32", taps_host, size, H, W, &t);
    if (rc != EMD_OK) return rc;
    if (B == 0) return EMD_OK;
    EMD_REQUIRE(workspace_bytes >= emd_ssim_workspace_bytes(B, H, W, size), EMD_E_INVALID, "emd_ssim_f32: workspace too small");
    EMD_REQUIRE(emd::aligned16(workspace), EMD_E_ALIGN, "emd_ssim_f32: workspace must be 16-byte aligned");
    hipStream_t st = static_cast<hipStream_t>(stream);
    int tiles;
    rc = launch_fwd(x, y, B, H, W, t, size, static_cast<double*>(workspace), ssim_map, cs_map, nullptr, st, &tiles);
    if (rc != EMD_OK) return rc;
    double* im = reinterpret_cast<double*>(static_cast<char*>(workspace) + fwd_part_bytes(B, H, W, size));
    return launch_final(static_cast<const double*>(workspace), im, B, tiles, H - size + 1, W - size + 1, means, nullptr, nullptr, 0, 0.f, 0, st);
}

extern "C" size_t emd_ssim_loss_workspace_bytes(int B, int H, int W, int size) {
    if (B < 1 || size < 3 || size > kMaxSize || size % 2 == 0 || H < size || W < size) return 0;
    return fwd_ws_bytes(B, H, W, size) + emd::round256((size_t)3 * B * (H - size + 1) * (W - size + 1) * sizeof(float));
}

extern "C" int emd_ssim_loss_f32(const float* x, const float* y, int B, int H, int W, const float* taps_host, int size, int per_image,
                                 float scale, const float* scale_dev, float* dout, float* result, float* loss_acc, int acc_stride,
                                 float acc_weight, void* workspace, size_t workspace_bytes, emd_stream_t stream) {
    EMD_REQUIRE(x && y && result && workspace, EMD_E_INVALID, "emd_ssim_loss_f32: null pointer");
    EMD_REQUIRE(B >= 0 && B <= 65535, EMD_E_INVALID, "emd_ssim_loss_f32: batch must be 0..65535");
    Taps t;
    int rc = check_window("emd_ssim_loss_f32", taps_host, size, H, W, &t);
    if (rc != EMD_OK) return rc;
    for (int k = 0; k < size / 2; ++k)
        EMD_REQUIRE(t.g[k] == t.g[size - 1 - k], EMD_E_INVALID, "emd_ssim_loss_f32: the window taps must be symmetric");
    EMD_REQUIRE(!loss_acc || acc_stride >= 1, EMD_E_INVALID, "emd_ssim_loss_f32: acc_stride must be >= 1");
    if (dout && H >= 1 && W >= 1 && B >= 1) {
        const size_t n = (size_t)B * H * W * sizeof(float);
        EMD_REQUIRE(!emd::overlap(dout, n, x, n) && !emd::overlap(dout, n, y, n), EMD_E_INVALID, "emd_ssim_loss_f32: dout may not alias x or y");
    }
    if (B == 0) return EMD_OK;
    EMD_REQUIRE(workspace_bytes >= emd_ssim_loss_workspace_bytes(B, H, W, size), EMD_E_INVALID, "emd_ssim_loss_f32: workspace too small");
    EMD_REQUIRE(emd::aligned16(workspace), EMD_E_ALIGN, "emd_ssim_loss_f32: workspace must be 16-byte aligned");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int Hm = H - size + 1, Wm = W - size + 1;
    double* part = static_cast<double*>(workspace);
    double* im = reinterpret_cast<double*>(static_cast<char*>(workspace) + fwd_part_bytes(B, H, W, size));
    float* G = dout ? reinterpret_cast<float*>(static_cast<char*>(workspace) + fwd_ws_bytes(B, H, W, size)) : nullptr;
    int tiles;
    rc = launch_fwd(x, y, B, H, W, t, size, part, nullptr, nullptr, G, st, &tiles);
    if (rc != EMD_OK) return rc;
    rc = launch_final(part, im, B, tiles, Hm, Wm, nullptr, result, loss_acc, acc_stride, acc_weight, per_image ? 1 : 0, st);
    if (rc != EMD_OK || !dout) return rc;
    const int tiles_x = emd::tiles_of(W, kTW);
    const dim3 grid((unsigned)(tiles_x * emd::tiles_of(H, kWaves * kGradSH)), (unsigned)B);
    const float s = per_image ? scale : scale / (float)B;   // the batch mean's gradient: 1 / B of each image's
    const long plane = (long)B * Hm * Wm;
#define EMD_SSIM_CASE(SZ) \
    case SZ:              \
        hipLaunchKernelGGL((ssim_grad_kernel<SZ>), grid, dim3(256), 0, st, G, plane, x, y, H, W, Hm, Wm, tiles_x, t, s, scale_dev, dout); \
        break;
    switch (size) {
        EMD_SSIM_CASE(3)
        EMD_SSIM_CASE(5)
        EMD_SSIM_CASE(7)
        EMD_SSIM_CASE(9)
        EMD_SSIM_CASE(11)
        EMD_SSIM_CASE(13)
        EMD_SSIM_CASE(15)
    }
#undef EMD_SSIM_CASE
    return emd::check_launch("ssim_grad_kernel");
}

extern "C" int emd_avgpool2x2_same_c1_f32(const float* x, float* y, int B, int H, int W, emd_stream_t stream) {
    EMD_REQUIRE(x && y, EMD_E_INVALID, "emd_avgpool2x2_same_c1_f32: null pointer");
    EMD_REQUIRE(B >= 0 && H >= 1 && W >= 1, EMD_E_INVALID, "emd_avgpool2x2_same_c1_f32: bad shape");
    EMD_REQUIRE(x != y, EMD_E_INVALID, "emd_avgpool2x2_same_c1_f32: y may not alias x");
    if (B == 0) return EMD_OK;
    return launch_pool(x, y, nullptr, nullptr, B, H, W, static_cast<hipStream_t>(stream));
}

namespace {
// workspace of emd_ms_ssim_f32: [partials of level 0 (the largest) and per-image means] [level means] [x, y of levels 1 .. level-1]
struct MsLayout {
    size_t part, means, pooled[kMaxLevel], total;
    int h[kMaxLevel], w[kMaxLevel];
};
MsLayout ms_layout(int B, int H, int W, int level, int size) {
    MsLayout L{};
    L.part = 0;
    L.means = fwd_ws_bytes(B, H, W, size);
    size_t off = L.means + emd::round256((size_t)level * (B + 1) * 2 * sizeof(float));
    L.h[0] = H, L.w[0] = W;
    for (int l = 1; l < level; ++l) {
        L.h[l] = (L.h[l - 1] + 1) / 2, L.w[l] = (L.w[l - 1] + 1) / 2;
        L.pooled[l] = off;
        off += 2 * emd::round256((size_t)B * L.h[l] * L.w[l] * sizeof(float));
    }
    L.total = off;
    return L;
}
bool ms_args_ok(int B, int H, int W, int level, int size) {
    if (B < 1 || level < 1 || level > kMaxLevel || size < 3 || size > kMaxSize || size % 2 == 0) return false;
    const long need = (long)size << (level - 1);   // then every level's image holds a window (the stated rule, also where SAME pooling would round up)
    return H >= need && W >= need;
}
}  // namespace

extern "C" size_t emd_ms_ssim_workspace_bytes(int B, int H, int W, int level, int size) {
    return ms_args_ok(B, H, W, level, size) ? ms_layout(B, H, W, level, size).total : 0;
}

extern "C" int emd_ms_ssim_f32(const float* x, const float* y, int B, int H, int W, int level, const float* taps_host, int size,
                               float* value, float* level_means, void* workspace, size_t workspace_bytes, emd_stream_t stream) {
    EMD_REQUIRE(x && y && value && workspace, EMD_E_INVALID, "emd_ms_ssim_f32: null pointer");
    EMD_REQUIRE(B >= 0 && B <= 65535, EMD_E_INVALID, "emd_ms_ssim_f32: batch must be 0..65535");
    EMD_REQUIRE(level >= 1 && level <= kMaxLevel, EMD_E_INVALID, "emd_ms_ssim_f32: level must be 1..5");
    Taps t;
    int rc = check_window("emd_ms_ssim_f32", taps_host, size, H, W, &t);
    if (rc != EMD_OK) return rc;
    if (!ms_args_ok(B > 0 ? B : 1, H, W, level, size)) {
        emd::set_error("emd_ms_ssim_f32: image %d x %d is too small for %d levels of a %d x %d window (needs >= %d)", H, W, level, size, size,
                       size << (level - 1));
        return EMD_E_INVALID;
    }
    if (B == 0) return EMD_OK;
    const MsLayout L = ms_layout(B, H, W, level, size);
    EMD_REQUIRE(workspace_bytes >= L.total, EMD_E_INVALID, "emd_ms_ssim_f32: workspace too small");
    EMD_REQUIRE(emd::aligned16(workspace), EMD_E_ALIGN, "emd_ms_ssim_f32: workspace must be 16-byte aligned");
    hipStream_t st = static_cast<hipStream_t>(stream);
    char* ws = static_cast<char*>(workspace);
    double* part = reinterpret_cast<double*>(ws + L.part);
    double* im = reinterpret_cast<double*>(ws + L.part + fwd_part_bytes(B, H, W, size));   // every level: B x 2 doubles
    float* lm = level_means ? level_means : reinterpret_cast<float*>(ws + L.means);
    const float *cx = x, *cy = y;
    for (int l = 0; l < level; ++l) {
        int tiles;
        rc = launch_fwd(cx, cy, B, L.h[l], L.w[l], t, size, part, nullptr, nullptr, nullptr, st, &tiles);
        if (rc != EMD_OK) return rc;
        rc = launch_final(part, im, B, tiles, L.h[l] - size + 1, L.w[l] - size + 1, lm + (size_t)l * (B + 1) * 2, nullptr, nullptr, 0, 0.f, 0, st);
        if (rc != EMD_OK) return rc;
        if (l + 1 < level) {
            float* nx = reinterpret_cast<float*>(ws + L.pooled[l + 1]);
            float* ny = reinterpret_cast<float*>(ws + L.pooled[l + 1] + emd::round256((size_t)B * L.h[l + 1] * L.w[l + 1] * sizeof(float)));
            rc = launch_pool(cx, nx, cy, ny, B, L.h[l], L.w[l], st);
            if (rc != EMD_OK) return rc;
            cx = nx, cy = ny;
        }
    }
    hipLaunchKernelGGL(ms_ssim_combine_kernel, dim3((unsigned)((B + 1 + 63) / 64)), dim3(64), 0, st, lm, B, level, kMsWeights, value);
    return emd::check_launch("ms_ssim_combine_kernel");
}

namespace {
int psnr_blocks(long npix) {
    long n = (npix + 256 * 8 - 1) / (256 * 8);
    return (int)(n < 1 ? 1 : (n > 256 ? 256 : n));
}
}  // namespace

extern "C" size_t emd_psnr_workspace_bytes(int B, long npix) {
    if (B < 1 || npix < 1) return 0;
    return emd::round256((size_t)B * psnr_blocks(npix) * sizeof(double)) + emd::round256((size_t)B * sizeof(double));
}

extern "C" int emd_psnr_f32(const float* x, const float* y, int B, long npix, float data_range, float* out, void* workspace,
                            size_t workspace_bytes, emd_stream_t stream) {
    EMD_REQUIRE(x && y && out && workspace, EMD_E_INVALID, "emd_psnr_f32: null pointer");
    EMD_REQUIRE(B >= 0 && B <= 65535 && npix >= 1, EMD_E_INVALID, "emd_psnr_f32: bad shape (batch 0..65535, npix >= 1)");
    EMD_REQUIRE(data_range > 0.f, EMD_E_INVALID, "emd_psnr_f32: data_range must be positive");
    if (B == 0) return EMD_OK;
    EMD_REQUIRE(workspace_bytes >= emd_psnr_workspace_bytes(B, npix), EMD_E_INVALID, "emd_psnr_f32: workspace too small");
    EMD_REQUIRE(emd::aligned16(workspace), EMD_E_ALIGN, "emd_psnr_f32: workspace must be 16-byte aligned");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int nblk = psnr_blocks(npix);
    hipLaunchKernelGGL(sqdiff_images_kernel, dim3((unsigned)nblk, (unsigned)B), dim3(256), 0, st, x, y, npix, static_cast<double*>(workspace));
    double* im = reinterpret_cast<double*>(static_cast<char*>(workspace) + emd::round256((size_t)B * nblk * sizeof(double)));
    hipLaunchKernelGGL(image_sums_kernel<1>, dim3((unsigned)B), dim3(256), 0, st, static_cast<const double*>(workspace), nblk, 1.0 / (double)npix, im);
    hipLaunchKernelGGL(psnr_final_kernel, dim3(1), dim3(256), 0, st, static_cast<const double*>(im), B,
                       (double)data_range * (double)data_range, out);
    return emd::check_launch("psnr_final_kernel");
}
