// Classical baseline filters on the device: what a microscopist would use instead of the networks, for the
// reference's comparison table (misc_py/err_hist_maker.py:26-45: methods Gaussian, Bilateral, Median, Wiener, Chambolle) and its
// ground-truth blur (misc_py/blur_images.py:13).
//
//   emd_filter_gaussian_f32    one launch: tile + halo into LDS, horizontal 1-D pass from LDS, vertical pass on a register ring
//   emd_filter_median_f32      3x3 / 5x5: forgetful selection by min/max exchanges in registers (no sort, no branch on data)
//   emd_filter_bilateral_f32   circular support of diameter d; the spatial weights come in as a kernel argument, the range
//                              weight is one v_exp_f32 with the constant folded
//   emd_filter_wiener_f32      scipy.signal.wiener: mean, then variance about that mean, of each window of the zero-padded image,
//                              read from LDS; with an estimated noise power a first launch leaves per-tile sums of the local
//                              variance (double, fixed order) and the second adds them per image and applies
//   emd_filter_tv_f32          Chambolle's dual projection, one launch per iteration on ping-pong dual planes
//   emd_filter_clip01_f32      min(max(x, 0), 1), what the comparison table applies before scoring when asked to
//
// Images are single-channel float32 [B,H,W], W-contiguous; a tile is 64 columns (a lane is a column) by four strips of rows
// (a wave owns a strip).  "Mirror" is reflect-101 (emd::reflect); no atomics: every result is bitwise reproducible.
#include <climits>
#include <cmath>

#include "f4_math.hpp"
#include "stencil_rows.hpp"

namespace {

using emd::reflect;

constexpr int kTW = 64;      // tile columns = lanes of a wave
constexpr int kWaves = 4;    // a wave owns a strip of rows of the tile
constexpr float kLog2e = 1.4426950408889634f;

// The tile rows r0 - R .. r0 - R + IR - 1 and columns c0 - R .. c0 - R + IC - 1 of one image into xs (row stride IC).  MIRROR: the
// mirrored pixel outside the image (needs R < min(H, W)); a position further out than the mirror reaches is past every pixel the
// tile writes and takes an edge pixel.  !MIRROR: zero outside the image.
template <bool MIRROR>
__device__ __forceinline__ void load_tile(float* __restrict__ xs, const float* __restrict__ xb, int H, int W, int r0, int c0, int R,
                                          int IR, int IC) {
    for (int i = threadIdx.x; i < IR * IC; i += 256) {
        const int r = i / IC, c = i - r * IC;
        int gr = r0 - R + r, gc = c0 - R + c;
        float v = 0.f;
        if (MIRROR) {
            gr = min(max(reflect(gr, H), 0), H - 1);
            gc = min(max(reflect(gc, W), 0), W - 1);
            v = xb[(long)gr * W + gc];
        } else if (gr >= 0 && gr < H && gc >= 0 && gc < W) {
            v = xb[(long)gr * W + gc];
        }
        xs[i] = v;
    }
}

struct TileId {
    int r0, c0, lane, wave;
    long base;   // offset of the image
};
template <int TH>
__device__ __forceinline__ TileId tile_id(int tiles_x, int H, int W) {
    TileId t;
    const int tile = blockIdx.x;
    t.r0 = (tile / tiles_x) * TH;
    t.c0 = (tile % tiles_x) * kTW;
    t.lane = threadIdx.x & 63;
    t.wave = threadIdx.x >> 6;
    t.base = (long)blockIdx.y * H * W;
    return t;
}

// ---- Gaussian: grid (tiles, B) ------------------------------------------------------------------------------------------
constexpr int kGaussSH = 16;
template <int S>
__global__ __launch_bounds__(256) void filter_gaussian_kernel(const float* __restrict__ x, float* __restrict__ out, int H, int W,
                                                              int tiles_x, Taps taps) {
    constexpr int R = S / 2, SH = kGaussSH, TH = kWaves * SH, IR = TH + S - 1, IC = kTW + S - 1;
    __shared__ float xs[IR * IC];
    const TileId t = tile_id<TH>(tiles_x, H, W);
    load_tile<true>(xs, x + t.base, H, W, t.r0, t.c0, R, IR, IC);
    __syncthreads();
    const int rs = t.r0 + t.wave * SH, gc = t.c0 + t.lane;
    if (rs >= H) return;
    const float* xr = xs + t.wave * SH * IC + t.lane;
    roll_rows<S, SH, 1>(
        taps,
        [&](int i, float* v) {
            float a = 0.f;
#pragma unroll
            for (int k = 0; k < S; ++k) a = fmaf(taps.g[k], xr[i * IC + k], a);
            v[0] = a;
        },
        [&](int o, const float* v) {
            const int gr = rs + o;
            if (gr < H && gc < W) out[t.base + (long)gr * W + gc] = v[0];
        });
}

// ---- median: grid (tiles, B) --------------------------------------------------------------------------------------------
__device__ __forceinline__ void cx(float& a, float& b) {   // a <= b afterwards
    const float lo = fminf(a, b), hi = fmaxf(a, b);
    a = lo;
    b = hi;
}
// the smallest of a[0 .. K-1] to a[0] and the largest to a[K-1]
template <int K>
__device__ __forceinline__ void min_max_to_ends(float* a) {
#pragma unroll
    for (int i = 0; i < K / 2; ++i) cx(a[i], a[K - 1 - i]);
#pragma unroll
    for (int i = 1; i < (K + 1) / 2; ++i) cx(a[0], a[i]);
#pragma unroll
    for (int i = K / 2; i < K - 1; ++i) cx(a[i], a[K - 1]);
}
// Forgetful selection of the median of v[0 .. N-1], N odd: of any N/2 + 2 of the values neither the smallest nor the largest is the
// median; drop both, take the next value in, and again, down to three.
template <int K, int N>
struct Forget {
    static __device__ __forceinline__ float run(float* a, const float* v) {
        min_max_to_ends<K>(a);
        if constexpr (K == 3) {
            return a[1];
        } else {
            constexpr int K0 = N / 2 + 2;
            a[0] = v[K0 + (K0 - K)];   // over the minimum; the maximum a[K-1] drops out of the set a[0 .. K-2]
            return Forget<K - 1, N>::run(a, v);
        }
    }
};
template <int N>
__device__ __forceinline__ float median_of(const float* v) {
    constexpr int K0 = N / 2 + 2;
    float a[K0];
#pragma unroll
    for (int i = 0; i < K0; ++i) a[i] = v[i];
    return Forget<K0, N>::run(a, v);
}

constexpr int kSmallSH = 8;   // rows per strip of the kernels that read their whole window from LDS per pixel
template <int K>
__global__ __launch_bounds__(256) void filter_median_kernel(const float* __restrict__ x, float* __restrict__ out, int H, int W,
                                                            int tiles_x) {
    constexpr int R = K / 2, SH = kSmallSH, TH = kWaves * SH, IR = TH + K - 1, IC = kTW + K - 1;
    __shared__ float xs[IR * IC];
    const TileId t = tile_id<TH>(tiles_x, H, W);
    load_tile<true>(xs, x + t.base, H, W, t.r0, t.c0, R, IR, IC);
    __syncthreads();
    const int rs = t.r0 + t.wave * SH, gc = t.c0 + t.lane;
    if (rs >= H || gc >= W) return;
    const float* xr = xs + t.wave * SH * IC + t.lane;
#pragma unroll 2
    for (int o = 0; o < SH; ++o) {
        const int gr = rs + o;
        if (gr >= H) break;
        float v[K * K];
#pragma unroll
        for (int i = 0; i < K; ++i) {
#pragma unroll
            for (int j = 0; j < K; ++j) v[i * K + j] = xr[(o + i) * IC + j];
        }
        out[t.base + (long)gr * W + gc] = median_of<K * K>(v);
    }
}

// ---- bilateral: grid (tiles, B) -----------------------------------------------------------------------------------------
constexpr int kMaxD = 9;
struct SpaceWeights {
    float w[kMaxD * kMaxD];   // [(dy + r) * d + dx + r] = exp(-(dx^2 + dy^2) / (2 sigma_space^2)); 0 outside the disc
};
// neg_c = -log2(e) / (2 sigma_color^2): the range weight is exp2(neg_c * (x[q] - x[p])^2)
template <int R>
__global__ __launch_bounds__(256) void filter_bilateral_kernel(const float* __restrict__ x, float* __restrict__ out, int H, int W,
                                                               int tiles_x, SpaceWeights sw, float neg_c) {
    constexpr int D = 2 * R + 1, SH = kSmallSH, TH = kWaves * SH, IR = TH + D - 1, IC = kTW + D - 1;
    __shared__ float xs[IR * IC];
    const TileId t = tile_id<TH>(tiles_x, H, W);
    load_tile<true>(xs, x + t.base, H, W, t.r0, t.c0, R, IR, IC);
    __syncthreads();
    const int rs = t.r0 + t.wave * SH, gc = t.c0 + t.lane;
    if (rs >= H || gc >= W) return;
    const float* xr = xs + t.wave * SH * IC + t.lane;
    for (int o = 0; o < SH; ++o) {
        const int gr = rs + o;
        if (gr >= H) break;
        const float c = xr[(o + R) * IC + R];
        float num = 0.f, den = 0.f;
#pragma unroll
        for (int i = 0; i < D; ++i) {
#pragma unroll
            for (int j = 0; j < D; ++j) {
                if ((i - R) * (i - R) + (j - R) * (j - R) <= R * R) {
                    const float q = xr[(o + i) * IC + j];
                    const float df = q - c;
                    const float w = sw.w[i * D + j] * __builtin_amdgcn_exp2f(neg_c * (df * df));
                    num = fmaf(w, q, num);
                    den += w;
                }
            }
        }
        out[t.base + (long)gr * W + gc] = num / den;   // den >= the centre's weight, 1
    }
}

// ---- Wiener: grid (tiles, B) --------------------------------------------------------------------------------------------
// MODE 0: the noise power is the argument; 1: only the per-tile sum of the local variance, part[b * tiles + tile]; 2: the noise
// power of image b is the mean of its local variance, summed here from part in a fixed order, then as 0.
constexpr int kWienerSH = 16;
template <int S, int MODE>
__global__ __launch_bounds__(256) void filter_wiener_kernel(const float* __restrict__ x, float* __restrict__ out, int H, int W,
                                                            int tiles_x, float noise, double* __restrict__ part,
                                                            float* __restrict__ noise_out) {
    constexpr int R = S / 2, SH = kWienerSH, TH = kWaves * SH, IR = TH + S - 1, IC = kTW + S - 1;
    __shared__ float xs[IR * IC];
    __shared__ double sh[MODE == 2 ? 256 : kWaves];
    const TileId t = tile_id<TH>(tiles_x, H, W);
    const float* xb = x + t.base;
    load_tile<false>(xs, xb, H, W, t.r0, t.c0, R, IR, IC);
    float n = noise;
    if (MODE == 2) {
        n = (float)(block_sum_fixed(part + (long)blockIdx.y * gridDim.x, (int)gridDim.x, 1, sh) / ((double)H * W));
    }
    __syncthreads();
    if (MODE != 1 && noise_out && blockIdx.x == 0 && threadIdx.x == 0) noise_out[blockIdx.y] = n;
    const int rs = t.r0 + t.wave * SH, gc = t.c0 + t.lane;
    const float inv = 1.f / (float)(S * S);
    double vsum = 0.0;
    if (rs < H && gc < W) {
        const float* xr = xs + t.wave * SH * IC + t.lane;
        for (int o = 0; o < SH; ++o) {
            const int gr = rs + o;
            if (gr >= H) break;
            // E[x^2] - m^2 cancels, so the variance is taken in a second pass over the window, of x - m; the mean is formed around
            // the window's own centre pixel c (a constant window gives c back exactly).  A padding zero is a value like any other:
            // a pixel's bits depend neither on where the tile grid falls nor on whether a zero is padding or data.
            const float c = xr[(o + R) * IC + R];
            float s1 = 0.f;
#pragma unroll
            for (int i = 0; i < S; ++i) {
#pragma unroll
                for (int j = 0; j < S; ++j) s1 += xr[(o + i) * IC + j] - c;
            }
            const float m = fmaf(s1, inv, c);
            float s2 = 0.f;
#pragma unroll
            for (int i = 0; i < S; ++i) {
#pragma unroll
                for (int j = 0; j < S; ++j) {
                    const float a = xr[(o + i) * IC + j] - m;
                    s2 = fmaf(a, a, s2);
                }
            }
            const float var = s2 * inv;
            if (MODE == 1) {
                vsum += (double)var;
            } else {
                // scipy: where(var < n, m, res); var == 0 (then n == 0 too) would be 0 / 0: the mean as well
                const float res = fmaf(c - m, 1.f - n / var, m);
                out[t.base + (long)gr * W + gc] = (var >= n && var > 0.f) ? res : m;
            }
        }
    }
    if (MODE == 1) {
        vsum = wave_sum_lane0(vsum);
        if (t.lane == 0) sh[t.wave] = vsum;
        __syncthreads();
        if (threadIdx.x == 0) part[(long)blockIdx.y * gridDim.x + blockIdx.x] = ((sh[0] + sh[1]) + sh[2]) + sh[3];
    }
}

// ---- Chambolle total variation: one iteration; grid (tiles, B) -----------------------------------------------------------
// u = x + div p from the dual planes pin (first: p = 0, nothing is read); last: out = u; else pout = the projected step.
__global__ __launch_bounds__(256) void filter_tv_kernel(const float* __restrict__ x, const float* __restrict__ pin1,
                                                        const float* __restrict__ pin2, float* __restrict__ pout1,
                                                        float* __restrict__ pout2, float* __restrict__ out, int H, int W, int tiles_x,
                                                        float tau, float tau_over_weight, int first, int last) {
    constexpr int SH = kSmallSH, TH = kWaves * SH, IR = TH + 2, IC = kTW + 2;
    __shared__ float xs[IR * IC];
    __shared__ float p1[IR * IC];
    __shared__ float p2[IR * IC];
    const TileId t = tile_id<TH>(tiles_x, H, W);
    load_tile<false>(xs, x + t.base, H, W, t.r0, t.c0, 1, IR, IC);
    if (first) {
        for (int i = threadIdx.x; i < IR * IC; i += 256) p1[i] = 0.f, p2[i] = 0.f;
    } else {
        load_tile<false>(p1, pin1 + t.base, H, W, t.r0, t.c0, 1, IR, IC);
        load_tile<false>(p2, pin2 + t.base, H, W, t.r0, t.c0, 1, IR, IC);
    }
    __syncthreads();
    const int rs = t.r0 + t.wave * SH, gc = t.c0 + t.lane;
    if (rs >= H || gc >= W) return;
    // u at tile position (r, c): the terms outside the image are the zeros of the border
    auto u_at = [&](int r, int c) {
        const int i = (r + 1) * IC + c + 1;
        return xs[i] + (((-p1[i] - p2[i]) + p1[i - IC]) + p2[i - 1]);
    };
    for (int o = 0; o < SH; ++o) {
        const int gr = rs + o, lr = t.wave * SH + o;
        if (gr >= H) break;
        const long idx = t.base + (long)gr * W + gc;
        const float u = u_at(lr, t.lane);
        if (last) {
            out[idx] = u;
            continue;
        }
        const float g1 = gr + 1 < H ? u_at(lr + 1, t.lane) - u : 0.f;
        const float g2 = gc + 1 < W ? u_at(lr, t.lane + 1) - u : 0.f;
        const float den = fmaf(tau_over_weight, sqrtf(fmaf(g1, g1, g2 * g2)), 1.f);
        const int i = (lr + 1) * IC + t.lane + 1;
        pout1[idx] = fmaf(-tau, g1, p1[i]) / den;
        pout2[idx] = fmaf(-tau, g2, p2[i]) / den;
    }
}

// ---- clip to [0, 1]: element-wise, in place or not
__global__ __launch_bounds__(256) void filter_clip01_kernel(const float* __restrict__ x, float* __restrict__ out, long n) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) out[i] = fminf(fmaxf(x[i], 0.f), 1.f);
}

// ---- host side -----------------------------------------------------------------------------------------------------------

// what every filter checks first: pointers, the batch, the extents (a grid of TH-row tiles must fit) and that out is not x
int check_images(const char* who, const float* x, const float* out, int B, int H, int W, int TH) {
    if (!x || !out) {
        emd::set_error("%s: null pointer", who);
        return EMD_E_INVALID;
    }
    if (B < 0 || B > 65535 || H < 1 || W < 1 || (long)emd::tiles_of(H, TH) * emd::tiles_of(W, kTW) > INT_MAX) {
        emd::set_error("%s: bad shape (batch 0..65535, H, W >= 1; got %d x %d x %d)", who, B, H, W);
        return EMD_E_INVALID;
    }
    if (B > 0 && emd::overlap(x, (size_t)B * H * W * sizeof(float), out, (size_t)B * H * W * sizeof(float))) {
        emd::set_error("%s: out may not alias x (a tile reads its neighbours' pixels)", who);
        return EMD_E_INVALID;
    }
    return EMD_OK;
}

int check_mirror(const char* who, int radius, int H, int W) {
    if (H <= radius || W <= radius) {
        emd::set_error("%s: the mirror border needs radius < min(H,W) (radius %d, image %d x %d)", who, radius, H, W);
        return EMD_E_INVALID;
    }
    return EMD_OK;
}

dim3 grid_of(int B, int H, int W, int TH, int* tiles_x) {
    *tiles_x = emd::tiles_of(W, kTW);
    return dim3((unsigned)(*tiles_x * emd::tiles_of(H, TH)), (unsigned)B);
}

constexpr int kWienerTH = kWaves * kWienerSH, kSmallTH = kWaves * kSmallSH, kGaussTH = kWaves * kGaussSH;

bool wiener_size_ok(int ksize) { return ksize >= 3 && ksize <= 9 && ksize % 2 == 1; }
size_t wiener_ws_bytes(int B, int H, int W) {
    return emd::round256((size_t)B * emd::tiles_of(H, kWienerTH) * emd::tiles_of(W, kTW) * sizeof(double));
}
size_t tv_plane_bytes(int B, int H, int W) { return emd::round256((size_t)B * H * W * sizeof(float)); }

template <int MODE>
void launch_wiener(int ksize, dim3 grid, hipStream_t st, const float* x, float* out, int H, int W, int tiles_x, float noise,
                   double* part, float* noise_out) {
#define EMD_WIENER_CASE(SZ) \
    case SZ:                \
        hipLaunchKernelGGL((filter_wiener_kernel<SZ, MODE>), grid, dim3(256), 0, st, x, out, H, W, tiles_x, noise, part, noise_out); \
        break;
    switch (ksize) {
        EMD_WIENER_CASE(3)
        EMD_WIENER_CASE(5)
        EMD_WIENER_CASE(7)
        EMD_WIENER_CASE(9)
    }
#undef EMD_WIENER_CASE
}

}  // namespace

extern "C" int emd_filter_gaussian_f32(const float* x, float* out, int B, int H, int W, const float* taps_host, int ksize,
                                       emd_stream_t stream) {
    int rc = check_images("emd_filter_gaussian_f32", x, out, B, H, W, kGaussTH);
    if (rc != EMD_OK) return rc;
    EMD_REQUIRE(taps_host, EMD_E_INVALID, "emd_filter_gaussian_f32: null pointer (taps_host)");
    EMD_REQUIRE(ksize >= 3 && ksize <= kMaxSize && ksize % 2 == 1, EMD_E_INVALID, "emd_filter_gaussian_f32: ksize must be odd, 3..15");
    rc = check_mirror("emd_filter_gaussian_f32", ksize / 2, H, W);
    if (rc != EMD_OK || B == 0) return rc;
    Taps t;
    for (int k = 0; k < kMaxSize; ++k) t.g[k] = k < ksize ? taps_host[k] : 0.f;
    int tiles_x;
    const dim3 grid = grid_of(B, H, W, kGaussTH, &tiles_x);
    hipStream_t st = static_cast<hipStream_t>(stream);
#define EMD_GAUSS_CASE(SZ) \
    case SZ:               \
        hipLaunchKernelGGL((filter_gaussian_kernel<SZ>), grid, dim3(256), 0, st, x, out, H, W, tiles_x, t); \
        break;
    switch (ksize) {
        EMD_GAUSS_CASE(3)
        EMD_GAUSS_CASE(5)
        EMD_GAUSS_CASE(7)
        EMD_GAUSS_CASE(9)
        EMD_GAUSS_CASE(11)
        EMD_GAUSS_CASE(13)
        EMD_GAUSS_CASE(15)
    }
#undef EMD_GAUSS_CASE
    return emd::check_launch("filter_gaussian_kernel");
}

extern "C" int emd_filter_median_f32(const float* x, float* out, int B, int H, int W, int ksize, emd_stream_t stream) {
    int rc = check_images("emd_filter_median_f32", x, out, B, H, W, kSmallTH);
    if (rc != EMD_OK) return rc;
    EMD_REQUIRE(ksize == 3 || ksize == 5, EMD_E_INVALID, "emd_filter_median_f32: ksize must be 3 or 5");
    rc = check_mirror("emd_filter_median_f32", ksize / 2, H, W);
    if (rc != EMD_OK || B == 0) return rc;
    int tiles_x;
    const dim3 grid = grid_of(B, H, W, kSmallTH, &tiles_x);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (ksize == 3)
        hipLaunchKernelGGL(filter_median_kernel<3>, grid, dim3(256), 0, st, x, out, H, W, tiles_x);
    else
        hipLaunchKernelGGL(filter_median_kernel<5>, grid, dim3(256), 0, st, x, out, H, W, tiles_x);
    return emd::check_launch("filter_median_kernel");
}

extern "C" int emd_filter_bilateral_f32(const float* x, float* out, int B, int H, int W, int d, float sigma_color, float sigma_space,
                                        emd_stream_t stream) {
    int rc = check_images("emd_filter_bilateral_f32", x, out, B, H, W, kSmallTH);
    if (rc != EMD_OK) return rc;
    EMD_REQUIRE(d >= 3 && d <= kMaxD && d % 2 == 1, EMD_E_INVALID, "emd_filter_bilateral_f32: d must be odd, 3..9");
    EMD_REQUIRE(sigma_color > 0.f && sigma_space > 0.f, EMD_E_INVALID, "emd_filter_bilateral_f32: the sigmas must be positive");
    const int r = d / 2;
    rc = check_mirror("emd_filter_bilateral_f32", r, H, W);
    if (rc != EMD_OK || B == 0) return rc;
    SpaceWeights sw{};   // once per launch, in double, rounded once
    for (int i = 0; i < d; ++i)
        for (int j = 0; j < d; ++j) {
            const int d2 = (i - r) * (i - r) + (j - r) * (j - r);
            if (d2 <= r * r) sw.w[i * d + j] = (float)std::exp(-(double)d2 / (2.0 * (double)sigma_space * (double)sigma_space));
        }
    const float neg_c = (float)(-(double)kLog2e / (2.0 * (double)sigma_color * (double)sigma_color));
    int tiles_x;
    const dim3 grid = grid_of(B, H, W, kSmallTH, &tiles_x);
    hipStream_t st = static_cast<hipStream_t>(stream);
#define EMD_BIL_CASE(RR) \
    case RR:             \
        hipLaunchKernelGGL((filter_bilateral_kernel<RR>), grid, dim3(256), 0, st, x, out, H, W, tiles_x, sw, neg_c); \
        break;
    switch (r) {
        EMD_BIL_CASE(1)
        EMD_BIL_CASE(2)
        EMD_BIL_CASE(3)
        EMD_BIL_CASE(4)
    }
#undef EMD_BIL_CASE
    return emd::check_launch("filter_bilateral_kernel");
}

extern "C" size_t emd_filter_wiener_workspace_bytes(int B, int H, int W) {
    if (B < 1 || B > 65535 || H < 1 || W < 1 || (long)emd::tiles_of(H, kWienerTH) * emd::tiles_of(W, kTW) > INT_MAX) return 0;
    return wiener_ws_bytes(B, H, W);
}

extern "C" int emd_filter_wiener_f32(const float* x, float* out, int B, int H, int W, int ksize, float noise, float* noise_out,
                                     void* workspace, size_t workspace_bytes, emd_stream_t stream) {
    int rc = check_images("emd_filter_wiener_f32", x, out, B, H, W, kWienerTH);
    if (rc != EMD_OK) return rc;
    EMD_REQUIRE(wiener_size_ok(ksize), EMD_E_INVALID, "emd_filter_wiener_f32: ksize must be odd, 3..9");
    EMD_REQUIRE(noise == noise, EMD_E_INVALID, "emd_filter_wiener_f32: noise is NaN");
    const bool estimate = noise < 0.f;
    if (estimate) {
        EMD_REQUIRE(workspace, EMD_E_INVALID, "emd_filter_wiener_f32: null pointer (the noise estimate needs the workspace)");
        EMD_REQUIRE(B == 0 || workspace_bytes >= wiener_ws_bytes(B, H, W), EMD_E_INVALID, "emd_filter_wiener_f32: workspace too small");
        EMD_REQUIRE(emd::aligned16(workspace), EMD_E_ALIGN, "emd_filter_wiener_f32: workspace must be 16-byte aligned");
    }
    if (B == 0) return EMD_OK;
    int tiles_x;
    const dim3 grid = grid_of(B, H, W, kWienerTH, &tiles_x);
    hipStream_t st = static_cast<hipStream_t>(stream);
    double* part = static_cast<double*>(workspace);
    if (!estimate) {
        launch_wiener<0>(ksize, grid, st, x, out, H, W, tiles_x, noise, nullptr, noise_out);
    } else {
        launch_wiener<1>(ksize, grid, st, x, out, H, W, tiles_x, 0.f, part, nullptr);
        rc = emd::check_launch("filter_wiener_kernel (moments)");
        if (rc != EMD_OK) return rc;
        launch_wiener<2>(ksize, grid, st, x, out, H, W, tiles_x, 0.f, part, noise_out);
    }
    return emd::check_launch("filter_wiener_kernel");
}

extern "C" size_t emd_filter_tv_workspace_bytes(int B, int H, int W) {
    if (B < 1 || B > 65535 || H < 1 || W < 1 || (long)emd::tiles_of(H, kSmallTH) * emd::tiles_of(W, kTW) > INT_MAX) return 0;
    return 4 * tv_plane_bytes(B, H, W);
}

extern "C" int emd_filter_tv_f32(const float* x, float* out, int B, int H, int W, float weight, int n_iter, void* workspace,
                                 size_t workspace_bytes, emd_stream_t stream) {
    int rc = check_images("emd_filter_tv_f32", x, out, B, H, W, kSmallTH);
    if (rc != EMD_OK) return rc;
    EMD_REQUIRE(weight > 0.f, EMD_E_INVALID, "emd_filter_tv_f32: weight must be positive");
    EMD_REQUIRE(n_iter >= 1, EMD_E_INVALID, "emd_filter_tv_f32: n_iter must be >= 1");
    EMD_REQUIRE(workspace, EMD_E_INVALID, "emd_filter_tv_f32: null pointer (workspace)");
    EMD_REQUIRE(B == 0 || workspace_bytes >= 4 * tv_plane_bytes(B, H, W), EMD_E_INVALID, "emd_filter_tv_f32: workspace too small");
    EMD_REQUIRE(emd::aligned16(workspace), EMD_E_ALIGN, "emd_filter_tv_f32: workspace must be 16-byte aligned");
    if (B == 0) return EMD_OK;
    const size_t n = (size_t)B * H * W * sizeof(float);
    EMD_REQUIRE(!emd::overlap(workspace, 4 * tv_plane_bytes(B, H, W), x, n) && !emd::overlap(workspace, 4 * tv_plane_bytes(B, H, W), out, n), EMD_E_INVALID, "emd_filter_tv_f32: the workspace may not overlap x or out");
    int tiles_x;
    const dim3 grid = grid_of(B, H, W, kSmallTH, &tiles_x);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t plane = tv_plane_bytes(B, H, W);
    char* ws = static_cast<char*>(workspace);
    const float tau = 0.25f;
    for (int k = 0; k < n_iter; ++k) {
        // iteration k reads the pair of planes iteration k - 1 wrote
        float* w1 = reinterpret_cast<float*>(ws + (size_t)(k & 1) * 2 * plane);
        const float* r1 = reinterpret_cast<const float*>(ws + (size_t)((k + 1) & 1) * 2 * plane);
        hipLaunchKernelGGL(filter_tv_kernel, grid, dim3(256), 0, st, x, r1, r1 + plane / sizeof(float), w1, w1 + plane / sizeof(float), out, H,
                           W, tiles_x, tau, tau / weight, k == 0 ? 1 : 0, k == n_iter - 1 ? 1 : 0);
        rc = emd::check_launch("filter_tv_kernel");
        if (rc != EMD_OK) return rc;
    }
    return EMD_OK;
}

extern "C" int emd_filter_clip01_f32(const float* x, float* out, long n, emd_stream_t stream) {
    EMD_REQUIRE(x && out, EMD_E_INVALID, "emd_filter_clip01_f32: null pointer");
    EMD_REQUIRE(n >= 0, EMD_E_INVALID, "emd_filter_clip01_f32: n must be >= 0");
    EMD_REQUIRE(out == x || !emd::overlap(x, (size_t)n * sizeof(float), out, (size_t)n * sizeof(float)), EMD_E_INVALID,
                "emd_filter_clip01_f32: out is x itself or does not overlap it");
    if (n == 0) return EMD_OK;
    const long nb = (n + 255) / 256;
    hipLaunchKernelGGL(filter_clip01_kernel, dim3((unsigned)(nb < 2048 ? nb : 2048)), dim3(256), 0, static_cast<hipStream_t>(stream), x, out, n);
    return emd::check_launch("filter_clip01_kernel");
}
