// Whole-micrograph tiling on the device: the host-side numpy around the three apply classes' denoise()
//   autoencoder.Micrograph_Autoencoder.preprocess     NaN/Inf -> 0, scale0to1, / mean          -> emd_tile_prep_f32(EMD_TILE_PREP_S)
//   kernel_denoiser.Micrograph_Autoencoder.denoise    NaN/Inf -> 0, statistics of the reflect-
//                                                     padded image, (x - off) / scale          -> emd_tile_prep_f32(EMD_TILE_PREP_K)
//   denoiser.Denoiser.preprocess                      cv2 resize, scale0to1, NaN/Inf -> 0.5,
//                                                     scale0to1 (numpy NaN semantics)          -> emd_tile_prep_f32(EMD_TILE_PREP_D)
//   the crop stacks of Denoiser.denoise / Micrograph_Autoencoder.denoise (+ the per-crop rescale) -> emd_tile_gather_f32
//   their overlap-add / count division                                                         -> emd_tile_blend_f32
//   K's inverse rescale                                                                        -> emd_tile_affine_f32
// Bandwidth-bound kernels with plain loads and stores; no atomics.  Per-image reductions are partials plus a second launch that
// sums them in a fixed order, so every result is deterministic.  The tile plan is the caller's (tiling.py): kernels read it,
// never recompute it, and index with REFLECT folding so that any plan content stays inside the image.
#include "emd_common.hpp"
#include "wave_reduce.hpp"

#include <cmath>

#pragma clang fp contract(off)  // every float operation rounds where numpy's does (no fused multiply-adds)

namespace {

using namespace emd;

constexpr int kThreads = 256;

struct Part {  // one slab's partial statistics of one image
    double sum;
    float mn, mx;
    int nan, pad_;
};
struct ImgStat {  // per image, between the launches of one emd_tile_prep_f32 call
    float lo, hi, mean;
    int flag;
};

// numpy's mode="reflect" (no edge repeat) for any offset: the periodic mirror of period 2(n-1)
__device__ inline int reflect_idx_periodic(int i, int n) {
    if (n == 1) return 0;
    const int p = 2 * (n - 1);
    i %= p;
    if (i < 0) i += p;
    return i < n ? i : p - i;
}

// how many times pixel r of n appears in the reflect-padded axis of pad p (p < n): 1 + mirrored into each pad
__device__ inline int pad_weight(int r, int n, int p) {
    return 1 + (r >= 1 && r <= p) + (r >= n - 1 - p && r <= n - 2);
}

__device__ inline float fix0(float v) { return isfinite(v) ? v : 0.f; }
// scale0to1 of one pixel with numpy's rounding: (x - lo) / (hi - lo); lo == hi -> 0.5; NaN lo / hi -> NaN
__device__ inline float s01(float v, float lo, float hi) { return lo == hi ? 0.5f : (v - lo) / (hi - lo); }

// (sum, min, max, nan) of a block of NW waves, in a fixed order; the result is valid in thread 0
template <int NW>
__device__ inline Part block_reduce(double sum, float mn, float mx, int nan) {
    __shared__ double ssum[NW];
    __shared__ float smn[NW], smx[NW];
    __shared__ int snan[NW];
    sum = wave_sum(sum);
    mn = wave_min(mn);
    mx = wave_max(mx);
    nan = wave_or(nan);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) ssum[w] = sum, smn[w] = mn, smx[w] = mx, snan[w] = nan;
    __syncthreads();
    Part p{};
    if (threadIdx.x == 0) {
        p.sum = ssum[0], p.mn = smn[0], p.mx = smx[0], p.nan = snan[0];
        for (int i = 1; i < NW; ++i) p.sum += ssum[i], p.mn = fminf(p.mn, smn[i]), p.mx = fmaxf(p.mx, smx[i]), p.nan |= snan[i];
    }
    return p;
}

// ---- image preparation: partial statistics per slab, one final launch per image, one elementwise write
enum Stage { ST_MINMAX_FIX0 = 0, ST_SUM_S01 = 1, ST_K = 2, ST_MINMAX_NAN = 3 };

// grid (slabs, N): slab s takes rows s, s + slabs, ... of image n, its threads stride the columns.  ST_MINMAX_FIX0 min/max of
// fix0(x); ST_SUM_S01 sum of scale0to1(fix0(x)); ST_K min/max of fix0(x) and its sum weighted by the reflect-pad multiplicities
// (pad kpad: a row weight per row, a column weight per pixel); ST_MINMAX_NAN min/max and whether any pixel is NaN
template <int ST>
__global__ void __launch_bounds__(kThreads) prep_partial_kernel(const float* __restrict__ x, int H, int W, int kpad,
                                                                const ImgStat* __restrict__ st, Part* __restrict__ part) {
    const int n = blockIdx.y, nslab = gridDim.x;
    const float* xi = x + (long)n * H * W;
    float lo = 0.f, hi = 0.f;
    if (ST == ST_SUM_S01) lo = st[n].lo, hi = st[n].hi;
    double sum = 0.0;
    float mn = INFINITY, mx = -INFINITY;
    int nan = 0;
    for (int r = blockIdx.x; r < H; r += nslab) {
        const float* row = xi + (long)r * W;
        double rsum = 0.0;
#pragma unroll 4
        for (int c = threadIdx.x; c < W; c += kThreads) {
            float v = row[c];
            if (ST == ST_MINMAX_NAN) {
                nan |= (v != v);
            } else {
                v = fix0(v);
            }
            if (ST == ST_SUM_S01) {
                rsum += (double)s01(v, lo, hi);
            } else {
                mn = fminf(mn, v);
                mx = fmaxf(mx, v);
            }
            if (ST == ST_K) rsum += (double)pad_weight(c, W, kpad) * (double)v;
        }
        sum += ST == ST_K ? (double)pad_weight(r, H, kpad) * rsum : rsum;
    }
    const Part p = block_reduce<kThreads / 64>(sum, mn, mx, nan);
    if (threadIdx.x == 0) part[(long)n * nslab + blockIdx.x] = p;
}

// one 64-thread block per image: the slabs in a fixed order -> ImgStat (and, for K, the (off, scale, flat) the inverse needs).
// count: the pixels the mean divides by (the padded image's for K).
template <int ST>
__global__ void prep_final_kernel(const Part* __restrict__ part, int nslab, double count, ImgStat* __restrict__ st,
                                  double* __restrict__ kstats) {
    const int n = blockIdx.x;
    double sum = 0.0;
    float mn = INFINITY, mx = -INFINITY;
    int nan = 0;
    for (int s = threadIdx.x; s < nslab; s += 64) {
        const Part p = part[(long)n * nslab + s];
        sum += p.sum;
        mn = fminf(mn, p.mn);
        mx = fmaxf(mx, p.mx);
        nan |= p.nan;
    }
    sum = wave_sum(sum);
    mn = wave_min(mn);
    mx = wave_max(mx);
    nan = wave_or(nan);
    if (threadIdx.x != 0) return;
    ImgStat r = st[n];
    if (ST == ST_MINMAX_FIX0) {
        r.lo = mn, r.hi = mx;
    } else if (ST == ST_SUM_S01) {
        r.mean = (float)(sum / count);  // np.mean of the float32 image, accumulated in double, rounded once
    } else if (ST == ST_MINMAX_NAN) {
        r.lo = nan ? NAN : mn, r.hi = nan ? NAN : mx;  // np.min / np.max are NaN when any pixel is
    } else {
        // kernel_denoiser.denoise: offset = float(min); flat if max == offset; scale = float(mean32) - offset (a double)
        const float mean32 = (float)(sum / count);
        const double scale = (double)mean32 - (double)mn;
        r.lo = mn, r.hi = mx, r.flag = (mx == mn);
        r.mean = (float)scale;  // (padded - offset) / scale runs in float32
        kstats[3 * n + 0] = (double)mn;
        kstats[3 * n + 1] = r.flag ? 0.0 : scale;
        kstats[3 * n + 2] = r.flag ? 1.0 : 0.0;
    }
    st[n] = r;
}

enum WriteMode { WR_S = 0, WR_K = 1, WR_D_FIRST = 2, WR_D_SECOND = 3 };

// grid (chunks, N); y may alias x
template <int WM>
__global__ void __launch_bounds__(kThreads) prep_write_kernel(const float* x, float* y, long npix, const ImgStat* __restrict__ st) {
    const int n = blockIdx.y;
    const ImgStat s = st[n];
    for (long k = (long)blockIdx.x * kThreads + threadIdx.x; k < npix; k += (long)gridDim.x * kThreads) {
        const long e = (long)n * npix + k;
        const float v = x[e];
        float o;
        if (WM == WR_S) {
            o = s01(fix0(v), s.lo, s.hi) / s.mean;
        } else if (WM == WR_K) {
            o = s.flag ? 1.f : (fix0(v) - s.lo) / s.mean;
        } else if (WM == WR_D_FIRST) {
            const float t = s01(v, s.lo, s.hi);
            o = isfinite(t) ? t : 0.5f;
        } else {
            o = s01(v, s.lo, s.hi);
        }
        y[e] = o;
    }
}

// cv2.resize INTER_LINEAR (half-pixel centres, edge clamp) in double, rounded to float32 once; [N,H,W] -> [N,S,S]
__global__ void __launch_bounds__(kThreads) resize_half_pixel_kernel(const float* __restrict__ x, float* __restrict__ y, int H, int W,
                                                                     int S) {
    const int n = blockIdx.y;
    const long npo = (long)S * S;
    const float* xi = x + (long)n * H * W;
    const double ry = (double)H / (double)S, rx = (double)W / (double)S;
    for (long k = (long)blockIdx.x * kThreads + threadIdx.x; k < npo; k += (long)gridDim.x * kThreads) {
        const int oy = (int)(k / S), ox = (int)(k - (long)oy * S);
        if (H == S && W == S) {  // the host path returns the image itself
            y[(long)n * npo + k] = xi[k];
            continue;
        }
        const double sy = ((double)oy + 0.5) * ry - 0.5, sx = ((double)ox + 0.5) * rx - 0.5;
        const double fy0 = floor(sy), fx0 = floor(sx);
        const double fy = sy - fy0, fx = sx - fx0;
        const int ly = (int)fy0, lx = (int)fx0;
        const int y0 = min(max(ly, 0), H - 1), y1 = min(max(ly + 1, 0), H - 1);
        const int x0 = min(max(lx, 0), W - 1), x1 = min(max(lx + 1, 0), W - 1);
        const double a = xi[(long)y0 * W + x0], b = xi[(long)y0 * W + x1];
        const double c = xi[(long)y1 * W + x0], d = xi[(long)y1 * W + x1];
        const double top = a * (1.0 - fx) + b * fx;
        const double bot = c * (1.0 - fx) + d * fx;
        y[(long)n * npo + k] = (float)(top * (1.0 - fy) + bot * fy);
    }
}

size_t part_bytes(int N, int nslab) { return ((size_t)N * (size_t)nslab * sizeof(Part) + 15) & ~(size_t)15; }

int slabs_of(int rows) { return rows < 1024 ? rows : 1024; }  // up to 1024 workgroups per image: 4 per CU for one 2048^2 image

unsigned chunks_of(long npix) {
    const long g = (npix + kThreads * 8 - 1) / (kThreads * 8);
    return (unsigned)(g < 1 ? 1 : (g > 1024 ? 1024 : g));
}

// ---- tile gather: crop t = (n, i, j) of the plan, rows/columns outside the image by REFLECT folding
__device__ inline void tile_of(int t, int ny, int nx, int& n, int& i, int& j) {
    const int tpi = ny * nx;
    n = t / tpi;
    const int r = t - n * tpi;
    i = r / nx;
    j = r - i * nx;
}

constexpr int kCopyRows = 4;

// grid (ceil(cs / kCopyRows), count): a verbatim copy (numpy slicing of the padded image)
__global__ void __launch_bounds__(kThreads) gather_copy_kernel(const float* __restrict__ src, int H, int W, int pad, int cs,
                                                               const int* __restrict__ ys, int ny, const int* __restrict__ xs, int nx,
                                                               int t0, float* __restrict__ out) {
    int n, i, j;
    tile_of(t0 + (int)blockIdx.y, ny, nx, n, i, j);
    const int y0 = ys[i] - pad, x0 = xs[j] - pad;
    const float* s = src + (long)n * H * W;
    float* o = out + (long)blockIdx.y * cs * cs;
    const int a0 = blockIdx.x * kCopyRows;
    const int rows = min(kCopyRows, cs - a0);
    for (int e = threadIdx.x; e < rows * cs; e += kThreads) {
        const int a = a0 + e / cs, b = e % cs;
        o[(long)a * cs + b] = s[(long)reflect_idx_periodic(y0 + a, H) * W + reflect_idx_periodic(x0 + b, W)];
    }
}

constexpr int kRescaleThreads = 1024;  // 16 waves per crop: the loads of one crop in flight together

// one workgroup per crop: (off, scale) = (min, mean - min) of the crop, then (x - off) / scale, or 1.0 for a flat crop
// (autoencoder.Micrograph_Autoencoder.denoise).  The second pass re-reads the crop, from cache.
__global__ void __launch_bounds__(kRescaleThreads) gather_rescale_kernel(const float* __restrict__ src, int H, int W, int pad, int cs,
                                                                  const int* __restrict__ ys, int ny, const int* __restrict__ xs, int nx,
                                                                  int t0, float* __restrict__ out, float* __restrict__ cstats) {
    __shared__ float s_off, s_scale;
    int n, i, j;
    tile_of(t0 + (int)blockIdx.x, ny, nx, n, i, j);
    const int y0 = ys[i] - pad, x0 = xs[j] - pad;
    const float* s = src + (long)n * H * W;
    float* o = out + (long)blockIdx.x * cs * cs;
    const int npc = cs * cs;
    double sum = 0.0;
    float mn = INFINITY;
    int nan = 0;
#pragma unroll 4
    for (int e = threadIdx.x; e < npc; e += kRescaleThreads) {
        const int a = e / cs, b = e - a * cs;
        const float v = s[(long)reflect_idx_periodic(y0 + a, H) * W + reflect_idx_periodic(x0 + b, W)];
        sum += (double)v;
        mn = fminf(mn, v);
        nan |= (v != v);
    }
    const Part p = block_reduce<kRescaleThreads / 64>(sum, mn, -INFINITY, nan);
    if (threadIdx.x == 0) {
        const float off = p.nan ? NAN : p.mn;
        const float mean = (float)(p.sum / (double)npc);
        s_off = off;
        s_scale = mean - off;
        cstats[2 * (long)blockIdx.x + 0] = off;
        cstats[2 * (long)blockIdx.x + 1] = mean - off;
    }
    __syncthreads();
    const float off = s_off, scale = s_scale;
#pragma unroll 4
    for (int e = threadIdx.x; e < npc; e += kRescaleThreads) {
        const int a = e / cs, b = e - a * cs;
        const float v = s[(long)reflect_idx_periodic(y0 + a, H) * W + reflect_idx_periodic(x0 + b, W)];
        o[e] = scale == 0.f ? 1.f : (v - off) / scale;
    }
}

// ---- blend in gather form: one thread per output pixel sums, in ascending tile order, the predictions of the tiles whose kept
// window [start + m, start + cs - m) covers it, divides by their count in double and rounds once.  rr / cr narrow the search to
// the plan's covering range; the window test itself decides, so a wrong range can drop terms but never read outside the tiles.
__global__ void __launch_bounds__(kThreads) blend_kernel(const float* __restrict__ preds, const float* __restrict__ cstats, int H, int W,
                                                         int pad, int cs, int m, const int* __restrict__ ys, int ny,
                                                         const int* __restrict__ xs, int nx, const int* __restrict__ rr,
                                                         const int* __restrict__ cr, int clip, float* __restrict__ out) {
    const int n = blockIdx.y;
    const long npix = (long)H * W;
    for (long k = (long)blockIdx.x * kThreads + threadIdx.x; k < npix; k += (long)gridDim.x * kThreads) {
        const int y = (int)(k / W), x = (int)(k - (long)y * W);
        const int py = y + pad, px = x + pad;
        const int i0 = max(rr[2 * y], 0), i1 = min(rr[2 * y + 1], ny);
        const int j0 = max(cr[2 * x], 0), j1 = min(cr[2 * x + 1], nx);
        double acc = 0.0;
        int cnt = 0;
        for (int i = i0; i < i1; ++i) {
            const int a = py - ys[i];
            if (a < m || a >= cs - m) continue;
            for (int j = j0; j < j1; ++j) {
                const int b = px - xs[j];
                if (b < m || b >= cs - m) continue;
                const long t = ((long)n * ny + i) * nx + j;
                float p = preds[t * cs * cs + (long)a * cs + b];
                if (cstats) p = p * cstats[2 * t + 1] + cstats[2 * t];  // float32 multiply, then add (no FMA)
                acc += (double)p;
                ++cnt;
            }
        }
        double v = acc / (double)cnt;
        if (clip) v = v < 0.0 ? 0.0 : (v > 1.0 ? 1.0 : v);  // NaN stays NaN, as in np.clip
        out[(long)n * npix + k] = (float)v;
    }
}

// y = x * scale + off, or x * off where scale == 0 (a flat image), in double, rounded once
__global__ void __launch_bounds__(kThreads) affine_kernel(const float* __restrict__ x, float* __restrict__ y, long npix,
                                                          const double* __restrict__ st) {
    const int n = blockIdx.y;
    const double off = st[3 * n], scale = st[3 * n + 1];
    for (long k = (long)blockIdx.x * kThreads + threadIdx.x; k < npix; k += (long)gridDim.x * kThreads) {
        const long e = (long)n * npix + k;
        const double v = (double)x[e];
        y[e] = (float)(scale != 0.0 ? v * scale + off : v * off);
    }
}

}  // namespace

extern "C" size_t emd_tile_prep_workspace_bytes(int N, int H, int W, int mode, int param) {
    if (N <= 0 || H <= 0 || W <= 0) return 0;
    const int rows = mode == EMD_TILE_PREP_D && param > H ? param : H;
    return part_bytes(N, slabs_of(rows)) + (size_t)N * sizeof(ImgStat) + 64;
}

extern "C" int emd_tile_prep_f32(const float* x, float* y, int N, int H, int W, int mode, int param, double* stats, void* workspace,
                                 size_t workspace_bytes, emd_stream_t stream) {
    EMD_REQUIRE(N >= 1 && H >= 1 && W >= 1, EMD_E_INVALID, "emd_tile_prep_f32: N, H and W must be positive");
    EMD_REQUIRE(mode == EMD_TILE_PREP_S || mode == EMD_TILE_PREP_K || mode == EMD_TILE_PREP_D, EMD_E_INVALID,
                "emd_tile_prep_f32: bad mode");
    EMD_REQUIRE(x && y && workspace, EMD_E_INVALID, "emd_tile_prep_f32: null pointer");
    EMD_REQUIRE(mode != EMD_TILE_PREP_K || stats, EMD_E_INVALID, "emd_tile_prep_f32: K mode needs stats (null pointer)");
    EMD_REQUIRE(mode != EMD_TILE_PREP_K || (param >= 0 && param < H && param < W), EMD_E_INVALID,
                "emd_tile_prep_f32: K mode needs 0 <= pad < min(H, W)");
    EMD_REQUIRE(mode != EMD_TILE_PREP_D || param >= 1, EMD_E_INVALID, "emd_tile_prep_f32: D mode needs an output size >= 1");
    EMD_REQUIRE(mode != EMD_TILE_PREP_D || x != y, EMD_E_INVALID, "emd_tile_prep_f32: D mode: y may not alias x");
    EMD_REQUIRE(workspace_bytes >= emd_tile_prep_workspace_bytes(N, H, W, mode, param), EMD_E_INVALID,
                "emd_tile_prep_f32: workspace too small");
    EMD_REQUIRE(N <= 65535, EMD_E_UNSUPPORTED, "emd_tile_prep_f32: more than 65535 images");
    EMD_REQUIRE((long)H * W < (1L << 31) && (mode != EMD_TILE_PREP_D || (long)param * param < (1L << 31)), EMD_E_UNSUPPORTED,
                "emd_tile_prep_f32: image of 2^31 pixels or more");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const long npix = (long)H * W;
    Part* part = static_cast<Part*>(workspace);
    const size_t pb = part_bytes(N, slabs_of(mode == EMD_TILE_PREP_D && param > H ? param : H));
    ImgStat* ist = reinterpret_cast<ImgStat*>(static_cast<char*>(workspace) + pb);
    const int ns = slabs_of(H);
    if (mode == EMD_TILE_PREP_S) {
        hipLaunchKernelGGL(prep_partial_kernel<ST_MINMAX_FIX0>, dim3(ns, N), dim3(kThreads), 0, st, x, H, W, 0, ist, part);
        hipLaunchKernelGGL(prep_final_kernel<ST_MINMAX_FIX0>, dim3(N), dim3(64), 0, st, part, ns, (double)npix, ist, nullptr);
        hipLaunchKernelGGL(prep_partial_kernel<ST_SUM_S01>, dim3(ns, N), dim3(kThreads), 0, st, x, H, W, 0, ist, part);
        hipLaunchKernelGGL(prep_final_kernel<ST_SUM_S01>, dim3(N), dim3(64), 0, st, part, ns, (double)npix, ist, nullptr);
        hipLaunchKernelGGL(prep_write_kernel<WR_S>, dim3(chunks_of(npix), N), dim3(kThreads), 0, st, x, y, npix, ist);
        return emd::check_launch("tile_prep S");
    }
    if (mode == EMD_TILE_PREP_K) {
        const double count = (double)(H + 2 * param) * (double)(W + 2 * param);
        hipLaunchKernelGGL(prep_partial_kernel<ST_K>, dim3(ns, N), dim3(kThreads), 0, st, x, H, W, param, ist, part);
        hipLaunchKernelGGL(prep_final_kernel<ST_K>, dim3(N), dim3(64), 0, st, part, ns, count, ist, stats);
        hipLaunchKernelGGL(prep_write_kernel<WR_K>, dim3(chunks_of(npix), N), dim3(kThreads), 0, st, x, y, npix, ist);
        return emd::check_launch("tile_prep K");
    }
    const int S = param;
    const long npo = (long)S * S;
    const int no = slabs_of(S);
    hipLaunchKernelGGL(resize_half_pixel_kernel, dim3(chunks_of(npo), N), dim3(kThreads), 0, st, x, y, H, W, S);
    hipLaunchKernelGGL(prep_partial_kernel<ST_MINMAX_NAN>, dim3(no, N), dim3(kThreads), 0, st, y, S, S, 0, ist, part);
    hipLaunchKernelGGL(prep_final_kernel<ST_MINMAX_NAN>, dim3(N), dim3(64), 0, st, part, no, (double)npo, ist, nullptr);
    hipLaunchKernelGGL(prep_write_kernel<WR_D_FIRST>, dim3(chunks_of(npo), N), dim3(kThreads), 0, st, y, y, npo, ist);
    hipLaunchKernelGGL(prep_partial_kernel<ST_MINMAX_NAN>, dim3(no, N), dim3(kThreads), 0, st, y, S, S, 0, ist, part);
    hipLaunchKernelGGL(prep_final_kernel<ST_MINMAX_NAN>, dim3(N), dim3(64), 0, st, part, no, (double)npo, ist, nullptr);
    hipLaunchKernelGGL(prep_write_kernel<WR_D_SECOND>, dim3(chunks_of(npo), N), dim3(kThreads), 0, st, y, y, npo, ist);
    return emd::check_launch("tile_prep D");
}

extern "C" int emd_tile_gather_f32(const float* src, int N, int H, int W, int pad, int cs, const int* ys, int ny, const int* xs, int nx,
                                   int t0, int count, float* out, float* crop_stats, emd_stream_t stream) {
    EMD_REQUIRE(N >= 1 && H >= 1 && W >= 1 && cs >= 1 && ny >= 1 && nx >= 1 && count >= 1 && pad >= 0 && t0 >= 0, EMD_E_INVALID,
                "emd_tile_gather_f32: sizes must be positive (pad, t0 non-negative)");
    EMD_REQUIRE(src && ys && xs && out, EMD_E_INVALID, "emd_tile_gather_f32: null pointer");
    EMD_REQUIRE(cs <= H + 2 * pad && cs <= W + 2 * pad, EMD_E_INVALID, "emd_tile_gather_f32: crop larger than the padded image");
    EMD_REQUIRE((long)t0 + count <= (long)N * ny * nx, EMD_E_INVALID, "emd_tile_gather_f32: tiles past the end of the plan");
    EMD_REQUIRE((long)N * ny * nx < (1L << 31) && (long)H * W < (1L << 31) && (long)cs * cs < (1L << 31), EMD_E_UNSUPPORTED,
                "emd_tile_gather_f32: index range");
    EMD_REQUIRE(count <= 65535, EMD_E_UNSUPPORTED, "emd_tile_gather_f32: more than 65535 tiles in one call");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (crop_stats) {
        hipLaunchKernelGGL(gather_rescale_kernel, dim3(count), dim3(kRescaleThreads), 0, st, src, H, W, pad, cs, ys, ny, xs, nx, t0, out,
                           crop_stats);
        return emd::check_launch("gather_rescale_kernel");
    }
    hipLaunchKernelGGL(gather_copy_kernel, dim3((cs + kCopyRows - 1) / kCopyRows, count), dim3(kThreads), 0, st, src, H, W, pad, cs, ys, ny,
                       xs, nx, t0, out);
    return emd::check_launch("gather_copy_kernel");
}

extern "C" int emd_tile_blend_f32(const float* preds, const float* crop_stats, int N, int H, int W, int pad, int cs, int m, const int* ys,
                                  int ny, const int* xs, int nx, const int* row_range, const int* col_range, int clip, float* out,
                                  emd_stream_t stream) {
    EMD_REQUIRE(N >= 1 && H >= 1 && W >= 1 && cs >= 1 && ny >= 1 && nx >= 1 && pad >= 0, EMD_E_INVALID,
                "emd_tile_blend_f32: sizes must be positive (pad non-negative)");
    EMD_REQUIRE(preds && ys && xs && row_range && col_range && out, EMD_E_INVALID, "emd_tile_blend_f32: null pointer");
    EMD_REQUIRE(cs <= H + 2 * pad && cs <= W + 2 * pad, EMD_E_INVALID, "emd_tile_blend_f32: crop larger than the padded image");
    EMD_REQUIRE(m >= 0 && 2 * m < cs, EMD_E_INVALID, "emd_tile_blend_f32: margin m must satisfy 0 <= m < cs/2");
    EMD_REQUIRE(clip == 0 || clip == 1, EMD_E_INVALID, "emd_tile_blend_f32: clip must be 0 or 1");
    EMD_REQUIRE(N <= 65535, EMD_E_UNSUPPORTED, "emd_tile_blend_f32: more than 65535 images");
    EMD_REQUIRE((long)H * W < (1L << 31), EMD_E_UNSUPPORTED, "emd_tile_blend_f32: image of 2^31 pixels or more");
    const long npix = (long)H * W;
    hipLaunchKernelGGL(blend_kernel, dim3(chunks_of(npix), N), dim3(kThreads), 0, static_cast<hipStream_t>(stream), preds, crop_stats, H, W,
                       pad, cs, m, ys, ny, xs, nx, row_range, col_range, clip, out);
    return emd::check_launch("blend_kernel");
}

extern "C" int emd_tile_affine_f32(const float* x, float* y, int N, long npix, const double* stats, emd_stream_t stream) {
    EMD_REQUIRE(N >= 1 && npix >= 1, EMD_E_INVALID, "emd_tile_affine_f32: N and npix must be positive");
    EMD_REQUIRE(x && y && stats, EMD_E_INVALID, "emd_tile_affine_f32: null pointer");
    EMD_REQUIRE(N <= 65535, EMD_E_UNSUPPORTED, "emd_tile_affine_f32: more than 65535 images");
    hipLaunchKernelGGL(affine_kernel, dim3(chunks_of(npix), N), dim3(kThreads), 0, static_cast<hipStream_t>(stream), x, y, npix, stats);
    return emd::check_launch("affine_kernel");
}
