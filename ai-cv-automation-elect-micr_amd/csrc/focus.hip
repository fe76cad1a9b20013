// Autofocus on the device (the rules are in include/emdenoise.h): the arithmetic of the reference's
// em_env/fresnel_env.py:163-208 (fresnel_quantifier, get_optimal_z) and misc_py/entropy.py:36-53 (image_entropy).
//   laplacian_kernel       cv2.Laplacian(x, CV_32F, ksize 1 or 3), BORDER_REFLECT_101: a tile with a halo of 1 in LDS, one launch
//   lap_pass_kernel        the same tile, the Laplacian kept in registers: pass 0 its sum, pass 1 the count and the sum of the values
//                          >= mean, pass 2 the set's centred 2nd and 4th power sums; two sums per tile, each a pair hi + lo of doubles
//   moments_stage_kernel   the tiles' partials -> the mean, the set's mean, the six outputs (one workgroup per image, fixed order)
//   chunk_sum_kernel, norm_stage_kernel, hist01_kernel    the image's mean and population std (two-pass), then the histogram over
//                          [0, 1] with integer LDS atomics per workgroup and integer global adds
//   hist_entropy_kernel    -sum p log2 p of (counts + eps)
//   spline_argmin_kernel   the not-a-knot cubic through (z, scores), its values on numpy's linspace grid, the first smallest
// No floating-point atomics, fixed summation orders, launches (and one memset) only.
#include <cmath>

#include "stencil_rows.hpp"
#include "wave_reduce.hpp"

// Every operation below rounds on its own, as the header writes the formulas: the grid point (i * step) + z[0] has numpy's two
// roundings, a moment's term the restatement's bits, and the two-sums are exact.  The pragma is what guarantees it.  The __fadd_rn /
// __dmul_rn family does not: the toolchain's header defines them as the plain operators, compiled under the header's own contraction
// setting, so after inlining their products and sums ARE fused (seen in this file's assembly: (double)g * step + z0 became one
// v_fma_f64 and zbest missed numpy's bits by an ulp).  Plain operators under the pragma carry no contraction flag.
#pragma clang fp contract(off)

namespace {

constexpr int kMaxExtent = 32768;   // H, W
constexpr int kTW = 64;             // tile columns = lanes of a wave
constexpr int kTH = 32;             // tile rows (a wave: 8)
constexpr int kTR = kTH / 4;
constexpr int kLW = kTW + 2;        // the tile with its halo of 1
constexpr int kLH = kTH + 2;
constexpr int kChunk = 32768;       // pixels per workgroup of the 1-D passes
constexpr int kMaxBins = 4096;
constexpr int kMaxKnots = 256;      // N of the spline
constexpr int kMaxFactor = 4096;    // interp_factor

// BORDER_REFLECT_101 for a halo of 1 (n >= 2): -1 -> 1, n -> n - 2.  Positions further out belong to no output; they are clamped
// into the image so that the address is valid.
__device__ __forceinline__ int reflect101(int i, int n) {
    if (i < 0) i = -i;
    if (i >= n) i = 2 * n - 2 - i;
    return i < 0 ? 0 : i;
}

// xs[r][c] = pixel (reflect(r0 - 1 + r), reflect(c0 - 1 + c)) of the image at xb
__device__ __forceinline__ void load_tile(const float* __restrict__ xb, int H, int W, int r0, int c0, float* xs) {
    for (int i = threadIdx.x; i < kLH * kLW; i += 256) {
        const int r = i / kLW, c = i - r * kLW;
        const int pr = reflect101(r0 - 1 + r, H), pc = reflect101(c0 - 1 + c, W);
        xs[i] = xb[(long)pr * W + pc];
    }
}

// The float32 operation order of include/emdenoise.h, every operation rounding on its own.  p: the centre inside the LDS tile.
template <int KS>
__device__ __forceinline__ float laplacian_at(const float* p) {
    if (KS == 1)
        return ((p[-kLW] + p[kLW]) + (p[-1] + p[1])) - 4.f * p[0];
    return 2.f * ((p[-kLW - 1] + p[-kLW + 1]) + (p[kLW - 1] + p[kLW + 1])) - 8.f * p[0];
}

// grid (tiles, B)
template <int KS>
__global__ __launch_bounds__(256) void laplacian_kernel(const float* __restrict__ x, float* __restrict__ y, int H, int W, int tiles_x) {
    __shared__ float xs[kLH * kLW];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r0 = ((int)blockIdx.x / tiles_x) * kTH, c0 = ((int)blockIdx.x % tiles_x) * kTW;
    const long img = (long)blockIdx.y * H * W;
    load_tile(x + img, H, W, r0, c0, xs);
    __syncthreads();
    const int c = c0 + lane;
#pragma unroll
    for (int q = 0; q < kTR; ++q) {
        const int lr = wave * kTR + q, r = r0 + lr;
        if (r < H && c < W) y[img + (long)r * W + c] = laplacian_at<KS>(xs + (lr + 1) * kLW + lane + 1);
    }
}

// The moments' sums are carried as unevaluated pairs hi + lo of doubles (hi = the pair's value rounded to double), so that a sum of
// n terms is off by about n 2^-104 of the terms' magnitude before its one rounding: the device then gives the exactly rounded sum
// (math.fsum's) but for ties to within that, and the last column's cancellation (m4 / m2^2 against 3) amplifies nothing.  Costs a
// dozen double operations per pixel under a memory-bound pass.
struct DD {
    double hi, lo;
};
__device__ __forceinline__ DD dd_add(DD a, double b) {   // Knuth's two-sum, then the renormalisation
    const double s = a.hi + b, bb = s - a.hi;
    const double e = ((a.hi - (s - bb)) + (b - bb)) + a.lo;
    DD r;
    r.hi = s + e;
    r.lo = e - (r.hi - s);
    return r;
}
__device__ __forceinline__ DD dd_add(DD a, DD b) {
    const double s = a.hi + b.hi, bb = s - a.hi;
    const double e = ((a.hi - (s - bb)) + (b.hi - bb)) + (a.lo + b.lo);
    DD r;
    r.hi = s + e;
    r.lo = e - (r.hi - s);
    return r;
}

// Sum of one pair per thread over the 256 threads of a workgroup: lanes, then the four waves, in a fixed order.  Valid in thread 0.
// sh: 8 doubles, not otherwise in use between two calls' barriers.
__device__ __forceinline__ DD block_sum_dd_thread0(DD v, double* sh) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        DD o;
        o.hi = __shfl_down(v.hi, off, 64);
        o.lo = __shfl_down(v.lo, off, 64);
        v = dd_add(v, o);
    }
    __syncthreads();   // sh may still be read from the previous call
    if ((threadIdx.x & 63) == 0) {
        sh[2 * (threadIdx.x >> 6)] = v.hi;
        sh[2 * (threadIdx.x >> 6) + 1] = v.lo;
    }
    __syncthreads();
    DD r = {sh[0], sh[1]};
#pragma unroll
    for (int w = 1; w < 4; ++w) r = dd_add(r, DD{sh[2 * w], sh[2 * w + 1]});
    return r;
}

// Sum of the pairs (hi[i], lo[i]), i < n, by the 256 threads of a workgroup: a thread's i, i + 256, ... in ascending order, then a
// binary tree in LDS (every thread returns it).  shh, shl: 256 doubles each.
__device__ DD block_sum_dd_fixed(const double* __restrict__ hi, const double* __restrict__ lo, int n, double* shh, double* shl) {
    const int tid = threadIdx.x;
    DD s = {0.0, 0.0};
    for (int i = tid; i < n; i += 256) s = dd_add(s, DD{hi[i], lo[i]});
    __syncthreads();   // the arrays may still be read from the previous call
    shh[tid] = s.hi;
    shl[tid] = s.lo;
    __syncthreads();
    for (int off = 128; off >= 1; off >>= 1) {
        if (tid < off) {
            const DD r = dd_add(DD{shh[tid], shl[tid]}, DD{shh[tid + off], shl[tid + off]});
            shh[tid] = r.hi;
            shl[tid] = r.lo;
        }
        __syncthreads();
    }
    return DD{shh[0], shl[0]};
}

// Per image: acc[0] = mean_L, acc[1] = n, acc[2] = mean_S.
constexpr int kAcc = 4;
constexpr int kPart = 4;   // per tile: two sums as pairs (hi, lo, hi, lo)
struct MomentBuffers {
    double* part;   // [B][kPart][tiles]
    double* acc;    // [B][kAcc]
};

// grid (tiles, B).  PASS 0: sum L.  PASS 1: #{L >= mean_L} (an integer: exact) and their sum.  PASS 2 over the set (RECTIFY: the
// values >= mean_L; else all): sum (L - mean_S)^2 and sum (L - mean_S)^4.  Every term is rounded on its own, so a term has the bits
// the restatement gives it; a thread adds its 8 rows in ascending order, then block_sum_dd_thread0.
template <int KS, int PASS, bool RECTIFY>
__global__ __launch_bounds__(256) void lap_pass_kernel(const float* __restrict__ x, int H, int W, int tiles_x, MomentBuffers mb) {
    __shared__ float xs[kLH * kLW];
    __shared__ double sh[8];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int tile = blockIdx.x, tiles = gridDim.x;
    const int r0 = (tile / tiles_x) * kTH, c0 = (tile % tiles_x) * kTW;
    const long b = blockIdx.y;
    load_tile(x + b * (long)H * W, H, W, r0, c0, xs);
    double mean_l = 0.0, mean_s = 0.0;
    if (PASS >= 1) mean_l = mb.acc[b * kAcc];
    if (PASS == 2) mean_s = mb.acc[b * kAcc + 2];
    __syncthreads();
    DD s0 = {0.0, 0.0}, s1 = {0.0, 0.0};
    const int c = c0 + lane;
#pragma unroll
    for (int q = 0; q < kTR; ++q) {
        const int lr = wave * kTR + q, r = r0 + lr;
        if (r < H && c < W) {
            const double l = (double)laplacian_at<KS>(xs + (lr + 1) * kLW + lane + 1);
            if (PASS == 0) {
                s0 = dd_add(s0, l);
            } else if (PASS == 1) {
                if (l >= mean_l) {
                    s0.hi += 1.0;
                    s1 = dd_add(s1, l);
                }
            } else if (!RECTIFY || l >= mean_l) {
                const double d = l - mean_s, d2 = d * d;
                s0 = dd_add(s0, d2);
                s1 = dd_add(s1, d2 * d2);
            }
        }
    }
    double* out = mb.part + b * kPart * tiles + tile;
    DD v = block_sum_dd_thread0(s0, sh);
    if (threadIdx.x == 0) {
        out[0] = v.hi;
        out[tiles] = v.lo;
    }
    if (PASS >= 1) {
        v = block_sum_dd_thread0(s1, sh);
        if (threadIdx.x == 0) {
            out[2L * tiles] = v.hi;
            out[3L * tiles] = v.lo;
        }
    }
}

// grid (B).  stage 0: mean_L (and, without rectify, n = count and mean_S = mean_L); stage 1: n and mean_S; stage 2: the six outputs.
__global__ __launch_bounds__(256) void moments_stage_kernel(MomentBuffers mb, int tiles, double count, int stage, int rectify,
                                                            double* __restrict__ out) {
    __shared__ double shh[256], shl[256];
    const long b = blockIdx.x;
    const double* p = mb.part + b * kPart * tiles;
    const double v0 = block_sum_dd_fixed(p, p + tiles, tiles, shh, shl).hi;
    const double v1 = stage >= 1 ? block_sum_dd_fixed(p + 2L * tiles, p + 3L * tiles, tiles, shh, shl).hi : 0.0;
    if (threadIdx.x != 0) return;
    double* a = mb.acc + b * kAcc;
    if (stage == 0) {
        a[0] = v0 / count;
        if (!rectify) {
            a[1] = count;
            a[2] = a[0];
        }
    } else if (stage == 1) {
        a[1] = v0;
        a[2] = v1 / v0;
    } else {
        double* o = out + b * EMD_NFOCUS;
        const double n = a[1], m2 = v0 / n, m4 = v1 / n;
        o[0] = a[0];
        o[1] = n;
        o[2] = a[2];
        o[3] = m2;
        o[4] = m4;
        o[5] = m4 / (m2 * m2) - 3.0;
    }
}

// ---- histogram over [0, 1] ---------------------------------------------------------------------------------------------------------
struct NormBuffers {
    double* part;   // [B][chunks]
    double* acc;    // [B][2]: mean, population std
};

// grid (chunks, B).  PASS 0: sum x;  PASS 1: sum (x - mean)^2.
template <int PASS>
__global__ __launch_bounds__(256) void chunk_sum_kernel(const float* __restrict__ x, long n, NormBuffers nb) {
    __shared__ double sh[4];
    const long b = blockIdx.y;
    const double mean = PASS ? nb.acc[b * 2] : 0.0;
    const long begin = (long)blockIdx.x * kChunk, end = begin + kChunk < n ? begin + kChunk : n;
    const float* xb = x + b * n;
    double s = 0.0;
    for (long i = begin + threadIdx.x; i < end; i += 256) {
        const double v = (double)xb[i];
        if (PASS) {
            const double d = v - mean;
            s += d * d;
        } else {
            s += v;
        }
    }
    const double r = block_sum_thread0(s, sh);
    if (threadIdx.x == 0) nb.part[b * gridDim.x + blockIdx.x] = r;
}

// grid (B).  stage 0: the mean;  stage 1: the population standard deviation.
__global__ __launch_bounds__(256) void norm_stage_kernel(NormBuffers nb, int chunks, double count, int stage) {
    __shared__ double sh[256];
    const long b = blockIdx.x;
    const double v = block_sum_fixed(nb.part + b * chunks, chunks, 1, sh);
    if (threadIdx.x == 0) nb.acc[b * 2 + stage] = stage ? sqrt(v / count) : v / count;
}

// The bin of a value in [0, 1] (bins a power of two: the product is exact), -1 for everything else, NaN included.
template <typename T>
__device__ __forceinline__ int bin01(T t, int bins) {
    if (t >= (T)0 && t < (T)1) return (int)(t * (T)bins);
    return t == (T)1 ? bins - 1 : -1;
}

// grid (chunks, B): counts of this workgroup's pixels in LDS (integer atomics), then one integer add per non-empty bin.
template <bool NORM>
__global__ __launch_bounds__(256) void hist01_kernel(const float* __restrict__ x, long n, int bins, NormBuffers nb,
                                                     unsigned long long* __restrict__ counts) {
    __shared__ unsigned h[kMaxBins];
    const long b = blockIdx.y;
    for (int i = threadIdx.x; i < bins; i += 256) h[i] = 0;
    double mean = 0.0, sd = 1.0;
    if (NORM) {
        mean = nb.acc[b * 2];
        sd = nb.acc[b * 2 + 1];
    }
    __syncthreads();
    const long begin = (long)blockIdx.x * kChunk, end = begin + kChunk < n ? begin + kChunk : n;
    const float* xb = x + b * n;
    for (long i = begin + threadIdx.x; i < end; i += 256) {
        const float v = xb[i];
        int k;
        if (NORM)
            k = bin01<double>((0.15 * ((double)v - mean)) / sd + 0.5, bins);
        else
            k = bin01<float>(v, bins);
        if (k >= 0) atomicAdd(&h[k], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < bins; i += 256)
        if (h[i]) atomicAdd(&counts[b * bins + i], (unsigned long long)h[i]);
}

// grid (B): -sum p log p / log 2, p = (c + eps) / sum (c + eps), as scipy.stats.entropy(c + eps, base=2) forms it.
__global__ __launch_bounds__(256) void hist_entropy_kernel(const long long* __restrict__ counts, int bins, double eps,
                                                           double* __restrict__ out) {
    __shared__ double sh[256];
    const long long* c = counts + (long)blockIdx.x * bins;
    double s = 0.0;
    for (int i = threadIdx.x; i < bins; i += 256) s += (double)c[i] + eps;
    const double total = block_tree_sum(s, sh);
    double e = 0.0;
    for (int i = threadIdx.x; i < bins; i += 256) {
        const double p = ((double)c[i] + eps) / total;
        e += p > 0.0 ? -(p * log(p)) : (p == 0.0 ? 0.0 : -INFINITY);   // scipy.special.entr
    }
    e = block_tree_sum(e, sh);
    if (threadIdx.x == 0) out[blockIdx.x] = e / log(2.0);
}

// ---- the spline ----------------------------------------------------------------------------------------------------------------------
// grid (B).  Thread 0 solves for the second derivatives m (the natural tridiagonal rows 1 .. N - 2; the not-a-knot conditions
// eliminate m[0] and m[N - 1] from the first and the last of them), every thread evaluates its grid points i, i + 256, ..., and the
// first smallest value is found by a tree over (value, index) pairs.
__global__ __launch_bounds__(256) void spline_argmin_kernel(const double* __restrict__ z, const double* __restrict__ scores, int N, int G,
                                                            double* __restrict__ zbest, double* __restrict__ curve,
                                                            long long* __restrict__ index) {
    __shared__ double zs[kMaxKnots], ys[kMaxKnots], m[kMaxKnots], cp[kMaxKnots], dp[kMaxKnots];
    __shared__ double bv[256];
    __shared__ int bi[256];
    const int tid = threadIdx.x;
    const long b = blockIdx.x;
    for (int i = tid; i < N; i += 256) {
        zs[i] = z[i];
        ys[i] = scores[b * N + i];
    }
    __syncthreads();
    if (tid == 0) {
        // row i (1 <= i <= N - 2):  h[i-1] m[i-1] + 2 (h[i-1] + h[i]) m[i] + h[i] m[i+1] = 6 (d[i] - d[i-1]),  d[i] = (y[i+1] - y[i]) / h[i]
        // m[0] = (1 + h0 / h1) m[1] - (h0 / h1) m[2];   m[N-1] = (1 + hl / hk) m[N-2] - (hl / hk) m[N-3]   (hl = h[N-2], hk = h[N-3])
        const int last = N - 2;
        const double h0 = zs[1] - zs[0], h1 = zs[2] - zs[1], hl = zs[N - 1] - zs[N - 2], hk = zs[N - 2] - zs[N - 3];
        const double q0 = h0 / h1, ql = hl / hk;
        for (int i = 1; i <= last; ++i) {
            const double ha = zs[i] - zs[i - 1], hb = zs[i + 1] - zs[i];
            double lo = ha, di = 2.0 * (ha + hb), up = hb;
            const double rhs = 6.0 * ((ys[i + 1] - ys[i]) / hb - (ys[i] - ys[i - 1]) / ha);
            if (i == 1) {
                di += h0 * (1.0 + q0);
                up -= h0 * q0;
                lo = 0.0;
            }
            if (i == last) {
                di += hl * (1.0 + ql);
                lo -= hl * ql;
                up = 0.0;
            }
            // Thomas: forward sweep
            const double den = i == 1 ? di : di - lo * cp[i - 1];
            cp[i] = up / den;
            dp[i] = (i == 1 ? rhs : rhs - lo * dp[i - 1]) / den;
        }
        m[last] = dp[last];
        for (int i = last - 1; i >= 1; --i) m[i] = dp[i] - cp[i] * m[i + 1];
        m[0] = (1.0 + q0) * m[1] - q0 * m[2];
        m[N - 1] = (1.0 + ql) * m[N - 2] - ql * m[N - 3];
    }
    __syncthreads();
    const double z0 = zs[0], z1 = zs[N - 1];
    const double step = (z1 - z0) / (double)(G > 1 ? G - 1 : 1);
    double best = INFINITY;
    int besti = 0x7fffffff;
    for (int g = tid; g < G; g += 256) {
        const double xg = g == G - 1 && G > 1 ? z1 : (double)g * step + z0;   // numpy.linspace: two roundings
        int lo = 0, hi = N - 2;   // the interval: the last i <= N - 2 with z[i] <= xg
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (zs[mid] <= xg) lo = mid;
            else hi = mid - 1;
        }
        const double h = zs[lo + 1] - zs[lo], dx = xg - zs[lo];
        const double c1 = (ys[lo + 1] - ys[lo]) / h - h * (2.0 * m[lo] + m[lo + 1]) / 6.0;
        const double c3 = (m[lo + 1] - m[lo]) / (6.0 * h);
        const double v = ys[lo] + dx * (c1 + dx * (0.5 * m[lo] + dx * c3));
        if (curve) curve[b * G + g] = v;
        if (v < best) {   // ascending g: the first of equals stays
            best = v;
            besti = g;
        }
    }
    bv[tid] = best;
    bi[tid] = besti;
    __syncthreads();
    for (int off = 128; off >= 1; off >>= 1) {
        if (tid < off) {
            const double ov = bv[tid + off];
            const int oi = bi[tid + off];
            if (ov < bv[tid] || (ov == bv[tid] && oi < bi[tid])) {
                bv[tid] = ov;
                bi[tid] = oi;
            }
        }
        __syncthreads();
    }
    if (tid == 0) {
        const int g = bi[0] < G ? bi[0] : 0;   // no finite value anywhere: index 0
        zbest[b] = g == G - 1 && G > 1 ? z1 : (double)g * step + z0;
        if (index) index[b] = g;
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------
bool image_shape_ok(const char* who, int B, int H, int W) {
    if (B >= 0 && B <= 65535 && H >= 2 && W >= 2 && H <= kMaxExtent && W <= kMaxExtent) return true;
    emd::set_error("%s: bad shape (batch 0..65535, 2 <= H, W <= %d; got %d x %d x %d)", who, kMaxExtent, B, H, W);
    return false;
}

struct Tiling {
    int tiles_x, tiles;
};
Tiling tiling(int H, int W) {
    Tiling t;
    t.tiles_x = emd::tiles_of(W, kTW);
    t.tiles = t.tiles_x * emd::tiles_of(H, kTH);
    return t;
}

int chunks_of(int H, int W) { return (int)(((long)H * W + kChunk - 1) / kChunk); }

bool bins_ok(int bins) { return bins >= 2 && bins <= kMaxBins && !(bins & (bins - 1)); }

template <int KS>
void launch_moments(const float* x, int B, int H, int W, int rectify, MomentBuffers mb, double* out, hipStream_t st) {
    const Tiling t = tiling(H, W);
    const dim3 grid((unsigned)t.tiles, (unsigned)B), per_image((unsigned)B);
    const double count = (double)H * (double)W;
    hipLaunchKernelGGL((lap_pass_kernel<KS, 0, false>), grid, dim3(256), 0, st, x, H, W, t.tiles_x, mb);
    hipLaunchKernelGGL(moments_stage_kernel, per_image, dim3(256), 0, st, mb, t.tiles, count, 0, rectify, out);
    if (rectify) {
        hipLaunchKernelGGL((lap_pass_kernel<KS, 1, true>), grid, dim3(256), 0, st, x, H, W, t.tiles_x, mb);
        hipLaunchKernelGGL(moments_stage_kernel, per_image, dim3(256), 0, st, mb, t.tiles, count, 1, rectify, out);
        hipLaunchKernelGGL((lap_pass_kernel<KS, 2, true>), grid, dim3(256), 0, st, x, H, W, t.tiles_x, mb);
    } else {
        hipLaunchKernelGGL((lap_pass_kernel<KS, 2, false>), grid, dim3(256), 0, st, x, H, W, t.tiles_x, mb);
    }
    hipLaunchKernelGGL(moments_stage_kernel, per_image, dim3(256), 0, st, mb, t.tiles, count, 2, rectify, out);
}

}  // namespace

extern "C" int emd_laplacian_f32(const float* x, int B, int H, int W, int ksize, float* y, emd_stream_t stream) {
    if (!image_shape_ok("emd_laplacian_f32", B, H, W)) return EMD_E_INVALID;
    EMD_REQUIRE(ksize == 1 || ksize == 3, EMD_E_INVALID, "emd_laplacian_f32: ksize must be 1 or 3");
    if (B == 0) return EMD_OK;
    EMD_REQUIRE(x && y, EMD_E_INVALID, "emd_laplacian_f32: null pointer");
    const size_t nx = (size_t)B * H * W * sizeof(float);
    EMD_REQUIRE(!emd::overlap(x, nx, y, nx), EMD_E_INVALID, "emd_laplacian_f32: y may not overlap x");
    const Tiling t = tiling(H, W);
    const dim3 grid((unsigned)t.tiles, (unsigned)B);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (ksize == 1)
        hipLaunchKernelGGL(laplacian_kernel<1>, grid, dim3(256), 0, st, x, y, H, W, t.tiles_x);
    else
        hipLaunchKernelGGL(laplacian_kernel<3>, grid, dim3(256), 0, st, x, y, H, W, t.tiles_x);
    return emd::check_launch("laplacian_kernel");
}

extern "C" size_t emd_laplacian_moments_workspace_bytes(int B, int H, int W) {
    if (B < 1 || B > 65535 || H < 2 || W < 2 || H > kMaxExtent || W > kMaxExtent) return 0;
    return emd::round256((size_t)B * kPart * tiling(H, W).tiles * sizeof(double)) + emd::round256((size_t)B * kAcc * sizeof(double));
}

extern "C" int emd_laplacian_moments_f64(const float* x, int B, int H, int W, int ksize, int rectify, double* out, void* workspace,
                                         size_t workspace_bytes, emd_stream_t stream) {
    if (!image_shape_ok("emd_laplacian_moments_f64", B, H, W)) return EMD_E_INVALID;
    EMD_REQUIRE(ksize == 1 || ksize == 3, EMD_E_INVALID, "emd_laplacian_moments_f64: ksize must be 1 or 3");
    EMD_REQUIRE(rectify == 0 || rectify == 1, EMD_E_INVALID, "emd_laplacian_moments_f64: rectify must be 0 or 1");
    if (B == 0) return EMD_OK;
    const size_t need = emd_laplacian_moments_workspace_bytes(B, H, W);
    const emd::Range r[] = {{workspace, need, 16, false, false},
                            {x, (size_t)B * H * W * sizeof(float), 4, false, true},
                            {out, (size_t)B * EMD_NFOCUS * sizeof(double), 8, false, false}};
    const int rc = emd::check_ranges("emd_laplacian_moments_f64", r, 3,
                                     "the workspace must be 16-byte aligned, out 8-byte, x 4-byte", &workspace_bytes);
    if (rc != EMD_OK) return rc;
    MomentBuffers mb;
    mb.part = static_cast<double*>(workspace);
    mb.acc = reinterpret_cast<double*>(static_cast<char*>(workspace) + emd::round256((size_t)B * kPart * tiling(H, W).tiles * sizeof(double)));
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (ksize == 1)
        launch_moments<1>(x, B, H, W, rectify, mb, out, st);
    else
        launch_moments<3>(x, B, H, W, rectify, mb, out, st);
    return emd::check_launch("emd_laplacian_moments_f64");
}

extern "C" size_t emd_histogram01_workspace_bytes(int B, int H, int W, int normalize) {
    if (B < 1 || B > 65535 || H < 1 || W < 1 || H > kMaxExtent || W > kMaxExtent) return 0;
    if (!normalize) return 0;
    return emd::round256((size_t)B * chunks_of(H, W) * sizeof(double)) + emd::round256((size_t)B * 2 * sizeof(double));
}

extern "C" int emd_histogram01_i64(const float* x, int B, int H, int W, int bins, int normalize, int64_t* counts, void* workspace,
                                   size_t workspace_bytes, emd_stream_t stream) {
    if (!(B >= 0 && B <= 65535 && H >= 1 && W >= 1 && H <= kMaxExtent && W <= kMaxExtent)) {
        emd::set_error("emd_histogram01_i64: bad shape (batch 0..65535, 1 <= H, W <= %d; got %d x %d x %d)", kMaxExtent, B, H, W);
        return EMD_E_INVALID;
    }
    EMD_REQUIRE(bins_ok(bins), EMD_E_INVALID, "emd_histogram01_i64: bins must be a power of two, 2..4096");
    EMD_REQUIRE(normalize == 0 || normalize == 1, EMD_E_INVALID, "emd_histogram01_i64: normalize must be 0 or 1");
    if (B == 0) return EMD_OK;
    const size_t need = emd_histogram01_workspace_bytes(B, H, W, normalize);
    const emd::Range r[] = {{workspace, need, 16, !normalize, false},
                            {x, (size_t)B * H * W * sizeof(float), 4, false, true},
                            {counts, (size_t)B * bins * sizeof(int64_t), 8, false, false}};
    const int rc = emd::check_ranges("emd_histogram01_i64", r, 3, "the workspace must be 16-byte aligned, counts 8-byte, x 4-byte",
                                     &workspace_bytes);
    if (rc != EMD_OK) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const hipError_t e = hipMemsetAsync(counts, 0, (size_t)B * bins * sizeof(int64_t), st);
    if (e != hipSuccess) {
        emd::set_error("emd_histogram01_i64: hipMemsetAsync: %s", hipGetErrorString(e));
        return EMD_E_LAUNCH;
    }
    const long n = (long)H * W;
    const int chunks = chunks_of(H, W);
    const dim3 grid((unsigned)chunks, (unsigned)B), per_image((unsigned)B);
    NormBuffers nb{nullptr, nullptr};
    unsigned long long* c = reinterpret_cast<unsigned long long*>(counts);
    if (normalize) {
        nb.part = static_cast<double*>(workspace);
        nb.acc = reinterpret_cast<double*>(static_cast<char*>(workspace) + emd::round256((size_t)B * chunks * sizeof(double)));
        hipLaunchKernelGGL(chunk_sum_kernel<0>, grid, dim3(256), 0, st, x, n, nb);
        hipLaunchKernelGGL(norm_stage_kernel, per_image, dim3(256), 0, st, nb, chunks, (double)n, 0);
        hipLaunchKernelGGL(chunk_sum_kernel<1>, grid, dim3(256), 0, st, x, n, nb);
        hipLaunchKernelGGL(norm_stage_kernel, per_image, dim3(256), 0, st, nb, chunks, (double)n, 1);
        hipLaunchKernelGGL(hist01_kernel<true>, grid, dim3(256), 0, st, x, n, bins, nb, c);
    } else {
        hipLaunchKernelGGL(hist01_kernel<false>, grid, dim3(256), 0, st, x, n, bins, nb, c);
    }
    return emd::check_launch("emd_histogram01_i64");
}

extern "C" int emd_hist_entropy_f64(const int64_t* counts, int B, int bins, double eps, double* entropy, emd_stream_t stream) {
    EMD_REQUIRE(B >= 0 && B <= 65535, EMD_E_INVALID, "emd_hist_entropy_f64: the batch must be 0..65535");
    EMD_REQUIRE(bins >= 1 && bins <= (1 << 20), EMD_E_INVALID, "emd_hist_entropy_f64: 1 <= bins <= 2^20");
    EMD_REQUIRE(eps >= 0.0, EMD_E_INVALID, "emd_hist_entropy_f64: eps must be >= 0");
    if (B == 0) return EMD_OK;
    EMD_REQUIRE(counts && entropy, EMD_E_INVALID, "emd_hist_entropy_f64: null pointer");
    EMD_REQUIRE(!emd::overlap(counts, (size_t)B * bins * sizeof(int64_t), entropy, (size_t)B * sizeof(double)), EMD_E_INVALID,
                "emd_hist_entropy_f64: entropy may not overlap counts");
    hipLaunchKernelGGL(hist_entropy_kernel, dim3((unsigned)B), dim3(256), 0, static_cast<hipStream_t>(stream),
                       reinterpret_cast<const long long*>(counts), bins, eps, entropy);
    return emd::check_launch("hist_entropy_kernel");
}

extern "C" int emd_spline_argmin_f64(const double* z, const double* scores, int B, int N, int interp_factor, double* zbest, double* curve,
                                     int64_t* index, emd_stream_t stream) {
    EMD_REQUIRE(B >= 0 && B <= 65535, EMD_E_INVALID, "emd_spline_argmin_f64: the batch must be 0..65535");
    EMD_REQUIRE(N >= 4 && N <= kMaxKnots, EMD_E_INVALID, "emd_spline_argmin_f64: the cubic spline needs 4 <= N <= 256 samples");
    EMD_REQUIRE(interp_factor >= 1 && interp_factor <= kMaxFactor, EMD_E_INVALID, "emd_spline_argmin_f64: 1 <= interp_factor <= 4096");
    if (B == 0) return EMD_OK;
    const int G = interp_factor * N;
    const emd::Range r[] = {{z, (size_t)N * sizeof(double), 8, false, true},
                            {scores, (size_t)B * N * sizeof(double), 8, false, true},
                            {zbest, (size_t)B * sizeof(double), 8, false, false},
                            {curve, (size_t)B * G * sizeof(double), 8, true, false},
                            {index, (size_t)B * sizeof(int64_t), 8, true, false}};
    const int rc = emd::check_ranges("emd_spline_argmin_f64", r, 5, "every array must be 8-byte aligned");
    if (rc != EMD_OK) return rc;
    hipLaunchKernelGGL(spline_argmin_kernel, dim3((unsigned)B), dim3(256), 0, static_cast<hipStream_t>(stream), z, scores, N, G, zbest,
                       curve, reinterpret_cast<long long*>(index));
    return emd::check_launch("spline_argmin_kernel");
}
