// Affine registration of a focal series by Mattes mutual information, and warping (misc_py/evolutionary_align.m, misc_py/warp_stack.m;
// DESIGN.md 3.22).  The formulas are in include/emdenoise.h; everything that is compared bit for bit is evaluated in double with
// fp contract(off), operation by operation as the header writes it.
//
//   warp_affine_kernel      32 x 8 tiles of the output (reg_crop_kernel's shape): the pull map, four taps, float32 out
//   mi_samples_kernel       one Philox call per thread: four sample indices
//   mi_range_part_kernel    a workgroup owns a run of pixels of one image: (min, max) partial
//   mi_range_final_kernel   one wave per image: the partials -> (fmin, fmax, mmin, mmax) of the pair
//   mi_hist_kernel          a workgroup owns a run of <= ceil(n / G) samples of one pair: the 64-bit fixed-point joint histogram in LDS
//                           (integer LDS atomics: the sum does not depend on the order), stored whole as partial g of the pair
//   mi_final_kernel         one workgroup per pair: the partials summed, marginals, MI (the public metric)
//   affine_reset_kernel     the optimizer's state
//   affine_step_kernel      one workgroup per pair: MI as above, then one thread does the (1+1) evolution step on the 6 x 6 matrix
//   affine_normals_kernel   the optimizer's normals alone
//   affine_chain_kernel     one thread: the pair transforms chained onto the middle image
//   affine_limits_kernel    one thread: the common rectangle
//
// No floating-point atomics, fixed orders: bitwise reproducible.  Launches only; state, ranges and status words are read on the device.
#include <climits>
#include <cmath>

#include "emd_common.hpp"
#include "philox.hpp"
#include "wave_reduce.hpp"

namespace {

using emd::check_ranges;
using emd::Range;

constexpr int kMinHW = 8, kMaxHW = 4096, kMaxPairs = 64, kMaxImages = 65535, kMinBins = 8, kMaxBins = 64, kPad = 2;
constexpr int kSamplesPerPart = 1024, kMaxParts = 64;   // histogram partials per pair: G = min(ceil(n / 1024), 64)
constexpr int kRangePixels = 4096, kMaxRangeParts = 64; // (min, max) partials per image
constexpr int kStepThreads = 1024;                      // mi_final_kernel, affine_step_kernel
constexpr int kState = EMD_AFFINE_STATE_DOUBLES;
// the slots of a pair's state (doubles; the counters are 64-bit integers in the same slots)
constexpr int kSX = 0, kSA = 6, kSN = 42, kSChild = 48, kSF = 54, kSMi = 55, kSIter = 56, kSAccepted = 57, kSStatus = 58, kSWeight = 59, kSFresh = 60;

struct Geo {
    double cx, cy, h;
};

Geo geo_of(int H, int W) { return {(double)(W - 1) / 2.0, (double)(H - 1) / 2.0, (double)(H > W ? H : W) / 2.0}; }

bool shape_ok(int H, int W) { return H >= kMinHW && H <= kMaxHW && W >= kMinHW && W <= kMaxHW; }

struct T6 {
    double t[6];
};

// (u', v') = T (u, v, 1), then back to pixels
__device__ __forceinline__ void pull(const T6& T, const Geo& g, int x, int y, double& xs, double& ys) {
#pragma clang fp contract(off)
    const double u = ((double)x - g.cx) / g.h, v = ((double)y - g.cy) / g.h;
    const double us = (T.t[0] * u + T.t[1] * v) + T.t[2], vs = (T.t[3] * u + T.t[4] * v) + T.t[5];
    xs = us * g.h + g.cx;
    ys = vs * g.h + g.cy;
}

// floor and the fraction behind it; a coordinate that is not finite, or far outside, puts every tap outside
__device__ __forceinline__ void split(double c, long& i0, double& f) {
#pragma clang fp contract(off)
    const double fl = floor(c);
    f = c - fl;
    i0 = fl > -1e9 && fl < 1e9 ? (long)fl : -2000000000L;
}

__device__ __forceinline__ double bilinear(double fx, double fy, double p00, double p01, double p10, double p11) {
#pragma clang fp contract(off)
    return (1.0 - fy) * ((1.0 - fx) * p00 + fx * p01) + fy * ((1.0 - fx) * p10 + fx * p11);
}

// grid (ceil(W / 32), ceil(H / 8), N), block (32, 8).  T: [N][6], or [6] with shared != 0
__global__ __launch_bounds__(256) void warp_affine_kernel(const float* __restrict__ images, int H, int W, Geo g, const double* __restrict__ T,
                                                          int shared, float fill, float* __restrict__ out) {
    const int c = blockIdx.x * 32 + threadIdx.x, r = blockIdx.y * 8 + threadIdx.y;
    const long n = blockIdx.z;
    if (c >= W || r >= H) return;
    T6 t;
    const double* tp = T + (shared ? 0 : 6 * n);
#pragma unroll
    for (int j = 0; j < 6; ++j) t.t[j] = tp[j];
    double xs, ys, fx, fy;
    pull(t, g, c, r, xs, ys);
    long x, y;
    split(xs, x, fx);
    split(ys, y, fy);
    const float* img = images + n * H * W;
    const bool xin0 = x >= 0 && x < W, xin1 = x + 1 >= 0 && x + 1 < W, yin0 = y >= 0 && y < H, yin1 = y + 1 >= 0 && y + 1 < H;
    float v = fill;
    if ((xin0 || xin1) && (yin0 || yin1)) {
        const double pad = (double)fill;
        const double p00 = yin0 && xin0 ? (double)img[y * W + x] : pad, p01 = yin0 && xin1 ? (double)img[y * W + x + 1] : pad;
        const double p10 = yin1 && xin0 ? (double)img[(y + 1) * W + x] : pad, p11 = yin1 && xin1 ? (double)img[(y + 1) * W + x + 1] : pad;
        v = (float)bilinear(fx, fy, p00, p01, p10, p11);
    }
    out[(n * H + r) * W + c] = v;
}

// grid (ceil(ceil(n / 4) / 256)): thread j draws the samples 4 j .. 4 j + 3
__global__ __launch_bounds__(256) void mi_samples_kernel(unsigned* __restrict__ samples, int n, unsigned HW, unsigned k0, unsigned k1) {
    const unsigned j = blockIdx.x * 256u + threadIdx.x;
    if ((long)j * 4 >= n) return;
    const emd::U4 r = emd::philox4x32_10({j, 0u, 0u, emd::kPhiloxTagMiSamples}, k0, k1);
    const unsigned w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if ((long)j * 4 + k < n) samples[(long)j * 4 + k] = __umulhi(w[k], HW);
}

// grid (R, 2 P): image i is fixed[i] for i < P, else moving[i - P].  part: [2 P][R][2] = (min, max); NaN pixels are passed over
__global__ __launch_bounds__(256) void mi_range_part_kernel(const float* __restrict__ fixed, const float* __restrict__ moving, int P, long HW,
                                                            float* __restrict__ part) {
    __shared__ float smin[4], smax[4];
    const long i = blockIdx.y;
    const float* src = (int)i < P ? fixed + i * HW : moving + (i - P) * HW;
    const long R = gridDim.x, run = (HW + R - 1) / R, a = blockIdx.x * run, b = a + run < HW ? a + run : HW;
    float lo = INFINITY, hi = -INFINITY;
    for (long k = a + threadIdx.x; k < b; k += 256) {
        const float v = src[k];
        lo = fminf(lo, v);
        hi = fmaxf(hi, v);
    }
    lo = emd::wave_min(lo);
    hi = emd::wave_max(hi);
    if ((threadIdx.x & 63) == 0) {
        smin[threadIdx.x >> 6] = lo;
        smax[threadIdx.x >> 6] = hi;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        part[(i * R + blockIdx.x) * 2] = fminf(fminf(smin[0], smin[1]), fminf(smin[2], smin[3]));
        part[(i * R + blockIdx.x) * 2 + 1] = fmaxf(fmaxf(smax[0], smax[1]), fmaxf(smax[2], smax[3]));
    }
}

// grid (2 P), 64 threads, R <= 64.  ranges: [P][4] = (fmin, fmax, mmin, mmax)
__global__ __launch_bounds__(64) void mi_range_final_kernel(const float* __restrict__ part, int R, int P, float* __restrict__ ranges) {
    const int i = blockIdx.x, l = threadIdx.x;
    float lo = l < R ? part[((long)i * R + l) * 2] : INFINITY, hi = l < R ? part[((long)i * R + l) * 2 + 1] : -INFINITY;
    lo = emd::wave_min(lo);
    hi = emd::wave_max(hi);
    if (l == 0) {
        float* d = ranges + 4 * (i < P ? i : i - P) + (i < P ? 0 : 2);
        d[0] = lo;
        d[1] = hi;
    }
}

__device__ __forceinline__ bool range_ok(float lo, float hi) { return hi > lo && hi - lo < INFINITY; }   // false for NaN, empty and infinite

// (4 - 6 a^2 + 3 a^3) / 6 for a = |u| < 1, (2 - a)^3 / 6 for a < 2, else 0
__device__ __forceinline__ double bspline3(double u) {
#pragma clang fp contract(off)
    const double a = fabs(u);
    if (a < 1.0) {
        const double a2 = a * a, a3 = a2 * a;
        return ((4.0 - 6.0 * a2) + 3.0 * a3) / 6.0;
    }
    if (a < 2.0) {
        const double t = 2.0 - a;
        return ((t * t) * t) / 6.0;
    }
    return 0.0;
}

// t = (v - lo) / width + pad; j = clip(floor(t), pad, bins - pad - 1); lo for a t that is not a number
__device__ __forceinline__ int parzen_index(double v, double lo, double width, int bins, double& t) {
#pragma clang fp contract(off)
    t = (v - lo) / width + (double)kPad;
    const double fl = floor(t);
    const int jlo = kPad, jhi = bins - kPad - 1;
    return fl >= (double)jlo ? (fl <= (double)jhi ? (int)fl : jhi) : jlo;
}

// grid (G, P), bins^2 * 8 bytes of LDS.  The candidate of pair p is cand[p * cstride .. + 6], plus [I | 0] where add_identity (the
// optimizer's parameters).  status (may be NULL): a pair whose word at status[p * kState] is not 0 is passed over, as is a pair with a
// degenerate range; the consumer of the partials passes it over on the same condition.  partials: [P][G][bins^2].
__global__ __launch_bounds__(256) void mi_hist_kernel(const float* __restrict__ fixed, const float* __restrict__ moving, int H, int W, Geo g,
                                                      const double* __restrict__ cand, int cstride, int add_identity,
                                                      const unsigned* __restrict__ samples, int n, int bins, const float* __restrict__ ranges,
                                                      const long long* __restrict__ status, unsigned long long* __restrict__ partials) {
    extern __shared__ __align__(16) unsigned char smem[];
    unsigned long long* h = reinterpret_cast<unsigned long long*>(smem);
    const long p = blockIdx.y;
    if (status && status[p * kState] != 0) return;
    const float* rg = ranges + 4 * p;
    if (!range_ok(rg[0], rg[1]) || !range_ok(rg[2], rg[3])) return;
    const int tid = threadIdx.x, nb = bins * bins, G = gridDim.x;
    for (int b = tid; b < nb; b += 256) h[b] = 0ull;
    __syncthreads();
    T6 t;
#pragma unroll
    for (int j = 0; j < 6; ++j) t.t[j] = cand[p * cstride + j];
    if (add_identity) {
        t.t[0] += 1.0;
        t.t[4] += 1.0;
    }
    const long HW = (long)H * W;
    const float* fimg = fixed + p * HW;
    const float* mimg = moving + p * HW;
    const double fmin = (double)rg[0], mmin = (double)rg[2];
    const double bf = ((double)rg[1] - fmin) / (double)(bins - 2 * kPad), bm = ((double)rg[3] - mmin) / (double)(bins - 2 * kPad);
    const int run = (n + G - 1) / G, s0 = blockIdx.x * run, s1 = s0 + run < n ? s0 + run : n;
    for (int s = s0 + tid; s < s1; s += 256) {
        const long idx = samples ? (long)samples[s] : (long)s;
        if (idx >= HW) continue;   // a caller's index past the image
        const int y = (int)(idx / W), x = (int)(idx - (long)y * W);
        double xs, ys;
        pull(t, g, x, y, xs, ys);
        if (!(xs >= 0.0 && xs <= (double)(W - 1) && ys >= 0.0 && ys <= (double)(H - 1))) continue;
        long ix, iy;
        double fx, fy;
        split(xs, ix, fx);
        split(ys, iy, fy);
        const bool xin1 = ix + 1 < W, yin1 = iy + 1 < H;   // ix, iy themselves are inside
        const double p00 = (double)mimg[iy * W + ix], p01 = xin1 ? (double)mimg[iy * W + ix + 1] : 0.0;
        const double p10 = yin1 ? (double)mimg[(iy + 1) * W + ix] : 0.0, p11 = yin1 && xin1 ? (double)mimg[(iy + 1) * W + ix + 1] : 0.0;
        const double m = bilinear(fx, fy, p00, p01, p10, p11);
        double tf, tm;
        const int jf = parzen_index((double)fimg[idx], fmin, bf, bins, tf);
        const int jm = parzen_index(m, mmin, bm, bins, tm);
#pragma unroll
        for (int d = -1; d <= 2; ++d) {
            const double w = bspline3((double)(jm + d) - tm);
            const unsigned long long q = (unsigned long long)rint(w * 4294967296.0);   // w <= 2 / 3
            if (q) atomicAdd(&h[jf * bins + jm + d], q);                               // pad - 1 <= jm + d <= bins - pad + 1
        }
    }
    __syncthreads();
    unsigned long long* dst = partials + (p * G + blockIdx.x) * nb;
    for (int b = tid; b < nb; b += 256) dst[b] = h[b];
}

// The G partials of one pair summed into h (LDS, bins^2), the marginals into marg (LDS, 129: rows, columns at 64, the total at 128), and
// MI = the sum, over the bins in row-major order, of P log(P / (pf pm)) (0 for an empty bin), by thread 0 alone: valid in thread 0.  The
// histogram goes to hist_out where that is not NULL.  blockDim.x >= 128.  h holds the terms afterwards.
__device__ __forceinline__ double mi_value(const unsigned long long* __restrict__ part, int G, int bins, unsigned long long* __restrict__ hist_out,
                                           unsigned long long* h, unsigned long long* marg) {
#pragma clang fp contract(off)
    const int tid = threadIdx.x, nt = blockDim.x, nb = bins * bins;
    for (int b = tid; b < nb; b += nt) {
        unsigned long long s = 0ull;
        for (int k = 0; k < G; ++k) s += part[(long)k * nb + b];
        h[b] = s;
        if (hist_out) hist_out[b] = s;
    }
    __syncthreads();
    if (tid < bins) {
        unsigned long long s = 0ull;
        for (int c = 0; c < bins; ++c) s += h[tid * bins + c];
        marg[tid] = s;
    } else if (tid >= 64 && tid - 64 < bins) {
        unsigned long long s = 0ull;
        for (int r = 0; r < bins; ++r) s += h[r * bins + tid - 64];
        marg[tid] = s;
    }
    __syncthreads();
    if (tid == 0) {
        unsigned long long s = 0ull;
        for (int r = 0; r < bins; ++r) s += marg[r];
        marg[128] = s;
    }
    __syncthreads();
    const unsigned long long total = marg[128];
    const double dn = (double)total;
    double* term = reinterpret_cast<double*>(h);
    for (int b = tid; b < nb; b += nt) {
        const unsigned long long hv = h[b];
        double v = 0.0;
        if (hv) {
            const double P = (double)hv / dn, pf = (double)marg[b / bins] / dn, pm = (double)marg[64 + b % bins] / dn;
            v = P * log(P / (pf * pm));
        }
        term[b] = v;
    }
    __syncthreads();
    double mi = 0.0;
    if (tid == 0 && total)
        for (int b = 0; b < nb; ++b) mi += term[b];
    return mi;
}

// grid (P), kStepThreads, bins^2 * 8 + 129 * 8 bytes of LDS.  status: EMD_MI_CONSTANT, EMD_MI_EMPTY or 0
__global__ __launch_bounds__(kStepThreads) void mi_final_kernel(const unsigned long long* __restrict__ partials, int G, int bins,
                                                                const float* __restrict__ ranges, double* __restrict__ mi, int* __restrict__ status,
                                                                unsigned long long* __restrict__ hist) {
    extern __shared__ __align__(16) unsigned char smem[];
    unsigned long long* h = reinterpret_cast<unsigned long long*>(smem);
    unsigned long long* marg = h + bins * bins;
    const long p = blockIdx.x;
    const int nb = bins * bins;
    const float* rg = ranges + 4 * p;
    if (!range_ok(rg[0], rg[1]) || !range_ok(rg[2], rg[3])) {
        if (hist)
            for (int b = threadIdx.x; b < nb; b += blockDim.x) hist[p * nb + b] = 0ull;
        if (threadIdx.x == 0) {
            mi[p] = 0.0;
            status[p] = EMD_MI_CONSTANT;
        }
        return;
    }
    const double v = mi_value(partials + p * G * nb, G, bins, hist ? hist + p * nb : nullptr, h, marg);
    if (threadIdx.x == 0) {
        mi[p] = v;
        status[p] = marg[128] ? 0 : EMD_MI_EMPTY;
    }
}

// z = sqrt(-2 log u1) (cospi(2 u2), sinpi(2 u2)), u = (r + 0.5) 2^-32, from the first two words of the Philox call (it, pair, draw, TAG)
__device__ __forceinline__ void normal_pair(unsigned k0, unsigned k1, unsigned it, unsigned pair, unsigned draw, double& z0, double& z1) {
#pragma clang fp contract(off)
    const emd::U4 r = emd::philox4x32_10({it, pair, draw, emd::kPhiloxTagAffineNormal}, k0, k1);
    const double u1 = ((double)r.x + 0.5) * 0x1p-32, u2 = ((double)r.y + 0.5) * 0x1p-32;
    const double rad = sqrt(-2.0 * log(u1));
    double s, c;
    sincospi(2.0 * u2, &s, &c);
    z0 = rad * c;
    z1 = rad * s;
}

// grid (ceil(iterations * P * 3 / 256)).  out: [iterations][P][6], iteration first + i
__global__ __launch_bounds__(256) void affine_normals_kernel(double* __restrict__ out, int iterations, int P, unsigned first, unsigned k0, unsigned k1) {
    const long j = (long)blockIdx.x * 256 + threadIdx.x;
    if (j >= (long)iterations * P * 3) return;
    const unsigned draw = (unsigned)(j % 3), pair = (unsigned)((j / 3) % P), it = first + (unsigned)(j / (3 * P));
    normal_pair(k0, k1, it, pair, draw, out[2 * j], out[2 * j + 1]);
}

// grid (P), 64 threads.  mode 1: x = T0 - [I | 0] (T0 NULL: 0), the counters to first_iteration, 0; mode 2: x and the counters stay.
// Either way A = radius I, the child is x itself, the next evaluation is the parent's and the status is 0.
__global__ __launch_bounds__(64) void affine_reset_kernel(double* __restrict__ state, const double* __restrict__ T0, int mode, double radius,
                                                          long long first_iteration) {
    double* s = state + (long)blockIdx.x * kState;
    long long* si = reinterpret_cast<long long*>(s);
    const int l = threadIdx.x;
    if (mode == 1 && l < 6) s[kSX + l] = T0 ? T0[blockIdx.x * 6 + l] - (l == 0 || l == 4 ? 1.0 : 0.0) : 0.0;
    __syncthreads();
    if (l < 36) s[kSA + l] = l / 6 == l % 6 ? radius : 0.0;
    if (l < 6) {
        s[kSN + l] = 0.0;
        s[kSChild + l] = s[kSX + l];
    }
    if (l == 0) {
        si[kSStatus] = 0;
        si[kSFresh] = 1;
        si[kSWeight] = 0;
        if (mode == 1) {
            s[kSF] = 0.0;
            s[kSMi] = 0.0;
            si[kSIter] = first_iteration;
            si[kSAccepted] = 0;
            for (int k = kSFresh + 1; k < kState; ++k) s[k] = 0.0;
        }
    }
}

struct StepArgs {
    double growth, shrink, epsilon;
    const double* variates;   // [rows][P][6], or NULL: Philox
    long long rows;
    unsigned k0, k1;
};

// grid (P), kStepThreads, bins^2 * 8 + 129 * 8 bytes of LDS: the value of the candidate that mi_hist_kernel evaluated, then thread 0:
// accept or reject, A <- A + ((factor - 1) / (n'n)) (A n) n', convergence, the next normals and the next child x + A n.
__global__ __launch_bounds__(kStepThreads) void affine_step_kernel(const unsigned long long* __restrict__ partials, int G, int bins,
                                                                   const float* __restrict__ ranges, int P, StepArgs a, double* __restrict__ state) {
#pragma clang fp contract(off)
    extern __shared__ __align__(16) unsigned char smem[];
    unsigned long long* h = reinterpret_cast<unsigned long long*>(smem);
    unsigned long long* marg = h + bins * bins;
    const long p = blockIdx.x;
    double* s = state + p * kState;
    long long* si = reinterpret_cast<long long*>(s);
    if (si[kSStatus] != 0) return;
    const float* rg = ranges + 4 * p;
    if (!range_ok(rg[0], rg[1]) || !range_ok(rg[2], rg[3])) {
        if (threadIdx.x == 0) {
            si[kSStatus] = EMD_AFFINE_DEGENERATE;
            s[kSF] = 0.0;
            s[kSMi] = 0.0;
        }
        return;
    }
    const double mi = mi_value(partials + p * G * bins * bins, G, bins, nullptr, h, marg);
    if (threadIdx.x) return;
    const long long t = si[kSIter];
    double x[6], A[36], nv[6];
    for (int j = 0; j < 6; ++j) x[j] = s[kSX + j];
    for (int j = 0; j < 36; ++j) A[j] = s[kSA + j];
    s[kSMi] = mi;
    si[kSWeight] = (long long)marg[128];
    si[kSIter] = t + 1;
    if (si[kSFresh]) {   // the parent's own value
        si[kSFresh] = 0;
        s[kSF] = mi;
    } else {
        const bool accept = mi > s[kSF];
        if (accept) {
            for (int j = 0; j < 6; ++j) x[j] = s[kSX + j] = s[kSChild + j];
            s[kSF] = mi;
            si[kSAccepted] += 1;
        }
        for (int j = 0; j < 6; ++j) nv[j] = s[kSN + j];
        double nn = 0.0;
        for (int j = 0; j < 6; ++j) nn += nv[j] * nv[j];
        if (nn > 0.0) {
            const double c = ((accept ? a.growth : a.shrink) - 1.0) / nn;
            double d[6];
            for (int i = 0; i < 6; ++i) {
                double v = A[i * 6] * nv[0];
                for (int j = 1; j < 6; ++j) v += A[i * 6 + j] * nv[j];
                d[i] = v;
            }
            for (int i = 0; i < 6; ++i)
                for (int j = 0; j < 6; ++j) s[kSA + i * 6 + j] = A[i * 6 + j] = A[i * 6 + j] + (c * d[i]) * nv[j];
        }
        double fro = 0.0;
        for (int j = 0; j < 36; ++j) fro += A[j] * A[j];
        if (sqrt(fro) < a.epsilon) {
            si[kSStatus] = EMD_AFFINE_CONVERGED;
            return;
        }
    }
    if (a.variates) {
        if (t < 0 || t >= a.rows) {   // the caller's stream has run out
            si[kSStatus] = EMD_AFFINE_EXHAUSTED;
            return;
        }
        for (int j = 0; j < 6; ++j) nv[j] = a.variates[(t * P + p) * 6 + j];
    } else {
        for (int d = 0; d < 3; ++d) normal_pair(a.k0, a.k1, (unsigned)t, (unsigned)p, (unsigned)d, nv[2 * d], nv[2 * d + 1]);
    }
    for (int i = 0; i < 6; ++i) {
        double v = A[i * 6] * nv[0];
        for (int j = 1; j < 6; ++j) v += A[i * 6 + j] * nv[j];
        s[kSChild + i] = x[i] + v;
        s[kSN + i] = nv[i];
    }
}

// ---- chaining onto the middle image ---------------------------------------------------------------------------------------------

struct M3 {
    double m[9];
};

__device__ __forceinline__ bool finite6(const double* t) {
    bool ok = true;
    for (int j = 0; j < 6; ++j) ok = ok && isfinite(t[j]);
    return ok;
}

__device__ __forceinline__ M3 hom(const double* t) {
    M3 r;
    for (int j = 0; j < 6; ++j) r.m[j] = t[j];
    r.m[6] = 0.0;
    r.m[7] = 0.0;
    r.m[8] = 1.0;
    return r;
}

// a pair transform the chain can go through in either direction: finite, with a determinant that is finite and not 0
__device__ __forceinline__ bool regular6(const double* t) {
#pragma clang fp contract(off)
    const double det = t[0] * t[4] - t[1] * t[3];
    return finite6(t) && isfinite(det) && det != 0.0;
}

__device__ __forceinline__ M3 nan3() {
    M3 r;
    for (int j = 0; j < 6; ++j) r.m[j] = NAN;
    r.m[6] = 0.0;
    r.m[7] = 0.0;
    r.m[8] = 1.0;
    return r;
}

// c_ik = (a_i0 b_0k + a_i1 b_1k) + a_i2 b_2k
__device__ __forceinline__ M3 mul3(const M3& a, const M3& b) {
#pragma clang fp contract(off)
    M3 c;
    for (int i = 0; i < 3; ++i)
        for (int k = 0; k < 3; ++k) c.m[i * 3 + k] = (a.m[i * 3] * b.m[k] + a.m[i * 3 + 1] * b.m[3 + k]) + a.m[i * 3 + 2] * b.m[6 + k];
    return c;
}

// the inverse of [a b c; d e f; 0 0 1] by the adjugate; NaNs for a singular or non-finite matrix
__device__ __forceinline__ M3 inv3(const double* t) {
#pragma clang fp contract(off)
    const double a = t[0], b = t[1], c = t[2], d = t[3], e = t[4], f = t[5];
    const double det = a * e - b * d;
    if (!regular6(t)) return nan3();
    M3 r;
    r.m[0] = e / det;
    r.m[1] = -b / det;
    r.m[2] = (b * f - c * e) / det;
    r.m[3] = -d / det;
    r.m[4] = a / det;
    r.m[5] = (c * d - a * f) / det;
    r.m[6] = 0.0;
    r.m[7] = 0.0;
    r.m[8] = 1.0;
    return r;
}

// one thread.  Tp: [N - 1][6]; C: [N][6]
__global__ void affine_chain_kernel(const double* __restrict__ Tp, int N, int middle, double* __restrict__ C) {
    if (blockIdx.x || threadIdx.x) return;
    M3 cur;
    for (int j = 0; j < 6; ++j) C[middle * 6 + j] = j == 0 || j == 4 ? 1.0 : 0.0;
    for (int dir = 0; dir < 2; ++dir) {
        for (int j = 0; j < 9; ++j) cur.m[j] = j % 4 == 0 ? 1.0 : 0.0;
        if (dir == 0) {
            for (int j = middle + 1; j < N; ++j) {
                const double* t = Tp + (j - 1) * 6;
                cur = regular6(t) ? mul3(hom(t), cur) : nan3();
                for (int k = 0; k < 6; ++k) C[j * 6 + k] = cur.m[k];
            }
        } else {
            for (int j = middle - 1; j >= 0; --j) {
                cur = mul3(inv3(Tp + j * 6), cur);
                for (int k = 0; k < 6; ++k) C[j * 6 + k] = cur.m[k];
            }
        }
    }
}

// one thread.  limits: [4] = (x0, y0, w, h)
__global__ void affine_limits_kernel(const double* __restrict__ C, int N, int H, int W, Geo g, int* __restrict__ limits) {
#pragma clang fp contract(off)
    if (blockIdx.x || threadIdx.x) return;
    double left = 0.0, top = 0.0, right = (double)(W - 1), bottom = (double)(H - 1);
    bool ok = true;
    const double X[4] = {0.0, (double)(W - 1), (double)(W - 1), 0.0}, Y[4] = {0.0, 0.0, (double)(H - 1), (double)(H - 1)};
    for (int j = 0; j < N; ++j) {
        const M3 D = inv3(C + j * 6);
        double xs[4], ys[4];
        for (int k = 0; k < 4; ++k) {
            xs[k] = (D.m[0] * (X[k] - g.cx) + D.m[1] * (Y[k] - g.cy)) + (D.m[2] * g.h + g.cx);
            ys[k] = (D.m[3] * (X[k] - g.cx) + D.m[4] * (Y[k] - g.cy)) + (D.m[5] * g.h + g.cy);
            ok = ok && isfinite(xs[k]) && isfinite(ys[k]);
        }
        if (!ok) break;
        left = fmax(left, ceil(fmax(xs[0], xs[3])));
        right = fmin(right, floor(fmin(xs[1], xs[2])));
        top = fmax(top, ceil(fmax(ys[0], ys[1])));
        bottom = fmin(bottom, floor(fmin(ys[2], ys[3])));
    }
    const double w = right - left + 1.0, h = bottom - top + 1.0;
    if (!ok || !(w > 0.0) || !(h > 0.0)) {
        limits[0] = ok ? (int)fmin(left, (double)(W - 1)) : 0;
        limits[1] = ok ? (int)fmin(top, (double)(H - 1)) : 0;
        limits[2] = ok && w > 0.0 ? (int)w : 0;
        limits[3] = ok && h > 0.0 ? (int)h : 0;
        return;
    }
    limits[0] = (int)left;
    limits[1] = (int)top;
    limits[2] = (int)w;
    limits[3] = (int)h;
}

// ---- host side -----------------------------------------------------------------------------------------------------------

struct MiLayout {
    size_t part, ranges, hist, bytes;
    int R, G, n;
};

bool mi_shape_ok(int P, int H, int W, int n, int bins) {
    return P >= 1 && P <= kMaxPairs && shape_ok(H, W) && bins >= kMinBins && bins <= kMaxBins && n >= 0 && (long)n <= (long)H * W * 4;
}

// n == 0: every pixel
MiLayout mi_layout(int P, int H, int W, int n, int bins) {
    MiLayout l{};
    const long HW = (long)H * W;
    l.n = n ? n : (int)HW;
    l.R = (int)((HW + kRangePixels - 1) / kRangePixels);
    if (l.R > kMaxRangeParts) l.R = kMaxRangeParts;
    l.G = emd::tiles_of(l.n, kSamplesPerPart);
    if (l.G > kMaxParts) l.G = kMaxParts;
    size_t bytes = 0;
    l.part = bytes;
    bytes += emd::round256((size_t)2 * P * l.R * 2 * sizeof(float));
    l.ranges = bytes;
    bytes += emd::round256((size_t)P * 4 * sizeof(float));
    l.hist = bytes;
    bytes += emd::round256((size_t)P * l.G * bins * bins * sizeof(unsigned long long));
    l.bytes = bytes;
    return l;
}

const char* kMiShape = "%s: bad shape (1..%d pairs, H and W %d..%d, bins %d..%d, 0 <= n <= 4 H W; got %d pairs of %d x %d, bins %d, n %d)";

void launch_ranges(const float* fixed, const float* moving, int P, int H, int W, const MiLayout& l, char* ws, hipStream_t st) {
    float* part = reinterpret_cast<float*>(ws + l.part);
    hipLaunchKernelGGL(mi_range_part_kernel, dim3((unsigned)l.R, (unsigned)(2 * P)), dim3(256), 0, st, fixed, moving, P, (long)H * W, part);
    hipLaunchKernelGGL(mi_range_final_kernel, dim3((unsigned)(2 * P)), dim3(64), 0, st, part, l.R, P, reinterpret_cast<float*>(ws + l.ranges));
}

}  // namespace

extern "C" int emd_warp_affine_f32(const float* images, int N, int H, int W, const double* T, int shared_T, float fill, float* out,
                                   emd_stream_t stream) {
    const char* who = "emd_warp_affine_f32";
    if (N < 1 || N > kMaxImages || !shape_ok(H, W)) {
        emd::set_error("%s: bad shape (1..%d images, H and W %d..%d; got %d of %d x %d)", who, kMaxImages, kMinHW, kMaxHW, N, H, W);
        return EMD_E_INVALID;
    }
    const size_t plane = (size_t)H * W * sizeof(float);
    const Range r[] = {{images, N * plane, 4, false, true}, {out, N * plane, 4, false, false},
                       {T, (size_t)(shared_T ? 1 : N) * 6 * sizeof(double), 8, false, true}};
    const int rc = check_ranges(who, r, 3, "T must be 8-byte aligned, images and out 4-byte");
    if (rc != EMD_OK) return rc;
    hipLaunchKernelGGL(warp_affine_kernel, dim3((unsigned)emd::tiles_of(W, 32), (unsigned)emd::tiles_of(H, 8), (unsigned)N), dim3(32, 8), 0,
                       static_cast<hipStream_t>(stream), images, H, W, geo_of(H, W), T, shared_T ? 1 : 0, fill, out);
    return emd::check_launch(who);
}

extern "C" int emd_mi_samples_u32(int n, int H, int W, uint64_t seed, uint32_t* samples, emd_stream_t stream) {
    const char* who = "emd_mi_samples_u32";
    if (!shape_ok(H, W) || n < 1 || (long)n > (long)H * W * 4) {
        emd::set_error("%s: bad shape (H and W %d..%d, 1 <= n <= 4 H W; got %d x %d, n %d)", who, kMinHW, kMaxHW, H, W, n);
        return EMD_E_INVALID;
    }
    const Range r[] = {{samples, (size_t)n * sizeof(uint32_t), 4, false, false}};
    const int rc = check_ranges(who, r, 1, "samples must be 4-byte aligned");
    if (rc != EMD_OK) return rc;
    hipLaunchKernelGGL(mi_samples_kernel, dim3((unsigned)emd::tiles_of(emd::tiles_of(n, 4), 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       samples, n, (unsigned)(H * W), (unsigned)seed, (unsigned)(seed >> 32));
    return emd::check_launch(who);
}

extern "C" size_t emd_mattes_mi_workspace_bytes(int P, int H, int W, int n, int bins) {
    return mi_shape_ok(P, H, W, n, bins) ? mi_layout(P, H, W, n, bins).bytes : 0;
}

extern "C" int emd_mattes_mi_f64(const float* fixed, const float* moving, int P, int H, int W, const double* T, const uint32_t* samples, int n,
                                 int bins, double* mi, int* status, uint64_t* hist, void* workspace, size_t workspace_bytes,
                                 emd_stream_t stream) {
    const char* who = "emd_mattes_mi_f64";
    if (!mi_shape_ok(P, H, W, n, bins) || (samples != nullptr) != (n > 0)) {
        emd::set_error(kMiShape, who, kMaxPairs, kMinHW, kMaxHW, kMinBins, kMaxBins, P, H, W, bins, n);
        return EMD_E_INVALID;
    }
    const MiLayout l = mi_layout(P, H, W, n, bins);
    const size_t plane = (size_t)H * W * sizeof(float), nb = (size_t)bins * bins;
    const Range r[] = {{workspace, l.bytes, 16, false, false},
                       {fixed, P * plane, 4, false, true},
                       {moving, P * plane, 4, false, true},
                       {T, (size_t)P * 6 * sizeof(double), 8, false, true},
                       {samples, (size_t)n * sizeof(uint32_t), 4, true, true},
                       {mi, (size_t)P * sizeof(double), 8, false, false},
                       {status, (size_t)P * sizeof(int), 4, false, false},
                       {hist, P * nb * sizeof(uint64_t), 8, true, false}};
    const int rc = check_ranges(who, r, 8, "the workspace must be 16-byte aligned, T, mi and hist 8-byte, images, samples and status 4-byte",
                                &workspace_bytes);
    if (rc != EMD_OK) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    char* ws = static_cast<char*>(workspace);
    const float* ranges = reinterpret_cast<const float*>(ws + l.ranges);
    unsigned long long* partials = reinterpret_cast<unsigned long long*>(ws + l.hist);
    launch_ranges(fixed, moving, P, H, W, l, ws, st);
    hipLaunchKernelGGL(mi_hist_kernel, dim3((unsigned)l.G, (unsigned)P), dim3(256), nb * 8, st, fixed, moving, H, W, geo_of(H, W), T, 6, 0, samples,
                       l.n, bins, ranges, static_cast<const long long*>(nullptr), partials);
    hipLaunchKernelGGL(mi_final_kernel, dim3((unsigned)P), dim3(kStepThreads), (nb + 129) * 8, st, partials, l.G, bins, ranges, mi, status,
                       reinterpret_cast<unsigned long long*>(hist));
    return emd::check_launch(who);
}

extern "C" int emd_affine_normals_f64(int iterations, int P, int first_iteration, uint64_t seed, double* normals, emd_stream_t stream) {
    const char* who = "emd_affine_normals_f64";
    if (iterations < 1 || iterations > (1 << 20) || P < 1 || P > kMaxPairs || first_iteration < 0) {
        emd::set_error("%s: bad shape (1..%d iterations from a first one >= 0, 1..%d pairs; got %d from %d, %d pairs)", who, 1 << 20, kMaxPairs,
                       iterations, first_iteration, P);
        return EMD_E_INVALID;
    }
    const Range r[] = {{normals, (size_t)iterations * P * 6 * sizeof(double), 8, false, false}};
    const int rc = check_ranges(who, r, 1, "normals must be 8-byte aligned");
    if (rc != EMD_OK) return rc;
    hipLaunchKernelGGL(affine_normals_kernel, dim3((unsigned)emd::tiles_of(iterations * P * 3, 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       normals, iterations, P, (unsigned)first_iteration, (unsigned)seed, (unsigned)(seed >> 32));
    return emd::check_launch(who);
}

extern "C" int emd_affine_register_f64(const float* fixed, const float* moving, int P, int H, int W, const uint32_t* samples, int n, int bins,
                                       double initial_radius, double growth, double epsilon, uint64_t seed, const double* variates,
                                       int variates_rows, int flags, const double* T0, int first_iteration, int iterations, double* state,
                                       void* workspace, size_t workspace_bytes, emd_stream_t stream) {
    const char* who = "emd_affine_register_f64";
    if (!mi_shape_ok(P, H, W, n, bins) || (samples != nullptr) != (n > 0)) {
        emd::set_error(kMiShape, who, kMaxPairs, kMinHW, kMaxHW, kMinBins, kMaxBins, P, H, W, bins, n);
        return EMD_E_INVALID;
    }
    const int mode = flags & (EMD_AFFINE_RESET | EMD_AFFINE_NEXT_LEVEL);
    if (iterations < 0 || iterations > (1 << 20) || first_iteration < 0 || (flags & ~(EMD_AFFINE_RESET | EMD_AFFINE_NEXT_LEVEL)) || mode == 3 ||
        (variates != nullptr) != (variates_rows > 0) || (T0 && mode != EMD_AFFINE_RESET)) {
        emd::set_error("%s: bad arguments (0..%d iterations, first_iteration >= 0, flags EMD_AFFINE_RESET or EMD_AFFINE_NEXT_LEVEL, variates_rows "
                       "> 0 with variates and 0 without, T0 only with EMD_AFFINE_RESET; got %d iterations, first %d, flags %d, %d rows)", who,
                       1 << 20, iterations, first_iteration, flags, variates_rows);
        return EMD_E_INVALID;
    }
    if (!(initial_radius > 0.0 && initial_radius < INFINITY && growth > 1.0 && growth < INFINITY && epsilon >= 0.0 && epsilon < INFINITY)) {
        emd::set_error("%s: initial_radius > 0, growth > 1 and epsilon >= 0, all finite (got %g, %g, %g)", who, initial_radius, growth, epsilon);
        return EMD_E_INVALID;
    }
    const MiLayout l = mi_layout(P, H, W, n, bins);
    const size_t plane = (size_t)H * W * sizeof(float), nb = (size_t)bins * bins;
    const Range r[] = {{workspace, l.bytes, 16, false, false},
                       {fixed, P * plane, 4, false, true},
                       {moving, P * plane, 4, false, true},
                       {samples, (size_t)n * sizeof(uint32_t), 4, true, true},
                       {variates, (size_t)variates_rows * P * 6 * sizeof(double), 8, true, true},
                       {T0, (size_t)P * 6 * sizeof(double), 8, true, true},
                       {state, (size_t)P * kState * sizeof(double), 8, false, false}};
    const int rc = check_ranges(who, r, 7, "the workspace must be 16-byte aligned, state, variates and T0 8-byte, images and samples 4-byte",
                                &workspace_bytes);
    if (rc != EMD_OK) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    char* ws = static_cast<char*>(workspace);
    const float* ranges = reinterpret_cast<const float*>(ws + l.ranges);
    unsigned long long* partials = reinterpret_cast<unsigned long long*>(ws + l.hist);
    if (mode)
        hipLaunchKernelGGL(affine_reset_kernel, dim3((unsigned)P), dim3(64), 0, st, state, T0, mode, initial_radius, (long long)first_iteration);
    if (iterations) launch_ranges(fixed, moving, P, H, W, l, ws, st);
    const StepArgs a = {growth, sqrt(sqrt(1.0 / growth)), epsilon, variates, (long long)variates_rows, (unsigned)seed, (unsigned)(seed >> 32)};
    const Geo g = geo_of(H, W);
    for (int it = 0; it < iterations; ++it) {
        hipLaunchKernelGGL(mi_hist_kernel, dim3((unsigned)l.G, (unsigned)P), dim3(256), nb * 8, st, fixed, moving, H, W, g, state + kSChild, kState, 1,
                           samples, l.n, bins, ranges, reinterpret_cast<const long long*>(state) + kSStatus, partials);
        hipLaunchKernelGGL(affine_step_kernel, dim3((unsigned)P), dim3(kStepThreads), (nb + 129) * 8, st, partials, l.G, bins, ranges, P, a, state);
    }
    return emd::check_launch(who);
}

extern "C" int emd_affine_chain_f64(const double* T_pairs, int N, int middle, double* C, emd_stream_t stream) {
    const char* who = "emd_affine_chain_f64";
    if (N < 1 || N > kMaxPairs + 1 || middle < 0 || middle >= N) {
        emd::set_error("%s: bad shape (1..%d images, 0 <= middle < N; got %d, middle %d)", who, kMaxPairs + 1, N, middle);
        return EMD_E_INVALID;
    }
    const Range r[] = {{T_pairs, (size_t)(N - 1) * 6 * sizeof(double), 8, N == 1, true}, {C, (size_t)N * 6 * sizeof(double), 8, false, false}};
    const int rc = check_ranges(who, r, 2, "T_pairs and C must be 8-byte aligned");
    if (rc != EMD_OK) return rc;
    hipLaunchKernelGGL(affine_chain_kernel, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), T_pairs, N, middle, C);
    return emd::check_launch(who);
}

extern "C" int emd_affine_limits_i32(const double* C, int N, int H, int W, int* limits, emd_stream_t stream) {
    const char* who = "emd_affine_limits_i32";
    if (N < 1 || N > kMaxPairs + 1 || !shape_ok(H, W)) {
        emd::set_error("%s: bad shape (1..%d images, H and W %d..%d; got %d of %d x %d)", who, kMaxPairs + 1, kMinHW, kMaxHW, N, H, W);
        return EMD_E_INVALID;
    }
    const Range r[] = {{C, (size_t)N * 6 * sizeof(double), 8, false, true}, {limits, 4 * sizeof(int), 4, false, false}};
    const int rc = check_ranges(who, r, 2, "C must be 8-byte aligned, limits 4-byte");
    if (rc != EMD_OK) return rc;
    hipLaunchKernelGGL(affine_limits_kernel, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), C, N, H, W, geo_of(H, W), limits);
    return emd::check_launch(who);
}
