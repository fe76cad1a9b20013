// Dose series on the device (the rules are in include/emdenoise.h): the arithmetic of the reference's
// misc_py/lq_img_gen-backup.py:6-91 (lq_chunks_gen, record_lq, lq_img_gen) in integers -- a micrograph as an unnormalised probability
// density, a fixed number of electrons thrown at it through its cumulative sum.
//   dose_fill_kernel        the words the atomics start from (the maxima, the status, min and max)
//   dose_max_kernel         the largest positive finite pixel: one integer atomicMax per workgroup on the float's bit pattern
//   dose_tile_sum_kernel    q = rint(x / m * 2^32) recomputed from x and m, one 64-bit sum per tile of kTile pixels
//   dose_scan_sums_kernel   one workgroup per image: the tiles' sums -> the tiles' offsets, in place
//   dose_tile_scan_kernel   q again, the inclusive scan inside the tile (wave_scan.hpp), + the tile's offset -> the CDF
//   dose_draw_kernel        grid-stride over Philox calls, two draws each: target t = (r T) >> 64, the pixel by a search of a table of
//                           the CDF in LDS, then between two of its entries in global memory; one integer atomicAdd per electron
//   dose_cumulate_kernel    increment planes -> cumulative planes in place, and every plane's min and max (integer atomics)
//   dose_rescale_kernel     record_lq's min-max rescale to 16 bits, or to [0, 1]
// Integers throughout, so every output is exact and independent of the order of the additions.  No launch waits on another
// workgroup: the scan is separate launches.  Launches only.
#include <cfloat>

#include "emd_common.hpp"
#include "philox.hpp"
#include "wave_reduce.hpp"
#include "wave_scan.hpp"

namespace {

typedef unsigned long long u64;

constexpr int kMaxExtent = 32768;        // H, W
constexpr long kMaxPixels = 1L << 30;    // H W: the total T <= 2^30 2^32 fits an int64
constexpr int kTile = EMD_DOSE_TILE;     // pixels per tile: 256 threads x 2 pixels x 4 steps
constexpr int kStep = 512;               // pixels of one step of the tile scan
constexpr int kCoarse = EMD_DOSE_COARSE; // entries of the draw kernel's table in LDS
constexpr int kMaxLevels = EMD_DOSE_MAX_LEVELS;
constexpr int kChunk = 4096;             // pixels per workgroup of the cumulate kernel: 16 per thread
static_assert(kTile == 4 * kStep && kStep == 2 * 256, "the tile scan's shape");

// A pixel that weighs: positive and finite (NaN fails the first comparison).
__device__ __forceinline__ bool weighs(float x) { return x > 0.f && x <= FLT_MAX; }

// q = rint(double(x) / double(m) * 2^32): an IEEE division, an exact scaling, one rounding to an integer in 0 .. 2^32.
__device__ __forceinline__ u64 weight(float x, double m) {
    return weighs(x) ? (u64)__double2ull_rn(((double)x / m) * 4294967296.0) : 0ull;
}

// grid (tiles, B).  maxw[b]: the bit pattern of the largest weighing pixel (non-negative floats order as their bits), zeroed by dose_fill_kernel.
__global__ __launch_bounds__(256) void dose_max_kernel(const float* __restrict__ x, long n, unsigned* __restrict__ maxw,
                                                       int* __restrict__ status) {
    __shared__ float shm[4];
    __shared__ int shf[4];
    const long b = blockIdx.y, begin = (long)blockIdx.x * kTile, end = begin + kTile < n ? begin + kTile : n;
    const float* xb = x + b * n;
    float m = 0.f;
    int bad = 0;
    for (long i = begin + threadIdx.x; i < end; i += 256) {
        const float v = xb[i];
        if (weighs(v)) m = fmaxf(m, v);
        bad |= !(v >= 0.f && v <= FLT_MAX);   // negative, infinite or NaN (-0 is a zero, not a negative)
    }
    m = emd::wave_max(m);
    bad = emd::wave_or(bad);
    if ((threadIdx.x & 63) == 0) {
        shm[threadIdx.x >> 6] = m;
        shf[threadIdx.x >> 6] = bad;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        m = fmaxf(fmaxf(shm[0], shm[1]), fmaxf(shm[2], shm[3]));
        bad = shf[0] | shf[1] | shf[2] | shf[3];
        if (m > 0.f) atomicMax(&maxw[b], __float_as_uint(m));
        if (bad && status) atomicOr(&status[b], EMD_DOSE_SANITIZED);
    }
}

// grid (tiles, B): sums[b][tile] = the sum of the tile's weights.
__global__ __launch_bounds__(256) void dose_tile_sum_kernel(const float* __restrict__ x, long n, const unsigned* __restrict__ maxw,
                                                            u64* __restrict__ sums) {
    __shared__ u64 sh[4];
    const long b = blockIdx.y, begin = (long)blockIdx.x * kTile, end = begin + kTile < n ? begin + kTile : n;
    const float* xb = x + b * n;
    const double m = (double)__uint_as_float(maxw[b]);
    u64 s = 0;
    for (long i = begin + threadIdx.x; i < end; i += 256) s += weight(xb[i], m);
    u64 total;
    emd::block_inclusive_scan(s, sh, &total);
    if (threadIdx.x == 0) sums[b * gridDim.x + blockIdx.x] = total;
}

// grid (B): sums[b][tile] -> the sum of the tiles before it, 256 tiles a step.  Sets EMD_DOSE_EMPTY.
__global__ __launch_bounds__(256) void dose_scan_sums_kernel(u64* __restrict__ sums, int tiles, const unsigned* __restrict__ maxw,
                                                             int* __restrict__ status) {
    __shared__ u64 sh[2][4];
    const long b = blockIdx.x;
    u64* s = sums + b * tiles;
    u64 carry = 0;
    int flip = 0;
    for (int t0 = 0; t0 < tiles; t0 += 256, flip ^= 1) {
        const int i = t0 + (int)threadIdx.x;
        const u64 v = i < tiles ? s[i] : 0ull;
        u64 total;
        const u64 incl = emd::block_inclusive_scan(v, sh[flip], &total);
        if (i < tiles) s[i] = carry + (incl - v);
        carry += total;
    }
    if (threadIdx.x == 0 && status && maxw[b] == 0u) status[b] |= EMD_DOSE_EMPTY;   // this image's only writer in this launch
}

// grid (tiles, B).  A step is 512 consecutive pixels, two per thread: loads of 8 and stores of 16 bytes per lane, both contiguous
// over the wave.  pair_ok: every image's CDF starts 16-byte aligned (n even, or one image).
__global__ __launch_bounds__(256) void dose_tile_scan_kernel(const float* __restrict__ x, long n, const unsigned* __restrict__ maxw,
                                                             const u64* __restrict__ offsets, long long* __restrict__ cdf, int pair_ok) {
    __shared__ u64 sh[2][4];
    const long b = blockIdx.y, begin = (long)blockIdx.x * kTile;
    const float* xb = x + b * n;
    long long* cb = cdf + b * n;
    const double m = (double)__uint_as_float(maxw[b]);
    u64 carry = offsets[b * gridDim.x + blockIdx.x];
#pragma unroll
    for (int it = 0; it < kTile / kStep; ++it) {
        const long i0 = begin + it * kStep + 2 * (long)threadIdx.x;   // uniform trip count: the barriers inside are reached by all
        const u64 q0 = i0 < n ? weight(xb[i0], m) : 0ull;
        const u64 q1 = i0 + 1 < n ? weight(xb[i0 + 1], m) : 0ull;
        u64 total;
        const u64 incl = carry + emd::block_inclusive_scan(q0 + q1, sh[it & 1], &total);
        carry += total;
        if (i0 + 1 < n && pair_ok) {
            longlong2 v;
            v.x = (long long)(incl - q1);
            v.y = (long long)incl;
            *reinterpret_cast<longlong2*>(cb + i0) = v;
        } else {
            if (i0 < n) cb[i0] = (long long)(incl - q1);
            if (i0 + 1 < n) cb[i0 + 1] = (long long)incl;
        }
    }
}

struct DoseBounds {
    long long b[kMaxLevels + 1];
};

// grid (workgroups, B), grid-stride over the Philox calls j0 .. j0 + calls - 1 of an image; call j makes the draws 2 j and 2 j + 1.
// E[k] = the CDF at the last pixel of segment k (seg pixels, a multiple of 16; K <= kCoarse segments cover the image: the tile ends
// where the image has kCoarse tiles, a finer table where it has fewer, a coarser one where it has more).  A target t < T: the first
// k with E[k] > t in LDS, then the first pixel of that segment with C > t in global memory, log2(seg) steps: 11 at 2048^2, 7 at
// 512^2, and as many more as an image beyond kCoarse tiles has tiles per entry.  That pixel has C[i-1] <= t < C[i]: as many pixels
// have C <= t as lie before it, and its weight is not zero.
__global__ __launch_bounds__(256) void dose_draw_kernel(const long long* __restrict__ cdf, long n, long seg, int K, unsigned k0, unsigned k1,
                                                        unsigned image0, u64 j0, long calls, DoseBounds bnd, int L,
                                                        int* __restrict__ planes) {
    __shared__ u64 E[kCoarse];
    const long b = blockIdx.y;
    const long long* c = cdf + b * n;
    for (int k = threadIdx.x; k < K; k += 256) {
        const long e = (k + 1) * seg < n ? (k + 1) * seg : n;
        E[k] = (u64)c[e - 1];
    }
    __syncthreads();
    const u64 T = E[K - 1];
    if (T == 0) return;   // an empty image: no electron lands
    int* pb = planes + b * L * n;
    const long long first = bnd.b[0], last = bnd.b[L];
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < calls; idx += (long)gridDim.x * 256) {
        const u64 j = j0 + (u64)idx;
        const emd::U4 r = emd::philox4x32_10(emd::U4{(unsigned)j, (unsigned)(j >> 32), image0 + (unsigned)b, emd::kPhiloxTagDose}, k0, k1);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const long long d = (long long)(2 * j + h);
            if (d < first || d >= last) continue;
            const u64 r64 = h ? ((u64)r.z << 32 | r.w) : ((u64)r.x << 32 | r.y);
            const u64 t = __umul64hi(r64, T);
            int a = 0, z = K - 1;
            while (a < z) {
                const int mid = (a + z) >> 1;
                if (E[mid] > t) z = mid;
                else a = mid + 1;
            }
            long lo = a * seg, hi = (lo + seg < n ? lo + seg : n) - 1;   // C[hi] = E[a] > t
            while (lo < hi) {
                const long mid = (lo + hi) >> 1;
                if ((u64)c[mid] > t) hi = mid;
                else lo = mid + 1;
            }
            int k = 0;   // the level: the last k with bounds[k] <= d (a uniform loop: the bounds stay in scalar registers)
            for (int q = 1; q < L; ++q) k += d >= bnd.b[q];
            atomicAdd(&pb[k * n + lo], 1);   // the result is not used: a no-return device-scope add
        }
    }
}

// grid (chunks, B).  Plane k becomes the sum of the planes 0 .. k; minmax[b][k] = {min, max}, set to all ones before: the min by an
// unsigned atomicMin, the max by a signed atomicMax (-1 to start with).  Counts are not negative.
__global__ __launch_bounds__(256) void dose_cumulate_kernel(int* __restrict__ planes, long n, int L, int* __restrict__ minmax) {
    __shared__ unsigned shmin[4];
    __shared__ int shmax[4];
    constexpr int kPer = kChunk / 256;
    const long b = blockIdx.y, begin = (long)blockIdx.x * kChunk;
    int* pb = planes + b * L * n;
    int acc[kPer];
#pragma unroll
    for (int q = 0; q < kPer; ++q) acc[q] = 0;
    for (int k = 0; k < L; ++k) {
        unsigned mn = 0xffffffffu;
        int mx = -1;
#pragma unroll
        for (int q = 0; q < kPer; ++q) {
            const long i = begin + q * 256 + threadIdx.x;
            if (i < n) {
                acc[q] += pb[k * n + i];
                if (k) pb[k * n + i] = acc[q];
                mn = min(mn, (unsigned)acc[q]);
                mx = max(mx, acc[q]);
            }
        }
#pragma unroll
        for (int o = 32; o; o >>= 1) {
            mn = min(mn, (unsigned)__shfl_xor((int)mn, o));
            mx = max(mx, __shfl_xor(mx, o));
        }
        __syncthreads();   // the arrays may still be read for the level before
        if ((threadIdx.x & 63) == 0) {
            shmin[threadIdx.x >> 6] = mn;
            shmax[threadIdx.x >> 6] = mx;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            int* mm = minmax + (b * L + k) * 2;
            atomicMin(reinterpret_cast<unsigned*>(mm), min(min(shmin[0], shmin[1]), min(shmin[2], shmin[3])));
            atomicMax(mm + 1, max(max(shmax[0], shmax[1]), max(shmax[2], shmax[3])));
        }
    }
}

// grid (chunks, L, B).  record_lq: 65535 (c - min) / (max - min) in double, truncated; or (c - min) / (max - min) rounded once to
// float32.  A flat plane (the reference divides by zero) is all 0.
template <int MODE>
__global__ __launch_bounds__(256) void dose_rescale_kernel(const int* __restrict__ planes, const int* __restrict__ minmax, long n,
                                                           void* __restrict__ out) {
    const long plane = (long)blockIdx.z * gridDim.y + blockIdx.y;
    const int mn = minmax[plane * 2], range = minmax[plane * 2 + 1] - mn;
    const long i = (long)blockIdx.x * 1024 + threadIdx.x;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const long p = i + q * 256;
        if (p >= n) continue;
        const double num = (double)(planes[plane * n + p] - mn);
        if (MODE == EMD_DOSE_UINT16)
            static_cast<int*>(out)[plane * n + p] = range ? (int)((65535.0 * num) / (double)range) : 0;
        else
            static_cast<float*>(out)[plane * n + p] = range ? (float)(num / (double)range) : 0.f;
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------
bool shape_ok(const char* who, int B, int H, int W) {
    if (B >= 0 && B <= 65535 && H >= 2 && W >= 2 && H <= kMaxExtent && W <= kMaxExtent && (long)H * W <= kMaxPixels) return true;
    emd::set_error("%s: bad shape (batch 0..65535, 2 <= H, W <= %d, H W <= 2^30; got %d x %d x %d)", who, kMaxExtent, B, H, W);
    return false;
}

bool levels_ok(const char* who, int L) {
    if (L >= 1 && L <= kMaxLevels) return true;
    emd::set_error("%s: 1 <= L <= %d levels (got %d)", who, kMaxLevels, L);
    return false;
}

int tiles_of_image(int H, int W) { return (int)(((long)H * W + kTile - 1) / kTile); }

// p0[0 .. n0) = p1[0 .. n1) = v (p1 may be NULL).  The words the atomics start from are set by this launch, not by a memset node: a
// captured hipMemsetAsync of a few bytes wrote other bytes than its value from the second replay of the graph on (seen as 0x50
// in every byte of the status words and of the maxima).
__global__ __launch_bounds__(256) void dose_fill_kernel(unsigned* __restrict__ p0, long n0, unsigned* __restrict__ p1, long n1, unsigned v) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n0) p0[i] = v;
    if (p1 && i < n1) p1[i] = v;
}

void launch_fill(unsigned* p0, long n0, unsigned* p1, long n1, unsigned v, hipStream_t st) {
    const long n = n0 > n1 ? n0 : n1;
    hipLaunchKernelGGL(dose_fill_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, p0, n0, p1, p1 ? n1 : 0, v);
}

}  // namespace

extern "C" size_t emd_dose_workspace_bytes(int B, int H, int W) {
    if (B < 1 || B > 65535 || H < 2 || W < 2 || H > kMaxExtent || W > kMaxExtent || (long)H * W > kMaxPixels) return 0;
    return emd::round256((size_t)B * sizeof(unsigned)) + emd::round256((size_t)B * tiles_of_image(H, W) * sizeof(u64));
}

extern "C" int emd_dose_cdf_i64(const float* x, int B, int H, int W, int64_t* cdf, int* status, void* workspace, size_t workspace_bytes,
                                emd_stream_t stream) {
    if (!shape_ok("emd_dose_cdf_i64", B, H, W)) return EMD_E_INVALID;
    if (B == 0) return EMD_OK;
    const long n = (long)H * W;
    const int tiles = tiles_of_image(H, W);
    const emd::Range r[] = {{workspace, emd_dose_workspace_bytes(B, H, W), 16, false, false},
                            {x, (size_t)B * n * sizeof(float), 4, false, true},
                            {cdf, (size_t)B * n * sizeof(int64_t), 8, false, false},
                            {status, (size_t)B * sizeof(int), 4, true, false}};
    const int rc = emd::check_ranges("emd_dose_cdf_i64", r, 4, "the workspace must be 16-byte aligned, cdf 8-byte, x and status 4-byte",
                               &workspace_bytes);
    if (rc != EMD_OK) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    unsigned* maxw = static_cast<unsigned*>(workspace);
    u64* sums = reinterpret_cast<u64*>(static_cast<char*>(workspace) + emd::round256((size_t)B * sizeof(unsigned)));
    launch_fill(maxw, B, reinterpret_cast<unsigned*>(status), B, 0u, st);
    const dim3 grid((unsigned)tiles, (unsigned)B);
    const int pair_ok = ((reinterpret_cast<uintptr_t>(cdf) & 15u) == 0 && (B == 1 || n % 2 == 0)) ? 1 : 0;
    hipLaunchKernelGGL(dose_max_kernel, grid, dim3(256), 0, st, x, n, maxw, status);
    hipLaunchKernelGGL(dose_tile_sum_kernel, grid, dim3(256), 0, st, x, n, maxw, sums);
    hipLaunchKernelGGL(dose_scan_sums_kernel, dim3((unsigned)B), dim3(256), 0, st, sums, tiles, maxw, status);
    hipLaunchKernelGGL(dose_tile_scan_kernel, grid, dim3(256), 0, st, x, n, maxw, sums, reinterpret_cast<long long*>(cdf), pair_ok);
    return emd::check_launch("emd_dose_cdf_i64");
}

extern "C" int emd_dose_draw_i32(const int64_t* cdf, int B, int H, int W, unsigned long long seed, unsigned long long first_image,
                                 const int64_t* bounds_host, int L, int* planes, emd_stream_t stream) {
    if (!shape_ok("emd_dose_draw_i32", B, H, W) || !levels_ok("emd_dose_draw_i32", L)) return EMD_E_INVALID;
    EMD_REQUIRE(bounds_host, EMD_E_INVALID, "emd_dose_draw_i32: null pointer (bounds)");
    DoseBounds bnd;
    for (int k = 0; k <= L; ++k) bnd.b[k] = bounds_host[k];
    for (int k = L + 1; k <= kMaxLevels; ++k) bnd.b[k] = bounds_host[L];
    EMD_REQUIRE(bnd.b[0] >= 0, EMD_E_INVALID, "emd_dose_draw_i32: bounds[0] must be >= 0");
    for (int k = 0; k < L; ++k) EMD_REQUIRE(bnd.b[k] <= bnd.b[k + 1], EMD_E_INVALID, "emd_dose_draw_i32: bounds must not descend");
    EMD_REQUIRE(bnd.b[L] - bnd.b[0] < (1LL << 31), EMD_E_INVALID, "emd_dose_draw_i32: bounds[L] - bounds[0] must be < 2^31 (counts are int32)");
    EMD_REQUIRE(first_image + (unsigned long long)B <= (1ULL << 32), EMD_E_INVALID,
                "emd_dose_draw_i32: first_image + B must be <= 2^32 (one counter word)");
    if (B == 0) return EMD_OK;
    const long n = (long)H * W;
    const emd::Range r[] = {{cdf, (size_t)B * n * sizeof(int64_t), 8, false, true}, {planes, (size_t)B * L * n * sizeof(int), 4, false, false}};
    const int rc = emd::check_ranges("emd_dose_draw_i32", r, 2, "cdf must be 8-byte aligned, planes 4-byte");
    if (rc != EMD_OK) return rc;
    if (bnd.b[L] == bnd.b[0]) return EMD_OK;
    // the table's spacing: the image over kCoarse entries, in whole groups of 16 pixels (one 128-byte line of the CDF); a tile
    // where the image has kCoarse tiles, less where it has fewer, more where it has more
    const long seg = ((n + kCoarse - 1) / kCoarse + 15) / 16 * 16;
    const int K = (int)((n + seg - 1) / seg);
    const u64 j0 = (u64)bnd.b[0] >> 1;
    const long calls = (long)((((u64)bnd.b[L] + 1) >> 1) - j0);
    // at least 16 calls a thread where there are that many, so that staging the table is a small part of a workgroup's work
    long wgs = (calls + 4095) / 4096, cap = 4096 / B > 1 ? 4096 / B : 1;
    wgs = wgs < 1 ? 1 : (wgs > cap ? cap : wgs);
    hipLaunchKernelGGL(dose_draw_kernel, dim3((unsigned)wgs, (unsigned)B), dim3(256), 0, static_cast<hipStream_t>(stream),
                       reinterpret_cast<const long long*>(cdf), n, seg, K, (unsigned)seed, (unsigned)(seed >> 32), (unsigned)first_image, j0,
                       calls, bnd, L, planes);
    return emd::check_launch("dose_draw_kernel");
}

extern "C" int emd_dose_cumulate_i32(int* planes, int B, int L, int H, int W, int* minmax, emd_stream_t stream) {
    if (!shape_ok("emd_dose_cumulate_i32", B, H, W) || !levels_ok("emd_dose_cumulate_i32", L)) return EMD_E_INVALID;
    if (B == 0) return EMD_OK;
    const long n = (long)H * W;
    const emd::Range r[] = {{planes, (size_t)B * L * n * sizeof(int), 4, false, false}, {minmax, (size_t)B * L * 2 * sizeof(int), 4, false, false}};
    const int rc = emd::check_ranges("emd_dose_cumulate_i32", r, 2, "planes and minmax must be 4-byte aligned");
    if (rc != EMD_OK) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    launch_fill(reinterpret_cast<unsigned*>(minmax), (long)B * L * 2, nullptr, 0, 0xffffffffu, st);
    hipLaunchKernelGGL(dose_cumulate_kernel, dim3((unsigned)((n + kChunk - 1) / kChunk), (unsigned)B), dim3(256), 0, st, planes, n, L, minmax);
    return emd::check_launch("dose_cumulate_kernel");
}

extern "C" int emd_dose_rescale(const int* planes, const int* minmax, int B, int L, int H, int W, int mode, void* out, emd_stream_t stream) {
    if (!shape_ok("emd_dose_rescale", B, H, W) || !levels_ok("emd_dose_rescale", L)) return EMD_E_INVALID;
    EMD_REQUIRE(mode == EMD_DOSE_UNIT || mode == EMD_DOSE_UINT16, EMD_E_INVALID, "emd_dose_rescale: mode must be EMD_DOSE_UNIT or EMD_DOSE_UINT16");
    if (B == 0) return EMD_OK;
    const long n = (long)H * W;
    const emd::Range r[] = {{planes, (size_t)B * L * n * sizeof(int), 4, false, true},
                            {minmax, (size_t)B * L * 2 * sizeof(int), 4, false, true},
                            {out, (size_t)B * L * n * 4, 4, false, false}};
    const int rc = emd::check_ranges("emd_dose_rescale", r, 3, "every array must be 4-byte aligned");
    if (rc != EMD_OK) return rc;
    const dim3 grid((unsigned)((n + 1023) / 1024), (unsigned)L, (unsigned)B);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (mode == EMD_DOSE_UINT16)
        hipLaunchKernelGGL(dose_rescale_kernel<EMD_DOSE_UINT16>, grid, dim3(256), 0, st, planes, minmax, n, out);
    else
        hipLaunchKernelGGL(dose_rescale_kernel<EMD_DOSE_UNIT>, grid, dim3(256), 0, st, planes, minmax, n, out);
    return emd::check_launch("dose_rescale_kernel");
}
