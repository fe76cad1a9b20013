// Harvesting raw micrographs on the device: the reference's MATLAB harvester, DM3stoTIFs-batch/img_params.m,
// img_params_lq.m and estimate_noise.m -- crop to the smaller dimension, box-resize to 2048 x 2048, a table of statistics, rescale
// to [0, 1] -- restated from the formulas in include/emdenoise.h.
//
//   emd_box_resize_f32    one launch: a workgroup owns 16 x 64 outputs; the input rows and columns their runs cover pass through
//                         LDS in coalesced segments of up to 16 rows x 256 columns, and every lane adds its own run from LDS, in
//                         double, rows then columns ascending
//   emd_image_stats_f64   tiles with a zero halo in LDS: min, max, the counts, sum x, sum x^2, sum sqrt, the Laplacian sum and the
//                         selection's first histogram from ONE read; a second read for the centred moments, which also feeds the
//                         selection's second histogram; two more selection reads; small per-image launches in between
//   emd_scale01_f32       element-wise, min and max read from the statistics on the device
//
// Images are float32; every image on its own; grid (tiles or chunks, B).  Histograms are integer atomics (order-free); there is
// no floating-point atomic: partial sums are doubles, stored per workgroup and added in a fixed order.
#include <cfloat>
#include <cmath>

#include "radix_select.hpp"
#include "stencil_rows.hpp"
#include "wave_reduce.hpp"

#pragma clang fp contract(off)   // every operation rounds on its own, as in the host restatement

namespace {

constexpr int kMaxExtent = 32768;   // H, W, d
constexpr int kMaxOut = 8192;       // S

// ---- box resize ------------------------------------------------------------------------------------------------------------
constexpr int kRT = 16;    // output rows of a tile (a wave: 4)
constexpr int kRW = 4;
constexpr int kRC = 64;    // output columns of a tile = lanes of a wave
constexpr int kSegR = 16;  // input rows of an LDS segment
constexpr int kSegC = 256; // input columns of an LDS segment

// The run (first, count) of output sample o, clamped into 0..d-1 whatever the table holds: no address leaves the crop.
__device__ __forceinline__ void run_of(const int* __restrict__ tab, int o, int d, int& first, int& end) {
    int f = tab[2 * o], n = tab[2 * o + 1];
    f = f < 0 ? 0 : (f > d - 1 ? d - 1 : f);
    n = n < 1 ? 1 : (n > d - f ? d - f : n);
    first = f;
    end = f + n;
}

// grid (tiles, B), 256 threads.  x: image b at x + b * xstride, rows row_stride apart, the top-left d x d pixels are read.
__global__ __launch_bounds__(256) void box_resize_kernel(const float* __restrict__ x, long xstride, int row_stride, int d,
                                                         float* __restrict__ y, int S, const int* __restrict__ tab, int tiles_x) {
    __shared__ float seg[kSegR * kSegC];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r0 = (blockIdx.x / tiles_x) * kRT, c0 = (blockIdx.x % tiles_x) * kRC;
    const float* xb = x + (long)blockIdx.y * xstride;
    // the rows and columns of the input the tile's runs cover (the runs ascend with the output index)
    const int rl = min(r0 + kRT, S) - 1, cl = min(c0 + kRC, S) - 1;
    int rb, re, cb, ce, t;
    run_of(tab, r0, d, rb, t);
    run_of(tab, rl, d, t, re);
    run_of(tab, c0, d, cb, t);
    run_of(tab, cl, d, t, ce);
    // this thread's outputs: column c0 + lane, rows r0 + wave * kRW + q
    const int oc = c0 + lane;
    int cf = 0, cend = 0, rf[kRW], rend[kRW];   // first and end of the runs
    if (oc < S) run_of(tab, oc, d, cf, cend);
    double acc[kRW];
#pragma unroll
    for (int q = 0; q < kRW; ++q) {
        const int orow = r0 + wave * kRW + q;
        rf[q] = rend[q] = 0;
        if (orow < S) run_of(tab, orow, d, rf[q], rend[q]);
        acc[q] = 0.0;
    }
    for (int sc = cb; sc < ce; sc += kSegC) {
        const int wc = min(kSegC, ce - sc);
        const int j0 = max(cf, sc) - sc, j1 = min(cend, sc + wc) - sc;   // this lane's columns inside the segment
        for (int sr = rb; sr < re; sr += kSegR) {
            const int hr = min(kSegR, re - sr);
            __syncthreads();   // the previous segment may still be read
            for (int r = wave; r < hr; r += 4) {
                const float* row = xb + (long)(sr + r) * row_stride + sc;
                for (int c = lane; c < wc; c += 64) seg[r * kSegC + c] = row[c];
            }
            __syncthreads();
#pragma unroll
            for (int q = 0; q < kRW; ++q) {
                const int i0 = max(rf[q], sr) - sr, i1 = min(rend[q], sr + hr) - sr;
                for (int i = i0; i < i1; ++i) {
                    for (int j = j0; j < j1; ++j) acc[q] += (double)seg[i * kSegC + j];
                }
            }
        }
    }
    if (oc < S) {
        float* yb = y + (long)blockIdx.y * S * S;
#pragma unroll
        for (int q = 0; q < kRW; ++q) {
            const int orow = r0 + wave * kRW + q;
            if (orow < S) yb[(long)orow * S + oc] = (float)(acc[q] / ((double)(rend[q] - rf[q]) * (double)(cend - cf)));
        }
    }
}

// ---- statistics ------------------------------------------------------------------------------------------------------------
constexpr int kTW = 64;          // tile columns = lanes of a wave
constexpr int kTH = 32;          // tile rows (a wave: 8)
constexpr int kTR = kTH / 4;
constexpr int kLW = kTW + 2;     // the tile with its halo of 1
constexpr int kLH = kTH + 2;
constexpr int kChunk = 4096;     // pixels per workgroup of the 1-D passes
constexpr int kPart1 = 8;        // per tile: sum x, sum x^2, sum sqrt, sum |laplacian|, min, max, nonzero, negative
constexpr int kPart2 = 6;        // per chunk: sum (x - mean)^k, k = 2, 3, 4; the same of sqrt(max(x, 0))
constexpr int kAcc = 16;         // per image: the eight of kPart1 reduced, then mean, sqrt_mean
struct StatsBuffers {
    double* part1;     // [B][kPart1][tiles]
    double* part2;     // [B][kPart2][chunks]
    double* acc;       // [B][kAcc]
    unsigned* hist;    // the selection's (radix_select.hpp): the key is signed_key, every pixel is counted
    unsigned* state;
};

// Pass 0 of everything: grid (tiles of the (H + 2) x (W + 2) full-convolution grid, B).  Position (er, ec) of that grid is centred on
// pixel (er - 1, ec - 1); a pixel is counted by the workgroup whose tile holds its centre, so every pixel is counted once.
__global__ __launch_bounds__(256) void stats_tile_kernel(const float* __restrict__ x, int H, int W, int tiles_x, StatsBuffers sb) {
    __shared__ float xs[kLH * kLW];
    __shared__ unsigned h[1][256];
    __shared__ double sh[4];
    __shared__ float shf[2][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tile = blockIdx.x, tiles = gridDim.x;
    const int er0 = (tile / tiles_x) * kTH, ec0 = (tile % tiles_x) * kTW;
    const long b = blockIdx.y;
    const float* xb = x + b * (long)H * W;
    h[0][tid] = 0;
    // xs[r][c] = pixel (er0 - 2 + r, ec0 - 2 + c), 0 outside the image
    for (int i = tid; i < kLH * kLW; i += 256) {
        const int r = i / kLW, c = i - r * kLW;
        const int pr = er0 - 2 + r, pc = ec0 - 2 + c;
        xs[i] = (pr >= 0 && pr < H && pc >= 0 && pc < W) ? xb[(long)pr * W + pc] : 0.f;
    }
    __syncthreads();
    double sx = 0.0, sxx = 0.0, ssq = 0.0, slap = 0.0;
    float mn = INFINITY, mx = -INFINITY;
    unsigned nz = 0, neg = 0;
    const int ec = ec0 + lane;
#pragma unroll
    for (int q = 0; q < kTR; ++q) {
        const int lr = wave * kTR + q, er = er0 + lr;
        if (er < H + 2 && ec < W + 2) {
            const float* p = xs + (lr + 1) * kLW + lane + 1;   // the centre
            const double c = (double)p[0];
            const double edges = ((double)p[-kLW] + (double)p[kLW]) + ((double)p[-1] + (double)p[1]);
            const double corners = ((double)p[-kLW - 1] + (double)p[-kLW + 1]) + ((double)p[kLW - 1] + (double)p[kLW + 1]);
            slap += fabs((4.0 * c - 2.0 * edges) + corners);
            if (er >= 1 && er <= H && ec >= 1 && ec <= W) {
                const float v = p[0];
                sx += c;
                sxx += c * c;
                ssq += sqrt(fmax(c, 0.0));
                mn = fminf(mn, v);
                mx = fmaxf(mx, v);
                nz += v != 0.f;
                neg += v < 0.f;
                select_count_first(h, signed_key(v));
            }
        }
    }
    double* out = sb.part1 + b * kPart1 * tiles + tile;
    double r;
    r = block_sum_thread0(sx, sh);
    if (tid == 0) out[0] = r;
    r = block_sum_thread0(sxx, sh);
    if (tid == 0) out[(long)tiles] = r;
    r = block_sum_thread0(ssq, sh);
    if (tid == 0) out[2L * tiles] = r;
    r = block_sum_thread0(slap, sh);
    if (tid == 0) out[3L * tiles] = r;
    r = block_sum_thread0((double)nz, sh);   // integers far below 2^53: exact
    if (tid == 0) out[6L * tiles] = r;
    r = block_sum_thread0((double)neg, sh);
    if (tid == 0) out[7L * tiles] = r;
    mn = emd::wave_min(mn);
    mx = emd::wave_max(mx);
    if (lane == 0) {
        shf[0][wave] = mn;
        shf[1][wave] = mx;
    }
    __syncthreads();   // also: every LDS histogram add has been made
    if (tid == 0) {
        out[4L * tiles] = (double)fminf(fminf(shf[0][0], shf[0][1]), fminf(shf[0][2], shf[0][3]));
        out[5L * tiles] = (double)fmaxf(fmaxf(shf[1][0], shf[1][1]), fmaxf(shf[1][2], shf[1][3]));
    }
    select_flush<1>(h, sb.hist + select_hist_at(b, 0));
}

// Minimum (MAX = false) or maximum of p[0 .. n - 1] by the workgroup; every thread returns it.
template <bool MAX>
__device__ double block_extreme(const double* __restrict__ p, int n, double* sh) {
    const int tid = threadIdx.x;
    double s = MAX ? -INFINITY : INFINITY;
    for (int i = tid; i < n; i += 256) s = MAX ? fmax(s, p[i]) : fmin(s, p[i]);
    __syncthreads();   // sh may still be read from the previous call
    sh[tid] = s;
    __syncthreads();
    for (int off = 128; off >= 1; off >>= 1) {
        if (tid < off) sh[tid] = MAX ? fmax(sh[tid], sh[tid + off]) : fmin(sh[tid], sh[tid + off]);
        __syncthreads();
    }
    return sh[0];
}

// grid (B): the tiles' partials -> acc, the means, and the selection's state for pass 1
__global__ __launch_bounds__(256) void stats_mid_kernel(StatsBuffers sb, int tiles, double count) {
    __shared__ double sh[256];
    __shared__ unsigned sc[2][256];
    __shared__ unsigned next[kStateWords];
    const long b = blockIdx.x;
    const double* p = sb.part1 + b * kPart1 * tiles;
    double v[kPart1];
    for (int k = 0; k < kPart1; ++k)
        v[k] = k == 4 ? block_extreme<false>(p + (long)k * tiles, tiles, sh)
                      : (k == 5 ? block_extreme<true>(p + (long)k * tiles, tiles, sh) : block_sum_fixed(p + (long)k * tiles, tiles, 1, sh));
    if (threadIdx.x == 0) {
        double* a = sb.acc + b * kAcc;
        for (int k = 0; k < kPart1; ++k) a[k] = v[k];
        a[8] = v[0] / count;
        a[9] = v[2] / count;
    }
    select_resolve(sb.hist + select_hist_at(b, 0), nullptr, 0, sc, next);
    if (threadIdx.x < kStateWords) sb.state[select_state_at(b, 1) + threadIdx.x] = next[threadIdx.x];
}

// grid (B): pass q's histograms -> the state of pass q + 1 (q = 1, 2)
__global__ __launch_bounds__(256) void stats_resolve_kernel(StatsBuffers sb, int q) {
    __shared__ unsigned sc[2][256];
    __shared__ unsigned next[kStateWords];
    const long b = blockIdx.x;
    select_resolve(sb.hist + select_hist_at(b, q), sb.state + select_state_at(b, q), q, sc, next);
    if (threadIdx.x < kStateWords) sb.state[select_state_at(b, q + 1) + threadIdx.x] = next[threadIdx.x];
}

// grid (chunks, B): selection pass `pass` (1..3) over the image as a row of n pixels; MOMENTS: the centred sums as well
template <bool MOMENTS>
__global__ __launch_bounds__(256) void stats_chunk_kernel(const float* __restrict__ x, long n, StatsBuffers sb, int pass) {
    __shared__ unsigned h[2][256];
    __shared__ double sh[4];
    const int tid = threadIdx.x;
    const long b = blockIdx.y;
    const unsigned* st = sb.state + select_state_at(b, pass);
    const unsigned prefix0 = st[0], prefix1 = st[1];
    h[0][tid] = 0;
    h[1][tid] = 0;
    __syncthreads();
    double mean = 0.0, smean = 0.0;
    if (MOMENTS) {
        mean = sb.acc[b * kAcc + 8];
        smean = sb.acc[b * kAcc + 9];
    }
    double m2 = 0.0, m3 = 0.0, m4 = 0.0, s2 = 0.0, s3 = 0.0, s4 = 0.0;
    const long begin = (long)blockIdx.x * kChunk, end = begin + kChunk < n ? begin + kChunk : n;
    const float* xb = x + b * n;
    for (long i = begin + tid; i < end; i += 256) {
        const float v = xb[i];
        select_count(h, signed_key(v), pass, prefix0, prefix1);
        if (MOMENTS) {
            const double dv = (double)v - mean, d2 = dv * dv;
            m2 += d2;
            m3 += d2 * dv;
            m4 += d2 * d2;
            const double e = sqrt(fmax((double)v, 0.0)) - smean, e2 = e * e;
            s2 += e2;
            s3 += e2 * e;
            s4 += e2 * e2;
        }
    }
    __syncthreads();
    select_flush<2>(h, sb.hist + select_hist_at(b, pass));
    if (MOMENTS) {
        const long chunks = gridDim.x;
        double* out = sb.part2 + b * kPart2 * chunks + blockIdx.x;
        const double vals[kPart2] = {m2, m3, m4, s2, s3, s4};
#pragma unroll
        for (int k = 0; k < kPart2; ++k) {
            const double r = block_sum_thread0(vals[k], sh);
            if (tid == 0) out[k * chunks] = r;
        }
    }
}

// grid (B): the seventeen
__global__ __launch_bounds__(256) void stats_final_kernel(StatsBuffers sb, int chunks, int H, int W, double* __restrict__ stats) {
    __shared__ double sh[256];
    __shared__ unsigned sc[2][256];
    __shared__ unsigned keys[kStateWords];
    const long b = blockIdx.x;
    select_resolve(sb.hist + select_hist_at(b, 3), sb.state + select_state_at(b, 3), 3, sc, keys);
    double c[kPart2];
    for (int k = 0; k < kPart2; ++k) c[k] = block_sum_fixed(sb.part2 + (b * kPart2 + k) * chunks, chunks, 1, sh);
    if (threadIdx.x != 0) return;
    const double* a = sb.acc + b * kAcc;
    const double N = (double)H * (double)W;
    const double mean = a[8], smean = a[9];
    double* s = stats + b * EMD_NSTATS;
    s[0] = a[4];
    s[1] = a[5];
    s[2] = a[6];
    s[3] = a[7];
    s[4] = mean;
    const double sd = sqrt(c[0] / (N - 1.0)), m2 = c[0] / N;
    s[5] = sd;
    s[6] = (c[1] / N) / (m2 * sqrt(m2));
    s[7] = (c[2] / N) / (m2 * m2);
    s[8] = ((double)signed_key_value(keys[0]) + (double)signed_key_value(keys[1])) * 0.5;
    s[9] = sqrt(a[1] / N);
    s[10] = 100.0 * sd / mean;
    s[11] = a[3] * sqrt(0.5 * M_PI) / (6.0 * (double)(W - 2) * (double)(H - 2));
    const double q2 = c[3] / N;
    s[12] = smean;
    s[13] = sqrt(c[3] / (N - 1.0));
    s[14] = (c[4] / N) / (q2 * sqrt(q2));
    s[15] = (c[5] / N) / (q2 * q2);
    s[16] = smean / mean;
}

// ---- scale to [0, 1]: grid (chunks, B) ----------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void scale01_kernel(const float* __restrict__ x, float* __restrict__ y, long n,
                                                      const double* __restrict__ stats) {
    const long b = blockIdx.y;
    const float lo = (float)stats[b * EMD_NSTATS], hi = (float)stats[b * EMD_NSTATS + 1];
    const float d = hi - lo;
    const bool flat = fabsf(d) < 1e-6f;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const long k = b * n + i;
        y[k] = flat ? 0.5f : (x[k] - lo) / d;
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------------

struct StatsLayout {
    int tiles_x, tiles, chunks;
    size_t part1, part2, acc, hist, state, bytes;
};

bool stats_shape_ok(int B, int H, int W) { return B >= 0 && B <= 65535 && H >= 3 && W >= 3 && H <= kMaxExtent && W <= kMaxExtent; }

StatsLayout stats_layout(int B, int H, int W) {
    StatsLayout l{};
    l.tiles_x = (W + 2 + kTW - 1) / kTW;
    l.tiles = l.tiles_x * ((H + 2 + kTH - 1) / kTH);
    l.chunks = (int)(((long)H * W + kChunk - 1) / kChunk);
    size_t bytes = 0;
    l.part1 = bytes;
    bytes += emd::round256((size_t)B * kPart1 * l.tiles * sizeof(double));
    l.part2 = bytes;
    bytes += emd::round256((size_t)B * kPart2 * l.chunks * sizeof(double));
    l.acc = bytes;
    bytes += emd::round256((size_t)B * kAcc * sizeof(double));
    l.hist = bytes;
    bytes += select_hist_bytes(B);
    l.state = bytes;
    bytes += select_state_bytes(B);
    l.bytes = bytes;
    return l;
}

}  // namespace

extern "C" int emd_box_resize_f32(const float* x, long image_stride, int row_stride, int B, int d, float* y, int S, const int* tab_dev,
                                  emd_stream_t stream) {
    EMD_REQUIRE(B >= 0 && B <= 65535, EMD_E_INVALID, "emd_box_resize_f32: the batch must be 0..65535");
    EMD_REQUIRE(d >= 1 && d <= kMaxExtent && S >= 1 && S <= kMaxOut, EMD_E_INVALID,
                "emd_box_resize_f32: 1 <= d <= 32768 and 1 <= S <= 8192");
    EMD_REQUIRE(row_stride >= d && image_stride >= 0, EMD_E_INVALID, "emd_box_resize_f32: row_stride must be >= d, image_stride >= 0");
    if (B == 0) return EMD_OK;
    EMD_REQUIRE(x && y && tab_dev, EMD_E_INVALID, "emd_box_resize_f32: null pointer");
    const size_t nx = ((size_t)(B - 1) * (size_t)image_stride + (size_t)(d - 1) * row_stride + d) * sizeof(float);
    EMD_REQUIRE(!emd::overlap(x, nx, y, (size_t)B * S * S * sizeof(float)), EMD_E_INVALID, "emd_box_resize_f32: y may not overlap x");
    const int tiles_x = (S + kRC - 1) / kRC;
    const dim3 grid((unsigned)(tiles_x * ((S + kRT - 1) / kRT)), (unsigned)B);
    hipLaunchKernelGGL(box_resize_kernel, grid, dim3(256), 0, static_cast<hipStream_t>(stream), x, image_stride, row_stride, d, y, S,
                       tab_dev, tiles_x);
    return emd::check_launch("box_resize_kernel");
}

extern "C" size_t emd_image_stats_workspace_bytes(int B, int H, int W) {
    if (B < 1 || !stats_shape_ok(B, H, W)) return 0;
    return stats_layout(B, H, W).bytes;
}

extern "C" int emd_image_stats_f64(const float* x, int B, int H, int W, double* stats, void* workspace, size_t workspace_bytes,
                                   emd_stream_t stream) {
    if (!stats_shape_ok(B, H, W)) {
        emd::set_error("emd_image_stats_f64: bad shape (batch 0..65535, 3 <= H, W <= %d; got %d x %d x %d)", kMaxExtent, B, H, W);
        return EMD_E_INVALID;
    }
    if (B == 0) return EMD_OK;
    EMD_REQUIRE(x && stats && workspace, EMD_E_INVALID, "emd_image_stats_f64: null pointer");
    const StatsLayout l = stats_layout(B, H, W);
    if (workspace_bytes < l.bytes) {
        emd::set_error("emd_image_stats_f64: workspace too small (%zu bytes, needs %zu)", workspace_bytes, l.bytes);
        return EMD_E_INVALID;
    }
    EMD_REQUIRE(emd::aligned16(workspace), EMD_E_ALIGN, "emd_image_stats_f64: workspace must be 16-byte aligned");
    const size_t nx = (size_t)B * H * W * sizeof(float), ns = (size_t)B * EMD_NSTATS * sizeof(double);
    EMD_REQUIRE(!emd::overlap(workspace, l.bytes, x, nx) && !emd::overlap(workspace, l.bytes, stats, ns) && !emd::overlap(stats, ns, x, nx), EMD_E_INVALID,
                "emd_image_stats_f64: x, stats and the workspace may not overlap");
    hipStream_t st = static_cast<hipStream_t>(stream);
    char* ws = static_cast<char*>(workspace);
    StatsBuffers sb;
    sb.part1 = reinterpret_cast<double*>(ws + l.part1);
    sb.part2 = reinterpret_cast<double*>(ws + l.part2);
    sb.acc = reinterpret_cast<double*>(ws + l.acc);
    sb.hist = reinterpret_cast<unsigned*>(ws + l.hist);
    sb.state = reinterpret_cast<unsigned*>(ws + l.state);
    const hipError_t e = hipMemsetAsync(sb.hist, 0, select_hist_bytes(B), st);
    if (e != hipSuccess) {
        emd::set_error("emd_image_stats_f64: hipMemsetAsync: %s", hipGetErrorString(e));
        return EMD_E_LAUNCH;
    }
    const long n = (long)H * W;
    const dim3 per_image((unsigned)B), chunks((unsigned)l.chunks, (unsigned)B);
    hipLaunchKernelGGL(stats_tile_kernel, dim3((unsigned)l.tiles, (unsigned)B), dim3(256), 0, st, x, H, W, l.tiles_x, sb);
    hipLaunchKernelGGL(stats_mid_kernel, per_image, dim3(256), 0, st, sb, l.tiles, (double)n);
    hipLaunchKernelGGL(stats_chunk_kernel<true>, chunks, dim3(256), 0, st, x, n, sb, 1);
    hipLaunchKernelGGL(stats_resolve_kernel, per_image, dim3(256), 0, st, sb, 1);
    hipLaunchKernelGGL(stats_chunk_kernel<false>, chunks, dim3(256), 0, st, x, n, sb, 2);
    hipLaunchKernelGGL(stats_resolve_kernel, per_image, dim3(256), 0, st, sb, 2);
    hipLaunchKernelGGL(stats_chunk_kernel<false>, chunks, dim3(256), 0, st, x, n, sb, 3);
    hipLaunchKernelGGL(stats_final_kernel, per_image, dim3(256), 0, st, sb, l.chunks, H, W, stats);
    return emd::check_launch("emd_image_stats_f64");
}

extern "C" int emd_scale01_f32(const float* x, float* y, int B, long n, const double* stats, emd_stream_t stream) {
    EMD_REQUIRE(B >= 0 && B <= 65535 && n >= 1, EMD_E_INVALID, "emd_scale01_f32: the batch must be 0..65535 and n positive");
    if (B == 0) return EMD_OK;
    EMD_REQUIRE(x && y && stats, EMD_E_INVALID, "emd_scale01_f32: null pointer");
    const size_t nx = (size_t)B * (size_t)n * sizeof(float);
    EMD_REQUIRE(x == y || !emd::overlap(x, nx, y, nx), EMD_E_INVALID, "emd_scale01_f32: y must be x itself or apart from it");
    const long want = (n + 256 * 8 - 1) / (256 * 8);
    hipLaunchKernelGGL(scale01_kernel, dim3((unsigned)(want > 2048 ? 2048 : want), (unsigned)B), dim3(256), 0,
                       static_cast<hipStream_t>(stream), x, y, n, stats);
    return emd::check_launch("scale01_kernel");
}
