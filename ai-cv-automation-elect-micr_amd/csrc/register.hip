// Registration of a focal series before the exit-wave reconstruction (ewrec_class.py:140-177, :190-269), in double:
// phase correlation between image pairs (cv2.phaseCorrelate restated in include/emdenoise.h), the chain of the shifts into one
// cropping centre per image, and the sub-pixel (bilinear) crop around each centre.  Square images of side S, a power of two, 8..4096,
// for the correlation; the 1-D transform is fft_line.hpp's (one line of S complex doubles in LDS), the inverse by conjugation.
//
//   pc_tables_kernel     exp(-2 pi i k / S) and the 1-D Hann table w[i] = 0.5 (1 - cos(2 pi i / (S - 1))), written into the workspace on
//                        every call
//   pc_window_kernel     the public 2-D window sqrt(w[y] w[x]) (and the 1-D table), from the same device function
//   pc_rows_kernel       a workgroup owns 8 consecutive rows of one image: load float32, times the window, transform, store transposed
//                        as T[img][kx][y] (the 8 rows make the eight 16-byte pieces of every 128-byte run)
//   pc_cols_kernel<NU>   a workgroup owns one kx: it transforms the line of image k along y and keeps it in registers (NU elements per
//                        thread); with the next image's line it forms R = P / |P|, P = F(a) conj F(b), in LDS, transforms back along y
//                        without leaving LDS and stores transposed as G[p][y][kx].  Chain mode: every image is transformed once
//   pc_surface_kernel    a workgroup owns 8 rows of G of one pair: transform back along x, write the real part at the fftshift-ed
//                        index ((i + S / 2) mod S in both axes), and reduce its rows to one (value, shifted index) partial: the largest
//                        value, on a tie the smallest row-major index
//   pc_peak_kernel       one wave per pair: the partials in a fixed order, the clipped 5 x 5 window read back from the surface, the
//                        weighted centroid, (dx, dy, response)
//   reg_centres_kernel   pos_k = pos_{k-1} + shift_{k-1}; centre_k = S / 2 + pos_k - mean(pos): one thread
//   reg_crop_kernel      32 x 8 tiles of the output: four taps, every operation rounded on its own, float32 out
//   reg_crop_cand_kernel the same pixel function over [C][N] planes: image b mod N under the centres of candidate b / N
//
// No floating-point atomics, every sum in a fixed order: bitwise reproducible.  Launches only; shifts and centres are read on the device.
#include <climits>
#include <cmath>

#include "emd_common.hpp"
#include "fft_line.hpp"

namespace {

constexpr int kMinS = 8, kMaxS = 4096, kMaxP = 64, kMaxCrops = 65535;
constexpr int kLines = 8;   // rows per workgroup of pc_rows_kernel and pc_surface_kernel: 8 x 16 bytes = one 128-byte run of a transposed store

bool size_ok(int S) { return S >= kMinS && S <= kMaxS && (S & (S - 1)) == 0; }

// w[i] = 0.5 (1 - cos(2 pi i / (S - 1))), in the order of numpy's 0.5 * (1 - cos(2 * pi * i / (S - 1)))
__device__ __forceinline__ double hann(int i, int S) {
#pragma clang fp contract(off)
    return 0.5 * (1.0 - cos(((2.0 * M_PI) * (double)i) / (double)(S - 1)));
}

// the 2-D window of cv2.createHanningWindow
__device__ __forceinline__ double window2(double wy, double wx) { return sqrt(wy * wx); }

// grid (ceil(S / 256)); win may be NULL
__global__ __launch_bounds__(256) void pc_tables_kernel(cplx* __restrict__ tw, double* __restrict__ win, int S) {
    twiddle_entry(tw, S);
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (win && k < S) win[k] = hann(k, S);
}

// grid (S * S / 256); either output may be NULL
__global__ __launch_bounds__(256) void pc_window_kernel(double* __restrict__ w1, double* __restrict__ w2, int S) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= S * S) return;
    const int y = j / S, x = j % S;
    const double wx = hann(x, S);
    if (w1 && y == 0) w1[x] = wx;
    if (w2) w2[j] = window2(hann(y, S), wx);
}

// grid (S / 8, nimg), S * 16 bytes of LDS.  Image img is a[img] for img < na, else b[img - na].  A thread reads and rewrites only the
// elements tid + 256 u of the line outside fft_line, whose first and last statements are barriers.
__global__ __launch_bounds__(256) void pc_rows_kernel(const float* __restrict__ a, const float* __restrict__ b, int na, int S,
                                                      const double* __restrict__ win, const cplx* __restrict__ tw, cplx* __restrict__ T) {
    extern __shared__ __align__(16) unsigned char smem[];
    cplx* line = reinterpret_cast<cplx*>(smem);
    const int tid = threadIdx.x;
    const long img = blockIdx.y, SS = (long)S * S;
    const float* src = (int)img < na ? a + img * SS : b + (img - na) * SS;
    const int l0 = blockIdx.x * kLines;
    for (int l = l0; l < l0 + kLines; ++l) {
        const float* p = src + (long)l * S;
        if (win) {
            const double wy = win[l];
            for (int i = tid; i < S; i += 256) line[swz(i)] = make_double2((double)p[i] * window2(wy, win[i]), 0.0);
        } else {
            for (int i = tid; i < S; i += 256) line[swz(i)] = make_double2((double)p[i], 0.0);
        }
        fft_line(line, S, tw);
        cplx* d = T + img * SS + l;
        for (int i = tid; i < S; i += 256) d[(long)i * S] = line[swz(i)];
    }
}

// R = P / |P|, P = a conj b; 0 where |P| = 0
__device__ __forceinline__ cplx cross_power(cplx a, cplx b) {
    const double re = a.x * b.x + a.y * b.y, im = a.y * b.x - a.x * b.y;
    const double m = sqrt(re * re + im * im);
    return m > 0.0 ? make_double2(re / m, im / m) : make_double2(0.0, 0.0);
}

// grid (S) in chain mode: pairs (k, k + 1), k = 0..P-1, of the P + 1 images of T; grid (S, P) in pair mode: pair p = blockIdx.y is
// (T[p], T[P + p]).  S * 16 bytes of LDS; NU = max(S / 256, 1) elements of the previous line per thread.  T: [img][kx][y]; G: [p][y][kx]
// (R, inverse-transformed along y only).
template <int NU>
__global__ __launch_bounds__(256) void pc_cols_kernel(const cplx* __restrict__ T, cplx* __restrict__ G, int P, int chain, int S,
                                                      const cplx* __restrict__ tw) {
    extern __shared__ __align__(16) unsigned char smem[];
    cplx* line = reinterpret_cast<cplx*>(smem);
    const int tid = threadIdx.x, kx = blockIdx.x;
    const int first = chain ? 0 : (int)blockIdx.y, step = chain ? 1 : P, npairs = chain ? P : 1;
    const double inv = 1.0 / (double)S;
    cplx prev[NU];
    for (int k = 0; k <= npairs; ++k) {
        const cplx* src = T + ((long)(first + k * step) * S + kx) * S;
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            const int i = tid + 256 * u;
            if (i < S) line[swz(i)] = src[i];
        }
        fft_line(line, S, tw);
        if (k == 0) {
#pragma unroll
            for (int u = 0; u < NU; ++u) {
                const int i = tid + 256 * u;
                if (i < S) prev[u] = line[swz(i)];
            }
            continue;
        }
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            const int i = tid + 256 * u;
            if (i < S) {
                const cplx cur = line[swz(i)];
                const cplx r = cross_power(prev[u], cur);
                prev[u] = cur;
                line[swz(i)] = make_double2(r.x, -r.y);
            }
        }
        fft_line(line, S, tw);
        cplx* dst = G + (long)(first + k - 1) * S * S + kx;   // pair mode: k = 1, pair `first`
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            const int i = tid + 256 * u;
            if (i < S) {
                const cplx v = line[swz(i)];
                dst[(long)i * S] = make_double2(v.x * inv, -v.y * inv);
            }
        }
    }
}

// the larger value; on a tie the smaller index
__device__ __forceinline__ void peak_take(double& v, int& idx, double ov, int oidx) {
    if (ov > v || (ov == v && oidx < idx)) {
        v = ov;
        idx = oidx;
    }
}

// over the wave; valid in lane 0
__device__ __forceinline__ void peak_wave(double& v, int& idx) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const double ov = __shfl_down(v, off, 64);
        const int oidx = __shfl_down(idx, off, 64);
        peak_take(v, idx, ov, oidx);
    }
}

// grid (S / 8, P), max(S * 16, 128) bytes of LDS.  surf: [p][S][S] in fftshift order; pval, pidx: [p][S / 8].
__global__ __launch_bounds__(256) void pc_surface_kernel(const cplx* __restrict__ G, int S, const cplx* __restrict__ tw, double* __restrict__ surf,
                                                         double* __restrict__ pval, int* __restrict__ pidx) {
    extern __shared__ __align__(16) unsigned char smem[];
    cplx* line = reinterpret_cast<cplx*>(smem);
    const int tid = threadIdx.x, h = S >> 1;
    const long p = blockIdx.y;
    const double inv = 1.0 / (double)S;
    double best = -INFINITY;
    int bidx = INT_MAX;
    const int l0 = blockIdx.x * kLines;
    for (int y = l0; y < l0 + kLines; ++y) {
        const cplx* src = G + (p * S + y) * S;
        for (int i = tid; i < S; i += 256) {
            const cplx v = src[i];
            line[swz(i)] = make_double2(v.x, -v.y);
        }
        fft_line(line, S, tw);
        const int ys = (y + h) & (S - 1);
        double* d = surf + (p * S + ys) * S;
        for (int i = tid; i < S; i += 256) {
            const int xs = (i + h) & (S - 1);
            const double v = line[swz(i)].x * inv;   // the real part of the conjugate
            d[xs] = v;
            peak_take(best, bidx, v, ys * S + xs);
        }
    }
    peak_wave(best, bidx);
    __syncthreads();   // the line is read no more: its first 48 bytes hold the four waves' partials
    double* sv = reinterpret_cast<double*>(smem);
    int* si = reinterpret_cast<int*>(smem + 32);
    if ((tid & 63) == 0) {
        sv[tid >> 6] = best;
        si[tid >> 6] = bidx;
    }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 4; ++w) peak_take(best, bidx, sv[w], si[w]);
        pval[p * gridDim.x + blockIdx.x] = best;
        pidx[p * gridDim.x + blockIdx.x] = bidx;
    }
}

// grid (P), 64 threads.  shifts: [p][3] = (dx, dy, response)
__global__ __launch_bounds__(64) void pc_peak_kernel(const double* __restrict__ surf, const double* __restrict__ pval, const int* __restrict__ pidx,
                                                     int nparts, int S, double* __restrict__ shifts) {
#pragma clang fp contract(off)
    const long p = blockIdx.x;
    double best = -INFINITY;
    int bidx = INT_MAX;
    for (int j = threadIdx.x; j < nparts; j += 64) peak_take(best, bidx, pval[p * nparts + j], pidx[p * nparts + j]);
    peak_wave(best, bidx);
    if (threadIdx.x) return;
    if (bidx < 0 || bidx >= S * S) bidx = 0;   // a surface of NaNs has no peak
    const int py = bidx / S, px = bidx % S;
    const int y0 = max(py - 2, 0), y1 = min(py + 2, S - 1), x0 = max(px - 2, 0), x1 = min(px + 2, S - 1);
    double sv = 0.0, sx = 0.0, sy = 0.0;
    for (int y = y0; y <= y1; ++y)
        for (int x = x0; x <= x1; ++x) {
            const double v = surf[(p * S + y) * S + x];
            sv += v;
            sx += (double)x * v;
            sy += (double)y * v;
        }
    const double h = (double)(S >> 1);
    const bool flat = sv == 0.0;
    shifts[3 * p] = flat ? 0.0 : h - sx / sv;
    shifts[3 * p + 1] = flat ? 0.0 : h - sy / sv;
    shifts[3 * p + 2] = flat ? 0.0 : sv;
}

// one thread.  shifts: [N - 1][3]; centres: [N][2] = (x, y)
__global__ void reg_centres_kernel(const double* __restrict__ shifts, int N, int S, double* __restrict__ centres) {
#pragma clang fp contract(off)
    if (blockIdx.x || threadIdx.x) return;
    const double h = (double)S / 2.0;
    double px = 0.0, py = 0.0, sx = 0.0, sy = 0.0;   // pos_0 = 0 opens the sums
    for (int k = 1; k < N; ++k) {
        px += shifts[3 * (k - 1)];
        py += shifts[3 * (k - 1) + 1];
        sx += px;
        sy += py;
    }
    const double mx = sx / (double)N, my = sy / (double)N;
    px = py = 0.0;
    for (int k = 0; k < N; ++k) {
        if (k) {
            px += shifts[3 * (k - 1)];
            py += shifts[3 * (k - 1) + 1];
        }
        centres[2 * k] = (h + px) - mx;
        centres[2 * k + 1] = (h + py) - my;
    }
}

// floor(c - side / 2) as an integer and the fraction behind it; a centre that is not finite, or far outside, puts every tap outside
__device__ __forceinline__ void crop_origin(double c, int side, long& i0, double& f) {
#pragma clang fp contract(off)
    const double x0 = c - (double)side / 2.0;
    const double fl = floor(x0);
    f = x0 - fl;
    i0 = fl > -1e9 && fl < 1e9 ? (long)fl : -2000000000L;
}

// grid (ceil(side / 32), ceil(side / 8), N), block (32, 8)
__global__ __launch_bounds__(256) void reg_crop_kernel(const float* __restrict__ images, int S, const double* __restrict__ centres, int side,
                                                       float pad_val, float* __restrict__ out) {
#pragma clang fp contract(off)
    const int c = blockIdx.x * 32 + threadIdx.x, r = blockIdx.y * 8 + threadIdx.y;
    const long n = blockIdx.z;
    if (c >= side || r >= side) return;
    long ix, iy;
    double fx, fy;
    crop_origin(centres[2 * n], side, ix, fx);
    crop_origin(centres[2 * n + 1], side, iy, fy);
    const float* img = images + n * S * S;
    const long x = ix + c, y = iy + r;
    const bool xin0 = x >= 0 && x < S, xin1 = x + 1 >= 0 && x + 1 < S, yin0 = y >= 0 && y < S, yin1 = y + 1 >= 0 && y + 1 < S;
    const double pad = (double)pad_val;
    const double p00 = yin0 && xin0 ? (double)img[y * S + x] : pad, p01 = yin0 && xin1 ? (double)img[y * S + x + 1] : pad;
    const double p10 = yin1 && xin0 ? (double)img[(y + 1) * S + x] : pad, p11 = yin1 && xin1 ? (double)img[(y + 1) * S + x + 1] : pad;
    const double v = (1.0 - fy) * ((1.0 - fx) * p00 + fx * p01) + fy * ((1.0 - fx) * p10 + fx * p11);
    out[(n * side + r) * side + c] = (float)v;
}

// reg_crop_kernel's arithmetic for one output pixel (r, c) of the crop of `img` [S][S] around centre = (x, y), statement by statement,
// for the candidates' kernel.  reg_crop_kernel keeps its own text: moving it onto this function changed its instructions (not its results'
// specification), and its digest is kept (profiles/exitwave_refine_isa_digest_compare.txt).
__device__ __forceinline__ float crop_pixel(const float* __restrict__ img, int S, const double* __restrict__ centre, int side, float pad_val,
                                            int r, int c) {
#pragma clang fp contract(off)
    long ix, iy;
    double fx, fy;
    crop_origin(centre[0], side, ix, fx);
    crop_origin(centre[1], side, iy, fy);
    const long x = ix + c, y = iy + r;
    const bool xin0 = x >= 0 && x < S, xin1 = x + 1 >= 0 && x + 1 < S, yin0 = y >= 0 && y < S, yin1 = y + 1 >= 0 && y + 1 < S;
    const double pad = (double)pad_val;
    const double p00 = yin0 && xin0 ? (double)img[y * S + x] : pad, p01 = yin0 && xin1 ? (double)img[y * S + x + 1] : pad;
    const double p10 = yin1 && xin0 ? (double)img[(y + 1) * S + x] : pad, p11 = yin1 && xin1 ? (double)img[(y + 1) * S + x + 1] : pad;
    const double v = (1.0 - fy) * ((1.0 - fx) * p00 + fx * p01) + fy * ((1.0 - fx) * p10 + fx * p11);
    return (float)v;
}


// grid (ceil(side / 32), ceil(side / 8), C N), block (32, 8): plane b = c N + n is image n = b mod N under centres_table[c][n]
__global__ __launch_bounds__(256) void reg_crop_cand_kernel(const float* __restrict__ images, int N, int S,
                                                            const double* __restrict__ centres_table, int side, float pad_val,
                                                            float* __restrict__ out) {
    const int c = blockIdx.x * 32 + threadIdx.x, r = blockIdx.y * 8 + threadIdx.y;
    const long b = blockIdx.z;
    if (c >= side || r >= side) return;
    out[(b * side + r) * side + c] = crop_pixel(images + (b % N) * S * S, S, centres_table + 2 * b, side, pad_val, r, c);
}

// ---- host side -----------------------------------------------------------------------------------------------------------

using emd::check_ranges;
using emd::Range;

struct PcLayout {
    size_t tw, win, T, G, surf, pval, pidx, bytes;
    int nimg;
};

PcLayout pc_layout(int P, int S, int flags) {
    PcLayout l{};
    l.nimg = (flags & EMD_PC_CHAIN) ? P + 1 : 2 * P;
    const size_t plane = (size_t)S * S;
    size_t bytes = 0;
    l.tw = bytes;
    bytes += emd::round256((size_t)S * sizeof(cplx));
    l.win = bytes;
    bytes += emd::round256((size_t)S * sizeof(double));
    l.T = bytes;
    bytes += emd::round256((size_t)l.nimg * plane * sizeof(cplx));
    l.G = bytes;
    bytes += emd::round256((size_t)P * plane * sizeof(cplx));
    l.surf = bytes;   // used where the caller passes no surface
    bytes += emd::round256((size_t)P * plane * sizeof(double));
    l.pval = bytes;
    bytes += emd::round256((size_t)P * (S / kLines) * sizeof(double));
    l.pidx = bytes;
    bytes += emd::round256((size_t)P * (S / kLines) * sizeof(int));
    l.bytes = bytes;
    return l;
}

bool pc_shape_ok(int P, int S, int flags) { return size_ok(S) && P >= 1 && P <= kMaxP && !(flags & ~(EMD_PC_WINDOW | EMD_PC_CHAIN)); }

void launch_cols(const cplx* T, cplx* G, int P, int chain, int S, const cplx* tw, hipStream_t st) {
    const size_t lds = (size_t)S * sizeof(cplx);
    const dim3 grid((unsigned)S, chain ? 1u : (unsigned)P);
#define PC_COLS(NU) hipLaunchKernelGGL(pc_cols_kernel<NU>, grid, dim3(256), lds, st, T, G, P, chain, S, tw)
    switch (S / 256) {
        case 0:
        case 1: PC_COLS(1); break;
        case 2: PC_COLS(2); break;
        case 4: PC_COLS(4); break;
        case 8: PC_COLS(8); break;
        default: PC_COLS(16); break;
    }
#undef PC_COLS
}

}  // namespace

extern "C" int emd_hanning_window_f64(int S, double* w1, double* w2, emd_stream_t stream) {
    if (!size_ok(S)) {
        emd::set_error("emd_hanning_window_f64: bad shape (S a power of two in %d..%d; got %d)", kMinS, kMaxS, S);
        return EMD_E_INVALID;
    }
    // at least one of the two
    const Range r[] = {{w1, (size_t)S * sizeof(double), 8, w2 != nullptr, false}, {w2, (size_t)S * S * sizeof(double), 8, w1 != nullptr, false}};
    const int rc = check_ranges("emd_hanning_window_f64", r, 2, "w1 and w2 must be 8-byte aligned");
    if (rc != EMD_OK) return rc;
    hipLaunchKernelGGL(pc_window_kernel, dim3((unsigned)emd::tiles_of(S * S, 256)), dim3(256), 0, static_cast<hipStream_t>(stream), w1, w2, S);
    return emd::check_launch("emd_hanning_window_f64");
}

extern "C" size_t emd_phase_correlate_workspace_bytes(int P, int S, int flags) {
    return pc_shape_ok(P, S, flags) ? pc_layout(P, S, flags).bytes : 0;
}

extern "C" int emd_phase_correlate_f64(const float* a, const float* b, int P, int S, int flags, double* shifts, double* surface,
                                       void* workspace, size_t workspace_bytes, emd_stream_t stream) {
    if (!pc_shape_ok(P, S, flags)) {
        emd::set_error("emd_phase_correlate_f64: bad shape (1..%d pairs, S a power of two in %d..%d, flags EMD_PC_WINDOW | EMD_PC_CHAIN; got "
                       "%d pairs of %d x %d, flags %d)", kMaxP, kMinS, kMaxS, P, S, S, flags);
        return EMD_E_INVALID;
    }
    const int chain = (flags & EMD_PC_CHAIN) ? 1 : 0;
    if (chain && b) {
        emd::set_error("emd_phase_correlate_f64: with EMD_PC_CHAIN the images are a[P + 1] and b is NULL");
        return EMD_E_INVALID;
    }
    const PcLayout l = pc_layout(P, S, flags);
    const size_t plane = (size_t)S * S;
    const Range r[] = {{workspace, l.bytes, 16, false, false},
                       {a, (size_t)(chain ? P + 1 : P) * plane * sizeof(float), 4, false, true},
                       {b, (size_t)P * plane * sizeof(float), 4, chain != 0, true},
                       {shifts, (size_t)P * 3 * sizeof(double), 8, false, false},
                       {surface, (size_t)P * plane * sizeof(double), 8, true, false}};
    const char* who = "emd_phase_correlate_f64";
    const int rc = check_ranges(who, r, 5, "the workspace must be 16-byte aligned, shifts and surface 8-byte, the images 4-byte", &workspace_bytes);
    if (rc != EMD_OK) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    char* ws = static_cast<char*>(workspace);
    cplx* tw = reinterpret_cast<cplx*>(ws + l.tw);
    double* win = (flags & EMD_PC_WINDOW) ? reinterpret_cast<double*>(ws + l.win) : nullptr;
    cplx* T = reinterpret_cast<cplx*>(ws + l.T);
    cplx* G = reinterpret_cast<cplx*>(ws + l.G);
    double* surf = surface ? surface : reinterpret_cast<double*>(ws + l.surf);
    double* pval = reinterpret_cast<double*>(ws + l.pval);
    int* pidx = reinterpret_cast<int*>(ws + l.pidx);
    const size_t lds = (size_t)S * sizeof(cplx);
    const int nparts = S / kLines;
    hipLaunchKernelGGL(pc_tables_kernel, dim3((unsigned)emd::tiles_of(S, 256)), dim3(256), 0, st, tw, win, S);
    hipLaunchKernelGGL(pc_rows_kernel, dim3((unsigned)nparts, (unsigned)l.nimg), dim3(256), lds, st, a, b, chain ? P + 1 : P, S, win, tw, T);
    launch_cols(T, G, P, chain, S, tw, st);
    hipLaunchKernelGGL(pc_surface_kernel, dim3((unsigned)nparts, (unsigned)P), dim3(256), lds < 128 ? (size_t)128 : lds, st, G, S, tw, surf, pval,
                       pidx);
    hipLaunchKernelGGL(pc_peak_kernel, dim3((unsigned)P), dim3(64), 0, st, surf, pval, pidx, nparts, S, shifts);
    return emd::check_launch(who);
}

extern "C" int emd_stack_centres_f64(const double* shifts, int N, int S, double* centres, emd_stream_t stream) {
    if (N < 2 || N > kMaxP + 1 || S < 1 || S > kMaxS) {
        emd::set_error("emd_stack_centres_f64: bad shape (2..%d images of side 1..%d; got %d of side %d)", kMaxP + 1, kMaxS, N, S);
        return EMD_E_INVALID;
    }
    const Range r[] = {{shifts, (size_t)(N - 1) * 3 * sizeof(double), 8, false, true}, {centres, (size_t)N * 2 * sizeof(double), 8, false, false}};
    const int rc = check_ranges("emd_stack_centres_f64", r, 2, "shifts and centres must be 8-byte aligned");
    if (rc != EMD_OK) return rc;
    hipLaunchKernelGGL(reg_centres_kernel, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), shifts, N, S, centres);
    return emd::check_launch("emd_stack_centres_f64");
}

extern "C" int emd_crop_stack_f32(const float* images, int N, int S, const double* centres, int side, float pad_val, float* out,
                                  emd_stream_t stream) {
    if (N < 1 || N > kMaxCrops || S < 1 || S > kMaxS || side < 1 || side > S) {
        emd::set_error("emd_crop_stack_f32: bad shape (1..%d images of side 1..%d, 1 <= side <= S; got %d of side %d, side %d)", kMaxCrops,
                       kMaxS, N, S, side);
        return EMD_E_INVALID;
    }
    const Range r[] = {{images, (size_t)N * S * S * sizeof(float), 4, false, true},
                       {out, (size_t)N * side * side * sizeof(float), 4, false, false},
                       {centres, (size_t)N * 2 * sizeof(double), 8, false, true}};
    const int rc = check_ranges("emd_crop_stack_f32", r, 3, "centres must be 8-byte aligned, images and out 4-byte");
    if (rc != EMD_OK) return rc;
    hipLaunchKernelGGL(reg_crop_kernel, dim3((unsigned)emd::tiles_of(side, 32), (unsigned)emd::tiles_of(side, 8), (unsigned)N), dim3(32, 8), 0,
                       static_cast<hipStream_t>(stream), images, S, centres, side, pad_val, out);
    return emd::check_launch("emd_crop_stack_f32");
}

// the launch of emd_crop_candidates_f32, for emd_exitwave_refine_f64 (exitwave.hip), which has checked the arguments
void emd::launch_crop_candidates(const float* images, int N, int S, const double* centres_table, int C, int side, float pad_val, float* out,
                                 hipStream_t st) {
    hipLaunchKernelGGL(reg_crop_cand_kernel, dim3((unsigned)emd::tiles_of(side, 32), (unsigned)emd::tiles_of(side, 8), (unsigned)(C * N)),
                       dim3(32, 8), 0, st, images, N, S, centres_table, side, pad_val, out);
}

extern "C" int emd_crop_candidates_f32(const float* images, int N, int S0, const double* centres_table, int C, int side, float pad_val,
                                       float* out, emd_stream_t stream) {
    if (N < 1 || C < 1 || (long)C * N > kMaxCrops || S0 < 1 || S0 > kMaxS || side < 1 || side > S0) {
        emd::set_error("emd_crop_candidates_f32: bad shape (candidates x images in 1..%d, images of side 1..%d, 1 <= side <= S0; got %d "
                       "candidates of %d images of side %d, side %d)", kMaxCrops, kMaxS, C, N, S0, side);
        return EMD_E_INVALID;
    }
    const Range r[] = {{images, (size_t)N * S0 * S0 * sizeof(float), 4, false, true},
                       {out, (size_t)C * N * side * side * sizeof(float), 4, false, false},
                       {centres_table, (size_t)C * N * 2 * sizeof(double), 8, false, true}};
    const int rc = check_ranges("emd_crop_candidates_f32", r, 3, "centres_table must be 8-byte aligned, images and out 4-byte");
    if (rc != EMD_OK) return rc;
    emd::launch_crop_candidates(images, N, S0, centres_table, C, side, pad_val, out, static_cast<hipStream_t>(stream));
    return emd::check_launch("emd_crop_candidates_f32");
}
