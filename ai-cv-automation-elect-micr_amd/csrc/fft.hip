// The 2-D real-to-complex FFT in double and the radial frequency profile of img_params.m:53-77: the four
// *Freq2048 fields of the harvester's table.  S x S float32 images, S a power of two, 8..4096; every image on its own.
//
//   twiddle_kernel        exp(-2 pi i k / S), k = 0..S-1, by sincospi in double, written into the workspace on every call
//   fft_rows_kernel       a workgroup owns 8 rows: two real rows are one complex line z = a + i b, transformed in LDS and split by
//                         Hermitian symmetry; kx = 0..S/2 is kept and written TRANSPOSED, T[b][kx][ky], so a column is a contiguous line
//   fft_cols_kernel       a workgroup per (kx, b): the same 1-D transform; writes the half spectrum in numpy.fft.rfft2's layout, or
//                         |F| as doubles over the first half of the line it read (MAG)
//   radial_bin_kernel     a workgroup per (bin, b): integer bin membership, fixed-order sums, the last-visited member for radialFreqs
//   radial_final_kernel   grid (B): p = profile / sum(profile) * radialFreqs and the four moments, two-pass
//
// The 1-D transform (fft_line.hpp, shared with exitwave.hip) is a Stockham autosort of radix-4 passes and a last radix-2 pass where
// log2 S is odd, on ONE line of S complex doubles in LDS (64 KiB at 4096), swizzled.
// No floating-point atomics: bitwise reproducible, and an image's result does not depend on the batch it is in.
#include <cmath>

#include "fft_line.hpp"
#include "stencil_rows.hpp"

namespace {

constexpr int kMinS = 8, kMaxS = 4096;
constexpr int kRowsPerBlock = 8;   // the row pass: four pairs; the four 32-byte pieces of every 128-byte run of T come from one workgroup

bool size_ok(int S) { return S >= kMinS && S <= kMaxS && (S & (S - 1)) == 0; }
int radial_bins(int S) {   // ceil(sqrt(2 mid^2)), mid = S / 2 + 1: the smallest r with r^2 >= 2 mid^2
    const long n = 2L * (S / 2 + 1) * (S / 2 + 1);
    long r = (long)std::sqrt((double)n);
    while (r * r < n) ++r;
    while ((r - 1) * (r - 1) >= n) --r;
    return (int)r;
}

__global__ __launch_bounds__(256) void twiddle_kernel(cplx* __restrict__ tw, int S) {
    twiddle_entry(tw, S);
}

// grid (S / 8, B), S * 16 bytes of LDS.  T: [B][S / 2 + 1][S].
__global__ __launch_bounds__(256) void fft_rows_kernel(const float* __restrict__ x, int S, const cplx* __restrict__ tw, cplx* __restrict__ T) {
    extern __shared__ __align__(16) unsigned char smem[];
    cplx* line = reinterpret_cast<cplx*>(smem);
    const int tid = threadIdx.x, h = S >> 1;
    const float* xb = x + (long)blockIdx.y * S * S;
    cplx* Tb = T + (long)blockIdx.y * (h + 1) * S;
    for (int p = 0; p < kRowsPerBlock / 2; ++p) {
        const int r0 = blockIdx.x * kRowsPerBlock + 2 * p;
        const float* ra = xb + (long)r0 * S;
        for (int i = tid; i < S; i += 256) line[swz(i)] = make_double2((double)ra[i], (double)ra[S + i]);
        fft_line(line, S, tw);
        // Z = A + i B with A, B the rows' transforms: A[k] = (Z[k] + conj Z[S - k]) / 2, B[k] = (Z[k] - conj Z[S - k]) / 2i
        for (int k = tid; k <= h; k += 256) {
            const cplx zk = line[swz(k)], zn = line[swz((S - k) & (S - 1))];
            cplx* out = Tb + (long)k * S + r0;
            out[0] = make_double2(0.5 * (zk.x + zn.x), 0.5 * (zk.y - zn.y));
            out[1] = make_double2(0.5 * (zk.y + zn.y), -0.5 * (zk.x - zn.x));
        }
        __syncthreads();   // the line is loaded again
    }
}

// grid (S / 2 + 1, B), S * 16 bytes of LDS.  MAG: |F| over the first S doubles of the line it read (the lines stay 2 S doubles apart);
// else spec [B][S][S / 2 + 1].
template <bool MAG>
__global__ __launch_bounds__(256) void fft_cols_kernel(cplx* __restrict__ T, int S, const cplx* __restrict__ tw, cplx* __restrict__ spec) {
    extern __shared__ __align__(16) unsigned char smem[];
    cplx* line = reinterpret_cast<cplx*>(smem);
    const int tid = threadIdx.x, h = S >> 1, kx = blockIdx.x;
    cplx* src = T + ((long)blockIdx.y * (h + 1) + kx) * S;
    for (int i = tid; i < S; i += 256) line[swz(i)] = src[i];
    fft_line(line, S, tw);   // its first barrier: the whole line has been read before any of it is written below
    if (MAG) {
        double* dst = reinterpret_cast<double*>(src);
        for (int i = tid; i < S; i += 256) {
            const cplx f = line[swz(i)];
            dst[i] = sqrt(f.x * f.x + f.y * f.y);
        }
    } else {
        cplx* dst = spec + (long)blockIdx.y * S * (h + 1) + kx;
        for (int i = tid; i < S; i += 256) dst[(long)i * (h + 1)] = line[swz(i)];
    }
}

#pragma clang fp contract(off)   // the profile and its moments: every operation rounds on its own, as in the host restatement

__device__ __forceinline__ int isqrt_floor(long v) {   // v >= 0, below 2^53
    long r = (long)sqrt((double)v);
    while (r * r > v) --r;
    while ((r + 1) * (r + 1) <= v) ++r;
    return (int)r;
}

// grid (R, B).  mag: image b, line a (= |kx|, 0..S/2) at mag + (b (S/2 + 1) + a) 2 S, S doubles over the unshifted ky.
// With signed frequencies ky, kx in [-S/2, S/2 - 1] and n = ky^2 + kx^2, bin t holds (t - 1)^2 < n <= t^2 (t = 0: n = 0).  Lines
// 1..S/2-1 stand for +kx and -kx (|F(-ky, -kx)| = |F(ky, kx)|, and the ky = -S/2 row is its own partner); lines 0 and S/2 (kx = -S/2)
// stand for themselves.  A thread adds its lines' members in ascending ky; the workgroup's sum has a fixed order.
// freq[b][t] = sqrt(n) / R of the bin's member with the largest kx, and among those the largest ky (the last one img_params.m's
// loop visits); 0 for an empty bin.
__global__ __launch_bounds__(256) void radial_bin_kernel(const double* __restrict__ mag, int S, int R, double* __restrict__ praw,
                                                         double* __restrict__ freq) {
    __shared__ double sh[4];
    __shared__ int shk[256];
    const int tid = threadIdx.x, h = S >> 1, t = blockIdx.x;
    const long b = blockIdx.y;
    const double* mb = mag + b * (long)(h + 1) * 2 * S;
    const long U = (long)t * t, L = t > 0 ? (long)(t - 1) * (t - 1) : -1;
    double s = 0.0;
    int best = -1;
    for (int a = tid; a <= h; a += 256) {
        const long hi2 = U - (long)a * a, lo2 = L - (long)a * a;
        if (hi2 < 0) continue;
        const int hi = isqrt_floor(hi2), lo1 = lo2 < 0 ? 0 : isqrt_floor(lo2) + 1;   // lo1 <= |ky| <= hi
        const int n0 = min(hi, h), n1 = max(lo1, 1);                                  // ky = -n0 .. -n1
        const int p0 = lo1, p1 = min(hi, h - 1);                                      // ky = p0 .. p1
        const double* row = mb + (long)a * 2 * S;
        double acc = 0.0;
        for (int m = n0; m >= n1; --m) acc += row[S - m];
        for (int m = p0; m <= p1; ++m) acc += row[m];
        s += (a == 0 || a == h) ? acc : 2.0 * acc;
        int ky;
        if (p1 >= p0) ky = p1;
        else if (n0 >= n1) ky = -n1;
        else continue;
        const int kx = a == h ? -h : a;
        best = max(best, (kx + h) * 8192 + (ky + h));
    }
    const double total = block_sum_thread0(s, sh);
    shk[tid] = best;
    __syncthreads();
    for (int off = 128; off >= 1; off >>= 1) {
        if (tid < off) shk[tid] = max(shk[tid], shk[tid + off]);
        __syncthreads();
    }
    if (tid == 0) {
        praw[b * R + t] = total;
        double f = 0.0;
        if (shk[0] >= 0) {
            const long kx = shk[0] / 8192 - h, ky = shk[0] % 8192 - h;
            f = sqrt((double)(kx * kx + ky * ky)) / (double)R;
        }
        freq[b * R + t] = f;
    }
}

// grid (B): p, then sum p, std (N - 1), skewness and kurtosis (population central moments) over the R entries
__global__ __launch_bounds__(256) void radial_final_kernel(const double* __restrict__ praw, const double* __restrict__ freq, int R,
                                                           double* __restrict__ pbuf, double* __restrict__ profile,
                                                           double* __restrict__ stats) {
    __shared__ double sh[256];
    const int tid = threadIdx.x;
    const long b = blockIdx.x;
    const double total = block_sum_fixed(praw + b * R, R, 1, sh);
    double* p = pbuf + b * R;
    double s = 0.0;
    for (int i = tid; i < R; i += 256) {
        const double v = praw[b * R + i] / total * freq[b * R + i];
        p[i] = v;   // read back below by the thread that wrote it
        if (profile) profile[b * R + i] = v;
        s += v;
    }
    const double sum = block_tree_sum(s, sh), mu = sum / (double)R;
    double c2 = 0.0, c3 = 0.0, c4 = 0.0;
    for (int i = tid; i < R; i += 256) {
        const double d = p[i] - mu, d2 = d * d;
        c2 += d2;
        c3 += d2 * d;
        c4 += d2 * d2;
    }
    c2 = block_tree_sum(c2, sh);
    c3 = block_tree_sum(c3, sh);
    c4 = block_tree_sum(c4, sh);
    if (tid != 0) return;
    const double m2 = c2 / (double)R;
    double* o = stats + b * EMD_NFREQ;
    o[0] = sum;
    o[1] = sqrt(c2 / ((double)R - 1.0));
    o[2] = (c3 / (double)R) / (m2 * sqrt(m2));
    o[3] = (c4 / (double)R) / (m2 * m2);
}

// ---- host side -----------------------------------------------------------------------------------------------------------

struct FftLayout {
    int R;
    size_t tw, T, praw, freq, pbuf, bytes;
};

FftLayout fft_layout(int B, int S, bool profile) {
    FftLayout l{};
    l.R = radial_bins(S);
    size_t bytes = 0;
    l.tw = bytes;
    bytes += emd::round256((size_t)S * sizeof(cplx));
    l.T = bytes;
    bytes += emd::round256((size_t)B * (S / 2 + 1) * S * sizeof(cplx));
    if (profile) {
        const size_t n = emd::round256((size_t)B * l.R * sizeof(double));
        l.praw = bytes;
        l.freq = bytes + n;
        l.pbuf = bytes + 2 * n;
        bytes += 3 * n;
    }
    l.bytes = bytes;
    return l;
}

// The checks the two entry points share; 1: nothing to do
int fft_check(const char* who, const void* x, int B, int S, const void* out, size_t out_bytes, const void* workspace,
              size_t workspace_bytes, size_t need) {
    if (B < 0 || B > 65535 || !size_ok(S)) {
        emd::set_error("%s: bad shape (batch 0..65535, S a power of two in %d..%d; got %d x %d x %d)", who, kMinS, kMaxS, B, S, S);
        return EMD_E_INVALID;
    }
    if (B == 0) return 1;
    if (!x || !out || !workspace) {
        emd::set_error("%s: null pointer", who);
        return EMD_E_INVALID;
    }
    if (workspace_bytes < need) {
        emd::set_error("%s: workspace too small (%zu bytes, needs %zu)", who, workspace_bytes, need);
        return EMD_E_INVALID;
    }
    if (!emd::aligned16(workspace) || !emd::aligned16(out)) {
        emd::set_error("%s: the workspace and the output must be 16-byte aligned", who);
        return EMD_E_ALIGN;
    }
    const size_t nx = (size_t)B * S * S * sizeof(float);
    if (emd::overlap(workspace, need, x, nx) || emd::overlap(workspace, need, out, out_bytes) || emd::overlap(out, out_bytes, x, nx)) {
        emd::set_error("%s: x, the output and the workspace may not overlap", who);
        return EMD_E_INVALID;
    }
    return EMD_OK;
}

// the table and the row pass
void launch_rows(const float* x, int B, int S, cplx* tw, cplx* T, hipStream_t st) {
    hipLaunchKernelGGL(twiddle_kernel, dim3((unsigned)emd::tiles_of(S, 256)), dim3(256), 0, st, tw, S);
    hipLaunchKernelGGL(fft_rows_kernel, dim3((unsigned)(S / kRowsPerBlock), (unsigned)B), dim3(256), (size_t)S * sizeof(cplx), st, x, S,
                       tw, T);
}

}  // namespace

extern "C" int emd_radial_bins(int S) { return size_ok(S) ? radial_bins(S) : 0; }

extern "C" size_t emd_rfft2_workspace_bytes(int B, int S) {
    if (B < 1 || B > 65535 || !size_ok(S)) return 0;
    return fft_layout(B, S, false).bytes;
}

extern "C" int emd_rfft2_f64(const float* x, int B, int S, double* spec, void* workspace, size_t workspace_bytes, emd_stream_t stream) {
    const FftLayout l = size_ok(S) && B > 0 && B <= 65535 ? fft_layout(B, S, false) : FftLayout{};
    const int rc = fft_check("emd_rfft2_f64", x, B, S, spec, (size_t)B * S * (S / 2 + 1) * sizeof(cplx), workspace, workspace_bytes, l.bytes);
    if (rc != EMD_OK) return rc == 1 ? EMD_OK : rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    char* ws = static_cast<char*>(workspace);
    cplx* tw = reinterpret_cast<cplx*>(ws + l.tw);
    cplx* T = reinterpret_cast<cplx*>(ws + l.T);
    launch_rows(x, B, S, tw, T, st);
    hipLaunchKernelGGL(fft_cols_kernel<false>, dim3((unsigned)(S / 2 + 1), (unsigned)B), dim3(256), (size_t)S * sizeof(cplx), st, T, S, tw,
                       reinterpret_cast<cplx*>(spec));
    return emd::check_launch("emd_rfft2_f64");
}

extern "C" size_t emd_freq_stats_workspace_bytes(int B, int S) {
    if (B < 1 || B > 65535 || !size_ok(S)) return 0;
    return fft_layout(B, S, true).bytes;
}

extern "C" int emd_freq_stats_f64(const float* x, int B, int S, double* profile, double* freq_stats, void* workspace,
                                  size_t workspace_bytes, emd_stream_t stream) {
    const FftLayout l = size_ok(S) && B > 0 && B <= 65535 ? fft_layout(B, S, true) : FftLayout{};
    const int rc = fft_check("emd_freq_stats_f64", x, B, S, freq_stats, (size_t)B * EMD_NFREQ * sizeof(double), workspace, workspace_bytes,
                             l.bytes);
    if (rc != EMD_OK) return rc == 1 ? EMD_OK : rc;
    const size_t np = (size_t)B * l.R * sizeof(double), nx = (size_t)B * S * S * sizeof(float);
    EMD_REQUIRE(!profile || (!emd::overlap(profile, np, workspace, l.bytes) && !emd::overlap(profile, np, x, nx) &&
                             !emd::overlap(profile, np, freq_stats, (size_t)B * EMD_NFREQ * sizeof(double))),
                EMD_E_INVALID, "emd_freq_stats_f64: the profile may not overlap x, freq_stats or the workspace");
    hipStream_t st = static_cast<hipStream_t>(stream);
    char* ws = static_cast<char*>(workspace);
    cplx* tw = reinterpret_cast<cplx*>(ws + l.tw);
    cplx* T = reinterpret_cast<cplx*>(ws + l.T);
    double* praw = reinterpret_cast<double*>(ws + l.praw);
    double* freq = reinterpret_cast<double*>(ws + l.freq);
    double* pbuf = reinterpret_cast<double*>(ws + l.pbuf);
    launch_rows(x, B, S, tw, T, st);
    hipLaunchKernelGGL(fft_cols_kernel<true>, dim3((unsigned)(S / 2 + 1), (unsigned)B), dim3(256), (size_t)S * sizeof(cplx), st, T, S, tw,
                       static_cast<cplx*>(nullptr));
    hipLaunchKernelGGL(radial_bin_kernel, dim3((unsigned)l.R, (unsigned)B), dim3(256), 0, st, reinterpret_cast<const double*>(T), S, l.R,
                       praw, freq);
    hipLaunchKernelGGL(radial_final_kernel, dim3((unsigned)B), dim3(256), 0, st, praw, freq, l.R, pbuf, profile, freq_stats);
    return emd::check_launch("emd_freq_stats_f64");
}
