// The 2-D FFT of any side (include/emdenoise.h "2-D FFT of any side"), in double: complex and real-input transforms
// of [B][H][W] with H and W independent, and Fresnel propagation between two of them.  A side that is a power of two, 8..4096, is one
// fft_line.hpp line, as in exitwave.hip (the same bits).  Any other side n, 2..2048, is Bluestein's chirp-z: with
// M = max(8, the smallest power of two >= 2 n - 1) <= 4096 and the chirp w[k] = exp(-i pi k^2 / n),
//     Y[k] = w[k] IFFT_M(FFT_M(a) Bf)[k],   a[j] = x[j] w[j] (0 from n up to M),   Bf = FFT_M(b),   b[j] = b[M - j] = conj w[j],
// two fft_line transforms of M on one line in LDS (64 KiB at M = 4096).  The inverse is by conjugation: x = conj(F(conj Y)) / n.
//
//   fa_tables_kernel     the twiddles of M, exp(-2 pi i k / M), and the chirp w [n] (k^2 mod 2 n in integers, then sincospi)
//   fa_filter_kernel     Bf [M] = FFT_M(b), one workgroup, by the same fft_line
//   fa_pass_kernel<OP>   one workgroup per line, grid (lines of one image, B): load a contiguous line (complex, or float32 as the real
//                        part), transform, store n_out elements with strides of the caller's choice (straight or transposed).
//                        OP: FWD; INV; PROP (forward, times Hf, inverse, without leaving LDS)
//
// The tables are written into the workspace by the two set-up kernels on every call, one set per distinct length: nothing persists,
// nothing is uploaded.  Every order is fixed and there are no atomics: an image's bits depend neither on B nor on the other images.
// Launches only; the defocuses are read on the device.
#include <cmath>

#include "emd_common.hpp"
#include "fft_line.hpp"

namespace {

constexpr int kMinPow2 = 8, kMaxPow2 = 4096, kMinAny = 2, kMaxAny = 2048;

enum { OP_FWD = 0, OP_INV = 1, OP_PROP = 2 };

bool plain_ok(int n) { return n >= kMinPow2 && n <= kMaxPow2 && (n & (n - 1)) == 0; }

// the length of the LDS line that serves a transform of n: n, Bluestein's M, or 0
int line_of(int n) {
    if (plain_ok(n)) return n;
    if (n < kMinAny || n > kMaxAny) return 0;
    int M = kMinPow2;
    while (M < 2 * n - 1) M <<= 1;
    return M;
}

// One length's tables.  w == NULL: a plain line, M == n.
struct LineTab {
    int n, M;
    const cplx *tw, *w, *Bf;   // exp(-2 pi i k / M) [M]; the chirp [n]; the filter's spectrum [M]
};

struct Optics {
    double lam, span_y, span_x, c4;   // wavelength; H px; W px; 0.5 lam^3 Cs
};

// Hf at the unshifted indices (iy, ix) of an H x W grid: j = i below (n + 1) / 2, else i - n (numpy.fft.fftfreq); q = j / (n px);
// t = lam df q2 + 0.5 lam^3 Cs q2 q2, every operation rounded on its own (as emd_transfer_function_f64); Hf = cospi(t) + i sinpi(t)
__device__ __forceinline__ cplx transfer_h(int iy, int ix, int H, int W, double df, Optics o) {
#pragma clang fp contract(off)
    const int jy = iy < ((H + 1) >> 1) ? iy : iy - H, jx = ix < ((W + 1) >> 1) ? ix : ix - W;
    const double qy = (double)jy / o.span_y, qx = (double)jx / o.span_x;
    const double q2 = qy * qy + qx * qx;
    const double t = o.lam * df * q2 + o.c4 * q2 * q2;
    double s, c;
    sincospi(t, &s, &c);
    return make_double2(c, s);
}

// grid (M / 256): tw[k], k < M; w[k] = (cospi(t / n), -sinpi(t / n)) with t = k^2 mod 2 n, k < n (w == NULL: a plain line)
__global__ __launch_bounds__(256) void fa_tables_kernel(cplx* __restrict__ tw, int M, cplx* __restrict__ w, int n) {
    twiddle_entry(tw, M);
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (w && k < n) {
        const int t = (k * k) % (2 * n);   // k < 2048: k^2 < 2^22
        double s, c;
        sincospi((double)t / (double)n, &s, &c);
        w[k] = make_double2(c, -s);
    }
}

// grid (1), M * 16 bytes of LDS: Bf = FFT_M(b), b[j] = conj w[j] for j < n, b[M - j] = conj w[j] for 1 <= j < n, 0 elsewhere
// (M >= 2 n - 1: the two runs do not meet)
__global__ __launch_bounds__(256) void fa_filter_kernel(cplx* __restrict__ Bf, int M, const cplx* __restrict__ w, int n,
                                                        const cplx* __restrict__ tw) {
    extern __shared__ __align__(16) unsigned char smem[];
    cplx* line = reinterpret_cast<cplx*>(smem);
    for (int j = threadIdx.x; j < M; j += 256) {
        cplx v = make_double2(0.0, 0.0);
        if (j < n)
            v = make_double2(w[j].x, -w[j].y);
        else if (M - j < n)
            v = make_double2(w[M - j].x, -w[M - j].y);
        line[swz(j)] = v;
    }
    fft_line(line, M, tw);
    for (int j = threadIdx.x; j < M; j += 256) Bf[j] = line[swz(j)];
}

// What element i < n of a line's input becomes in LDS: itself, or times the chirp.  Elements n..M-1 of a Bluestein line are zeros.
__device__ __forceinline__ cplx chirped(cplx v, int i, const LineTab& t) { return t.w ? cmul(v, t.w[i]) : v; }

// The forward, unnormalised transform of the n elements that were stored through chirped(): line[swz(0..n-1)] in natural order
// (elements from n up hold nothing of use afterwards).  A thread touches only the elements tid + 256 u outside fft_line, whose first
// and last statements are barriers.
__device__ __forceinline__ void dft_line(cplx* line, const LineTab& t) {
    fft_line(line, t.M, t.tw);
    if (!t.w) return;
    for (int i = threadIdx.x; i < t.M; i += 256) {
        const cplx v = cmul(line[swz(i)], t.Bf[i]);
        line[swz(i)] = make_double2(v.x, -v.y);
    }
    fft_line(line, t.M, t.tw);
    const double inv = 1.0 / (double)t.M;   // exact
    for (int i = threadIdx.x; i < t.n; i += 256) {
        const cplx v = line[swz(i)];
        line[swz(i)] = cmul(make_double2(v.x * inv, -v.y * inv), t.w[i]);
    }
}

struct PassArgs {
    const void* src;   // lines of n complex doubles, or of n float32 (src_real)
    long src_batch, src_line;
    int src_real;
    cplx* dst;         // element i of line l of image b: dst[b dst_batch + l dst_line + i dst_elem], i < n_out <= n
    long dst_batch, dst_line, dst_elem;
    int n_out;
    LineTab t;
    const double* defocus;   // PROP: one per image; the line is kx, its elements are ky
    int H, W;
    Optics o;
};

// grid (lines, B), M * 16 bytes of LDS
template <int OP>
__global__ __launch_bounds__(256) void fa_pass_kernel(PassArgs a) {
    extern __shared__ __align__(16) unsigned char smem[];
    cplx* line = reinterpret_cast<cplx*>(smem);
    const int tid = threadIdx.x, n = a.t.n, M = a.t.M;
    const long b = blockIdx.y, l = blockIdx.x;
    if (a.src_real) {
        const float* p = static_cast<const float*>(a.src) + b * a.src_batch + l * a.src_line;
        for (int i = tid; i < M; i += 256)
            line[swz(i)] = i < n ? chirped(make_double2((double)p[i], 0.0), i, a.t) : make_double2(0.0, 0.0);
    } else {
        const cplx* p = static_cast<const cplx*>(a.src) + b * a.src_batch + l * a.src_line;
        for (int i = tid; i < M; i += 256) {
            cplx v = make_double2(0.0, 0.0);
            if (i < n) {
                v = p[i];
                if (OP == OP_INV) v.y = -v.y;
                v = chirped(v, i, a.t);
            }
            line[swz(i)] = v;
        }
    }
    dft_line(line, a.t);
    if (OP == OP_PROP) {
        const double df = a.defocus[b];
        for (int i = tid; i < M; i += 256) {
            cplx v = make_double2(0.0, 0.0);
            if (i < n) {
                v = cmul(line[swz(i)], transfer_h(i, (int)l, a.H, a.W, df, a.o));
                v = chirped(make_double2(v.x, -v.y), i, a.t);
            }
            line[swz(i)] = v;
        }
        dft_line(line, a.t);
    }
    cplx* d = a.dst + b * a.dst_batch + l * a.dst_line;
    const double dn = (double)n;
    for (int i = tid; i < a.n_out; i += 256) {
        cplx v = line[swz(i)];
        if (OP != OP_FWD) v = make_double2(v.x / dn, -v.y / dn);
        d[(long)i * a.dst_elem] = v;
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------------

bool batch_ok(int B) { return B >= 0 && B <= 65535; }
bool shape_ok(int B, int H, int W) { return batch_ok(B) && line_of(H) && line_of(W); }

// where one length's tables lie in the workspace
struct TabLayout {
    int n, M;
    bool blue;
    size_t tw, w, Bf;
};

size_t place_tables(TabLayout& t, int n, size_t bytes) {
    t.n = n;
    t.M = line_of(n);
    t.blue = !plain_ok(n);
    t.tw = bytes;
    bytes += emd::round256((size_t)t.M * sizeof(cplx));
    if (t.blue) {
        t.w = bytes;
        bytes += emd::round256((size_t)n * sizeof(cplx));
        t.Bf = bytes;
        bytes += emd::round256((size_t)t.M * sizeof(cplx));
    }
    return bytes;
}

// The tables of W (rows) and of H (columns; the rows' own where H == W), then T: the first pass's lines, transposed, kept lines of
// H each; then U (propagate only): [B][H][W]
struct Layout {
    TabLayout row, col;
    size_t T, U, bytes;
};

Layout layout(int B, int H, int W, int kept, bool with_u) {
    Layout l{};
    size_t bytes = place_tables(l.row, W, 0);
    if (H == W)
        l.col = l.row;
    else
        bytes = place_tables(l.col, H, bytes);
    l.T = bytes;
    bytes += emd::round256((size_t)B * kept * H * sizeof(cplx));
    if (with_u) {
        l.U = bytes;
        bytes += emd::round256((size_t)B * H * W * sizeof(cplx));
    }
    l.bytes = bytes;
    return l;
}

LineTab write_tables(const TabLayout& t, char* ws, hipStream_t st) {
    cplx* tw = reinterpret_cast<cplx*>(ws + t.tw);
    cplx* w = t.blue ? reinterpret_cast<cplx*>(ws + t.w) : nullptr;
    cplx* Bf = t.blue ? reinterpret_cast<cplx*>(ws + t.Bf) : nullptr;
    hipLaunchKernelGGL(fa_tables_kernel, dim3((unsigned)emd::tiles_of(t.M, 256)), dim3(256), 0, st, tw, t.M, w, t.n);
    if (t.blue) hipLaunchKernelGGL(fa_filter_kernel, dim3(1), dim3(256), (size_t)t.M * sizeof(cplx), st, Bf, t.M, w, t.n, tw);
    return LineTab{t.n, t.M, tw, w, Bf};
}

// the set-up launches of a call: (row tables, column tables)
void write_all_tables(const Layout& l, char* ws, hipStream_t st, LineTab* row, LineTab* col) {
    *row = write_tables(l.row, ws, st);
    *col = l.col.tw == l.row.tw ? *row : write_tables(l.col, ws, st);
}

template <int OP>
void launch_pass(const PassArgs& a, int nlines, int B, hipStream_t st) {
    hipLaunchKernelGGL(fa_pass_kernel<OP>, dim3((unsigned)nlines, (unsigned)B), dim3(256), (size_t)a.t.M * sizeof(cplx), st, a);
}

PassArgs pass_args(const void* src, int src_real, long src_batch, long src_line, cplx* dst, long dst_batch, long dst_line, long dst_elem,
                   int n_out, const LineTab& t) {
    PassArgs a{};
    a.src = src;
    a.src_real = src_real;
    a.src_batch = src_batch;
    a.src_line = src_line;
    a.dst = dst;
    a.dst_batch = dst_batch;
    a.dst_line = dst_line;
    a.dst_elem = dst_elem;
    a.n_out = n_out;
    a.t = t;
    return a;
}

const char* const kAligned = "the inputs, the outputs and the workspace must be 16-byte aligned (float32 images: 4-byte, defocuses: 8-byte)";

void shape_error(const char* who, int B, int H, int W) {
    emd::set_error("%s: bad shape (batch 0..65535, each side %d..%d, or a power of two up to %d; got %d x %d x %d)", who, kMinAny, kMaxAny,
                   kMaxPow2, B, H, W);
}

}  // namespace

extern "C" int emd_fft_any_line(int n) { return line_of(n); }

extern "C" size_t emd_cfft2_any_workspace_bytes(int B, int H, int W) {
    if (B < 1 || !shape_ok(B, H, W)) return 0;
    return layout(B, H, W, W, false).bytes;
}

extern "C" int emd_cfft2_any_f64(const void* x, int x_is_real_f32, int B, int H, int W, int inverse, double* out, void* workspace,
                                 size_t workspace_bytes, emd_stream_t stream) {
    const char* who = "emd_cfft2_any_f64";
    if (!shape_ok(B, H, W)) {
        shape_error(who, B, H, W);
        return EMD_E_INVALID;
    }
    if (B == 0) return EMD_OK;
    const Layout l = layout(B, H, W, W, false);
    const size_t ne = (size_t)B * H * W;
    const emd::Range r[] = {{workspace, l.bytes, 16, false, false},
                            {x, ne * (x_is_real_f32 ? sizeof(float) : sizeof(cplx)), x_is_real_f32 ? 4u : 16u, false, true},
                            {out, ne * sizeof(cplx), 16, false, false}};
    const int rc = emd::check_ranges(who, r, 3, kAligned, &workspace_bytes);
    if (rc != EMD_OK) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    char* ws = static_cast<char*>(workspace);
    LineTab row, col;
    write_all_tables(l, ws, st, &row, &col);
    cplx* T = reinterpret_cast<cplx*>(ws + l.T);
    const long HW = (long)H * W;
    // rows, written transposed: T [B][W][H]; then the columns, written transposed again
    const PassArgs pr = pass_args(x, x_is_real_f32 ? 1 : 0, HW, W, T, HW, 1, H, W, row);
    const PassArgs pc = pass_args(T, 0, HW, H, reinterpret_cast<cplx*>(out), HW, 1, W, H, col);
    if (inverse) {
        launch_pass<OP_INV>(pr, H, B, st);
        launch_pass<OP_INV>(pc, W, B, st);
    } else {
        launch_pass<OP_FWD>(pr, H, B, st);
        launch_pass<OP_FWD>(pc, W, B, st);
    }
    return emd::check_launch(who);
}

extern "C" size_t emd_rfft2_any_workspace_bytes(int B, int H, int W) {
    if (B < 1 || !shape_ok(B, H, W)) return 0;
    return layout(B, H, W, W / 2 + 1, false).bytes;
}

extern "C" int emd_rfft2_any_f64(const float* x, int B, int H, int W, double* spec, void* workspace, size_t workspace_bytes,
                                 emd_stream_t stream) {
    const char* who = "emd_rfft2_any_f64";
    if (!shape_ok(B, H, W)) {
        shape_error(who, B, H, W);
        return EMD_E_INVALID;
    }
    if (B == 0) return EMD_OK;
    const int K = W / 2 + 1;
    const Layout l = layout(B, H, W, K, false);
    const emd::Range r[] = {{workspace, l.bytes, 16, false, false},
                            {x, (size_t)B * H * W * sizeof(float), 4, false, true},
                            {spec, (size_t)B * H * K * sizeof(cplx), 16, false, false}};
    const int rc = emd::check_ranges(who, r, 3, kAligned, &workspace_bytes);
    if (rc != EMD_OK) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    char* ws = static_cast<char*>(workspace);
    LineTab row, col;
    write_all_tables(l, ws, st, &row, &col);
    cplx* T = reinterpret_cast<cplx*>(ws + l.T);
    // every real row as a complex line, of which kx = 0..W/2 are kept: T [B][K][H]; then the K columns
    launch_pass<OP_FWD>(pass_args(x, 1, (long)H * W, W, T, (long)K * H, 1, H, K, row), H, B, st);
    launch_pass<OP_FWD>(pass_args(T, 0, (long)K * H, H, reinterpret_cast<cplx*>(spec), (long)H * K, 1, K, H, col), K, B, st);
    return emd::check_launch(who);
}

extern "C" size_t emd_propagate_any_workspace_bytes(int B, int H, int W) {
    if (B < 1 || !shape_ok(B, H, W)) return 0;
    return layout(B, H, W, W, true).bytes;
}

extern "C" int emd_propagate_any_f64(const void* psi, int psi_is_real_f32, int B, int H, int W, const double* defocus, double wavelength,
                                     double px, double cs, double* out, void* workspace, size_t workspace_bytes, emd_stream_t stream) {
    const char* who = "emd_propagate_any_f64";
    if (!shape_ok(B, H, W) || !(px > 0.0)) {
        emd::set_error("%s: bad shape (batch 0..65535, each side %d..%d, or a power of two up to %d, px > 0; got %d x %d x %d, px %g)", who,
                       kMinAny, kMaxAny, kMaxPow2, B, H, W, px);
        return EMD_E_INVALID;
    }
    if (B == 0) return EMD_OK;
    const Layout l = layout(B, H, W, W, true);
    const size_t ne = (size_t)B * H * W;
    const emd::Range r[] = {{workspace, l.bytes, 16, false, false},
                            {psi, ne * (psi_is_real_f32 ? sizeof(float) : sizeof(cplx)), psi_is_real_f32 ? 4u : 16u, false, true},
                            {out, ne * sizeof(cplx), 16, false, false},
                            {defocus, (size_t)B * sizeof(double), 8, false, true}};
    const int rc = emd::check_ranges(who, r, 4, kAligned, &workspace_bytes);
    if (rc != EMD_OK) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    char* ws = static_cast<char*>(workspace);
    LineTab row, col;
    write_all_tables(l, ws, st, &row, &col);
    cplx* T = reinterpret_cast<cplx*>(ws + l.T);
    cplx* U = reinterpret_cast<cplx*>(ws + l.U);
    const long HW = (long)H * W;
    // rows forward -> T [B][kx][y]; columns forward, times Hf, inverse -> U [B][y][kx]; rows inverse -> out
    launch_pass<OP_FWD>(pass_args(psi, psi_is_real_f32 ? 1 : 0, HW, W, T, HW, 1, H, W, row), H, B, st);
    PassArgs c = pass_args(T, 0, HW, H, U, HW, 1, W, H, col);
    c.defocus = defocus;
    c.H = H;
    c.W = W;
    c.o = Optics{wavelength, (double)H * px, (double)W * px, 0.5 * (wavelength * wavelength * wavelength) * cs};
    launch_pass<OP_PROP>(c, W, B, st);
    launch_pass<OP_INV>(pass_args(U, 0, HW, W, reinterpret_cast<cplx*>(out), HW, W, 1, W, row), H, B, st);
    return emd::check_launch(who);
}
