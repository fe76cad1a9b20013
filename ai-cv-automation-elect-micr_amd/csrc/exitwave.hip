// Exit-wave reconstruction from a through-focus series (ewrec_class.py:100-110, :272-380), in double: the Fresnel
// transfer function, the complex 2-D FFT, propagation between two 2-D FFTs, and the iteration that averages the back-propagated
// images into an exit wave, propagates it to every focus and restores the measured amplitudes.  Square images of side s, padded
// side S = s (1 + pad_periods), a power of two, 8..4096.  The 1-D transform is fft_line.hpp's (one line of S complex doubles in
// LDS); the inverse is by conjugation.
//
//   ew_twiddle_kernel      exp(-2 pi i k / S), written into the workspace on every call
//   ew_transfer_kernel     H [n][S][S] for the public transfer_function; the other kernels compute H on the fly and never read it
//   ew_pass_kernel<OP>     a workgroup owns 8 consecutive lines of one image, one after the other: load a contiguous line (complex, or
//                          float32 as the real part; elements >= n_in are zeros that are never read), transform, store n_out elements
//                          with strides of the caller's choice: straight, or TRANSPOSED, where the 8 lines of a workgroup make the
//                          eight 16-byte pieces of every 128-byte run.  OP: FWD; INV; PROP (forward, times H, inverse, without leaving
//                          LDS); MOD (inverse, psi = a b / |b|, forward: the fused reconstruction's row launch); MODC (MOD with the
//                          image b mod N)
//   recon_cols             (a device function) the fused reconstruction's column launch: a workgroup owns one kx; for k = 0..N-1 it
//                          transforms the line of image k, multiplies by H(-df_k) and accumulates in registers; then for every k it
//                          forms E^ H(+df_k) in LDS, transforms back and stores transposed
//   ew_recon_cols_cand_kernel, ew_recon_cols_kernel   recon_cols on grid (S, C) for C candidates, and on grid (S) for one
//   ew_mean_kernel         the composed path's mean
//   ew_modulus_cand_kernel, ew_loss_rows_cand_kernel, ew_loss_resid_cand_kernel, ew_loss_final_kernel, ew_worst_kernel   the modulus
//                          constraint in real space, the loss's two passes and its end, the largest loss of a candidate
//   ew_search_*, ew_section_decide_kernel, ew_plateau_decide_kernel   the defocus search's table and decisions, one workgroup each
//   ew_refine_*            the refinement's state, poll tables and decisions, one workgroup each
//
// There is one reconstruction, of one stack under C defocus tables at once: the candidate is a grid dimension, the
// image of plane b = c N + k is b mod N ("cand" in a name).  emd_exitwave_reconstruct_f64 is C = 1; its two launches
// of an iteration take the instances without the candidate dimension (ew_recon_cols_kernel, MOD), which were measured faster.
// Candidates that have their own images (emd_exitwave_candidate_stacks_f64, the refinement's polls) are C N images
// to the same kernels: b mod (C N) = b, and iteration 0 reads with the candidate stride of the others.  No kernel instance is added.
//
// No floating-point atomics, every sum in a fixed order: bitwise reproducible.  Launches only; the defocuses are read on the device.
#include <cmath>

#include "fft_line.hpp"
#include "stencil_rows.hpp"

namespace {

constexpr int kMinS = 8, kMaxS = 4096, kMaxN = 64, kMaxIter = 1000000;
constexpr int kLines = 8;   // lines per workgroup of ew_pass_kernel: 8 x 16 bytes = one 128-byte run of a transposed store

enum { OP_FWD = 0, OP_INV = 1, OP_PROP = 2, OP_MOD = 3, OP_MODC = 4 };   // MODC: MOD over [C][N] planes, the image is b mod nimg

bool size_ok(int S) { return S >= kMinS && S <= kMaxS && (S & (S - 1)) == 0; }
// the padded side, or 0
int padded_side(int s, int pad) {
    if (s < 1 || pad < 0 || pad > kMaxS) return 0;
    const long S = (long)s * (1 + pad);
    return S <= kMaxS && size_ok((int)S) ? (int)S : 0;
}

struct Optics {
    double lam, span, c4;   // wavelength; S px; 0.5 lam^3 Cs
};

Optics optics(double wavelength, double px, double cs, int S) {
    Optics o;
    o.lam = wavelength;
    o.span = (double)S * px;
    o.c4 = 0.5 * (wavelength * wavelength * wavelength) * cs;
    return o;
}

// H at the unshifted indices (iy, ix): j = i below S / 2, else i - S; q = j / (S px); t = lam df q2 + 0.5 lam^3 Cs q2 q2, every
// operation rounded on its own (as the float64 restatement); H = cospi(t) + i sinpi(t)
__device__ __forceinline__ cplx transfer_h(int iy, int ix, int S, double df, Optics o) {
#pragma clang fp contract(off)
    const int jy = iy < (S >> 1) ? iy : iy - S, jx = ix < (S >> 1) ? ix : ix - S;
    const double qy = (double)jy / o.span, qx = (double)jx / o.span;
    const double q2 = qy * qy + qx * qx;
    const double t = o.lam * df * q2 + o.c4 * q2 * q2;
    double s, c;
    sincospi(t, &s, &c);
    return make_double2(c, s);
}

// a_k from the float32 image: |x|, or sqrt(max(x, 0)) of an intensity
__device__ __forceinline__ double amplitude(float x, int from_intensity) {
    const double v = (double)x;
    return from_intensity ? sqrt(fmax(v, 0.0)) : fabs(v);
}

// psi = a b / |b|; a where |b| = 0 (the reference gives NaN there)
__device__ __forceinline__ cplx restore_amplitude(double a, cplx b) {
    const double m = sqrt(b.x * b.x + b.y * b.y);
    return m > 0.0 ? make_double2(a * b.x / m, a * b.y / m) : make_double2(a, 0.0);
}

__global__ __launch_bounds__(256) void ew_twiddle_kernel(cplx* __restrict__ tw, int S) {
    twiddle_entry(tw, S);
}

// grid (S * S / 256, n)
__global__ __launch_bounds__(256) void ew_transfer_kernel(cplx* __restrict__ H, int S, const double* __restrict__ defocus, Optics o) {
    const long j = (long)blockIdx.x * 256 + threadIdx.x;
    if (j >= (long)S * S) return;
    H[(long)blockIdx.y * S * S + j] = transfer_h((int)(j / S), (int)(j % S), S, defocus[blockIdx.y], o);
}

struct PassArgs {
    const void* src;   // lines of complex doubles, or of float32 (src_real; 2: an intensity, sqrt(max(x, 0)) is loaded)
    long src_batch, src_line;
    int n_in, src_real;
    cplx* dst;         // element i of line l of image b: dst[b dst_batch + l dst_line + i dst_elem], i < n_out
    long dst_batch, dst_line, dst_elem;
    int n_out, nlines, S;
    const cplx* tw;
    const double* defocus;   // PROP: df = sign defocus[b]
    double sign;
    Optics o;
    const float* amp;        // MOD: the image, [B][nlines][S]; MODC: [nimg][nlines][S], image b mod nimg
    int from_intensity;
    int nimg;                // MODC only (it sits in what was the struct's tail padding)
};

// grid (ceil(nlines / 8), B), S * 16 bytes of LDS.  A thread reads and rewrites only the elements tid + 256 u of the line outside
// fft_line, whose first and last statements are barriers: no other barrier is needed between the lines of a workgroup.
template <int OP>
__global__ __launch_bounds__(256) void ew_pass_kernel(PassArgs a) {
    constexpr bool kMod = OP == OP_MOD || OP == OP_MODC;
    extern __shared__ __align__(16) unsigned char smem[];
    cplx* line = reinterpret_cast<cplx*>(smem);
    const int tid = threadIdx.x, S = a.S;
    const long b = blockIdx.y;
    const double inv = 1.0 / (double)S;
    const int l0 = blockIdx.x * kLines, l1 = min(l0 + kLines, a.nlines);
    for (int l = l0; l < l1; ++l) {
        if (a.src_real) {
            const float* p = static_cast<const float*>(a.src) + b * a.src_batch + (long)l * a.src_line;
            for (int i = tid; i < S; i += 256) line[swz(i)] = make_double2(i < a.n_in ? (a.src_real == 2 ? amplitude(p[i], 1) : (double)p[i]) : 0.0, 0.0);
        } else {
            const cplx* p = static_cast<const cplx*>(a.src) + b * a.src_batch + (long)l * a.src_line;
            for (int i = tid; i < S; i += 256) {
                cplx v = i < a.n_in ? p[i] : make_double2(0.0, 0.0);
                if (OP == OP_INV || kMod) v.y = -v.y;
                line[swz(i)] = v;
            }
        }
        fft_line(line, S, a.tw);
        if (OP == OP_PROP) {
            const double df = a.sign * a.defocus[b];
            for (int i = tid; i < S; i += 256) {
                const cplx v = cmul(line[swz(i)], transfer_h(i, l, S, df, a.o));
                line[swz(i)] = make_double2(v.x, -v.y);
            }
            fft_line(line, S, a.tw);
        }
        if (kMod) {
            const float* am = a.amp + ((OP == OP_MODC ? b % a.nimg : b) * a.nlines + l) * S;
            for (int i = tid; i < S; i += 256) {
                const cplx v = line[swz(i)];
                line[swz(i)] = restore_amplitude(amplitude(am[i], a.from_intensity), make_double2(v.x * inv, -v.y * inv));
            }
            fft_line(line, S, a.tw);
        }
        cplx* d = a.dst + b * a.dst_batch + (long)l * a.dst_line;
        for (int i = tid; i < a.n_out; i += 256) {
            cplx v = line[swz(i)];
            if (OP == OP_INV || OP == OP_PROP) v = make_double2(v.x * inv, -v.y * inv);
            d[(long)i * a.dst_elem] = v;
        }
    }
}

// The column launch's work for one stack, S * 16 bytes of LDS; NU = max(S / 256, 1) elements of the line per thread.  Wt: [N][kx][y]
// (the rows' transforms, transposed); G: [N][y][kx] (b_k, inverse-transformed along y only); Eh: [y][kx] (the exit wave, likewise),
// or NULL.
template <int NU>
__device__ __forceinline__ void recon_cols(const cplx* __restrict__ Wt, cplx* __restrict__ G, cplx* __restrict__ Eh, int N, int S,
                                           const cplx* __restrict__ tw, const double* __restrict__ defocus, Optics o) {
    extern __shared__ __align__(16) unsigned char smem[];
    cplx* line = reinterpret_cast<cplx*>(smem);
    const int tid = threadIdx.x, kx = blockIdx.x;
    const double inv = 1.0 / (double)S, n = (double)N;
    cplx acc[NU];
#pragma unroll
    for (int u = 0; u < NU; ++u) acc[u] = make_double2(0.0, 0.0);
    for (int k = 0; k < N; ++k) {   // E^ = sum_k psi^_k H(-df_k), ascending k
        const cplx* src = Wt + ((long)k * S + kx) * S;
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            const int i = tid + 256 * u;
            if (i < S) line[swz(i)] = src[i];
        }
        fft_line(line, S, tw);
        const double df = -defocus[k];
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            const int i = tid + 256 * u;
            if (i < S) acc[u] = cadd(acc[u], cmul(line[swz(i)], transfer_h(i, kx, S, df, o)));
        }
    }
#pragma unroll
    for (int u = 0; u < NU; ++u) acc[u] = make_double2(acc[u].x / n, acc[u].y / n);
    if (Eh) {
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            const int i = tid + 256 * u;
            if (i < S) line[swz(i)] = make_double2(acc[u].x, -acc[u].y);
        }
        fft_line(line, S, tw);
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            const int i = tid + 256 * u;
            if (i < S) {
                const cplx v = line[swz(i)];
                Eh[(long)i * S + kx] = make_double2(v.x * inv, -v.y * inv);
            }
        }
    }
    for (int k = 0; k < N; ++k) {   // b^_k = E^ H(+df_k), back along y
        const double df = defocus[k];
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            const int i = tid + 256 * u;
            if (i < S) {
                const cplx v = cmul(acc[u], transfer_h(i, kx, S, df, o));
                line[swz(i)] = make_double2(v.x, -v.y);
            }
        }
        fft_line(line, S, tw);
        cplx* dst = G + (long)k * S * S + kx;
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

// grid (S): workgroup kx runs recon_cols for the one stack of C = 1.  The candidate form below does the same at C = 1, 0.6 us a
// launch slower (profiles/exitwave_unify.txt); this instance costs three lines.
template <int NU>
__global__ __launch_bounds__(256) void ew_recon_cols_kernel(const cplx* __restrict__ Wt, cplx* __restrict__ G, cplx* __restrict__ Eh, int N,
                                                            int S, const cplx* __restrict__ tw, const double* __restrict__ defocus,
                                                            Optics o) {
    recon_cols<NU>(Wt, G, Eh, N, S, tw, defocus, o);
}

// grid (S, C): workgroup (kx, c) runs recon_cols for candidate c, with defocus_table[c][.], W planes w_stride apart (0: every
// candidate reads the same planes, the images' own transforms in iteration 0), G [C][N][y][kx] and Eh [C][y][kx] (or NULL).
template <int NU>
__global__ __launch_bounds__(256) void ew_recon_cols_cand_kernel(const cplx* __restrict__ Wt, long w_stride, cplx* __restrict__ G,
                                                                 cplx* __restrict__ Eh, int N, int S, const cplx* __restrict__ tw,
                                                                 const double* __restrict__ defocus_table, Optics o) {
    const long c = blockIdx.y, plane = (long)S * S;
    recon_cols<NU>(Wt + c * w_stride, G + c * N * plane, Eh ? Eh + c * plane : nullptr, N, S, tw, defocus_table + c * N, o);
}

// grid (ceil(n / 256)): E[j] = (sum_k P[k][j]) / N, ascending k
__global__ __launch_bounds__(256) void ew_mean_kernel(const cplx* __restrict__ P, int N, long n, cplx* __restrict__ E) {
    const long j = (long)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    cplx s = make_double2(0.0, 0.0);
    for (int k = 0; k < N; ++k) s = cadd(s, P[k * n + j]);
    E[j] = make_double2(s.x / (double)N, s.y / (double)N);
}

// grid (ceil(n / 256), C N): psi = a b / |b| over [C][N] planes, plane b against image b mod N
__global__ __launch_bounds__(256) void ew_modulus_cand_kernel(const cplx* __restrict__ Bw, const float* __restrict__ img, long n, int N,
                                                              int from_intensity, cplx* __restrict__ psi) {
    const long j = (long)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const long e = blockIdx.y * n + j;
    psi[e] = restore_amplitude(amplitude(img[(blockIdx.y % N) * n + j], from_intensity), Bw[e]);
}

#pragma clang fp contract(off)   // the loss: every operation rounds on its own, as in the host restatement

// grid (s, C N), plane b = c N + k of Bw against image k = b mod N: part[b][y] = (sum of the image's row, sum of I = |b|^2 over the row)
__global__ __launch_bounds__(256) void ew_loss_rows_cand_kernel(const cplx* __restrict__ Bw, const float* __restrict__ img, int s, int N,
                                                                double* __restrict__ part) {
    __shared__ double sh[4];
    const long row = (long)blockIdx.y * s + blockIdx.x, irow = (long)(blockIdx.y % N) * s + blockIdx.x;
    double si = 0.0, sI = 0.0;
    for (int i = threadIdx.x; i < s; i += 256) {
        const cplx v = Bw[row * s + i];
        si += (double)img[irow * s + i];
        sI += v.x * v.x + v.y * v.y;
    }
    si = block_sum_thread0(si, sh);
    sI = block_sum_thread0(sI, sh);
    if (threadIdx.x == 0) {
        part[2 * row] = si;
        part[2 * row + 1] = sI;
    }
}

// grid (s, C N): c = mean(image) / mean(I) from the rows' sums, then resid[b][y] = sum over the row of (image - c I)^2
__global__ __launch_bounds__(256) void ew_loss_resid_cand_kernel(const cplx* __restrict__ Bw, const float* __restrict__ img, int s, int N,
                                                                 const double* __restrict__ part, double* __restrict__ resid) {
    __shared__ double sh[256];
    const long b = blockIdx.y, row = b * s + blockIdx.x, irow = (b % N) * s + blockIdx.x;
    const double npx = (double)s * (double)s;
    const double si = block_sum_fixed(part + 2 * b * s, s, 2, sh), sI = block_sum_fixed(part + 2 * b * s + 1, s, 2, sh);
    const double c = (si / npx) / (sI / npx);
    double r = 0.0;
    for (int i = threadIdx.x; i < s; i += 256) {
        const cplx v = Bw[row * s + i];
        const double d = (double)img[irow * s + i] - c * (v.x * v.x + v.y * v.y);
        r += d * d;
    }
    r = block_tree_sum(r, sh);
    if (threadIdx.x == 0) resid[row] = r;
}

// grid (C N)
__global__ __launch_bounds__(256) void ew_loss_final_kernel(const double* __restrict__ resid, int s, double* __restrict__ losses) {
    __shared__ double sh[256];
    const double r = block_sum_fixed(resid + (long)blockIdx.x * s, s, 1, sh);
    if (threadIdx.x == 0) losses[blockIdx.x] = r / ((double)s * (double)s);
}

// grid (1), C <= 64 threads in use: worst[c] = the largest of losses[c][0..N), ascending k; a NaN loss makes it NaN (torch.max)
__global__ __launch_bounds__(64) void ew_worst_kernel(const double* __restrict__ losses, int C, int N, double* __restrict__ worst) {
    const int c = threadIdx.x;
    if (c >= C) return;
    double w = losses[(long)c * N];
    for (int k = 1; k < N; ++k) {
        const double v = losses[(long)c * N + k];
        if (w == w && (v != v || v > w)) w = v;
    }
    worst[c] = w;
}

// ---- the defocus search's decisions: one small workgroup between two reconstructions, nothing is read back ------

enum { ST_LO = 0, ST_HI = 1, ST_BEST_INC = 2, ST_BEST_LOSS = 3, ST_PREV = 4, ST_COUNT = 5 };   // doubles of the search state
enum { SI_STATUS = 0, SI_STEPS = 1, SI_DONE = 2, SI_COUNT = 4 };                               // ints behind them

struct SearchState {
    double d[ST_COUNT];
    int i[SI_COUNT];
};

__device__ __forceinline__ bool finite_d(double v) { return v - v == 0.0; }

// grid (1).  section: seed = (lo, hi); plateau: seed = (incr1, incr2, prev), kept in (lo, hi, prev)
__global__ __launch_bounds__(64) void ew_search_init_kernel(const double* __restrict__ seed, int plateau, SearchState* __restrict__ st) {
    if (threadIdx.x != 0) return;
    st->d[ST_LO] = seed[0];
    st->d[ST_HI] = seed[1];
    st->d[ST_BEST_INC] = __longlong_as_double(0x7FF8000000000000ll);
    st->d[ST_BEST_LOSS] = __longlong_as_double(0x7FF0000000000000ll);
    st->d[ST_PREV] = plateau ? seed[2] : 0.0;
    for (int j = 0; j < SI_COUNT; ++j) st->i[j] = 0;
}

// grid (1), C threads in use: inc_c = lo + c ((hi - lo) / (C - 1)), inc_{C-1} = hi; increments[c] = inc_c; table[c][k] = inc_c ramp[k].
// C == 1 (a plateau step): the midpoint 0.5 (incr1 + incr2), or incr2 itself once the search is done.  C == -1: the result's row
// (the best increment of a section search, incr2 of a plateau search); increments may be NULL.
__global__ __launch_bounds__(64) void ew_search_table_kernel(const SearchState* __restrict__ st, const double* __restrict__ ramp, int C,
                                                             int N, int plateau, double* __restrict__ increments,
                                                             double* __restrict__ table) {
    const int c = threadIdx.x;
    if (c >= (C < 0 ? 1 : C)) return;
    const double lo = st->d[ST_LO], hi = st->d[ST_HI];
    double inc;
    if (C < 0)
        inc = plateau ? hi : st->d[ST_BEST_INC];
    else if (plateau)
        inc = st->i[SI_DONE] ? hi : 0.5 * (lo + hi);
    else
        inc = c == C - 1 ? hi : lo + (double)c * ((hi - lo) / (double)(C - 1));
    if (increments) increments[c] = inc;
    for (int k = 0; k < N; ++k) table[(long)c * N + k] = inc * ramp[k];
}

// grid (1), one thread: the section round's decision from its increments and worst losses [C]
__global__ __launch_bounds__(64) void ew_section_decide_kernel(const double* __restrict__ increments, const double* __restrict__ worst, int C,
                                                               SearchState* __restrict__ st) {
    if (threadIdx.x != 0) return;
    int best = -1;
    for (int c = 0; c < C; ++c)
        if (finite_d(worst[c]) && (best < 0 || worst[c] < worst[best])) best = c;
    if (best < 0) {
        st->i[SI_STATUS] |= EMD_SEARCH_NONFINITE;
        return;
    }
    if (worst[best] < st->d[ST_BEST_LOSS]) {
        st->d[ST_BEST_LOSS] = worst[best];
        st->d[ST_BEST_INC] = increments[best];
    }
    st->d[ST_LO] = increments[best > 0 ? best - 1 : 0];
    st->d[ST_HI] = increments[best < C - 1 ? best + 1 : C - 1];
    st->i[SI_STEPS] += 1;
}

// grid (1), one thread: the plateau step's decision from its increment and loss
__global__ __launch_bounds__(64) void ew_plateau_decide_kernel(const double* __restrict__ increment, const double* __restrict__ loss,
                                                               SearchState* __restrict__ st) {
    if (threadIdx.x != 0 || st->i[SI_DONE]) return;
    const double l = loss[0];
    if (!finite_d(l)) {
        st->i[SI_STATUS] |= EMD_SEARCH_NONFINITE;
        st->i[SI_DONE] = 1;
    } else if (l < st->d[ST_PREV]) {
        st->d[ST_LO] = st->d[ST_HI];
        st->d[ST_HI] = increment[0];
        st->d[ST_PREV] = l;
        st->i[SI_STEPS] += 1;
    } else {
        st->i[SI_DONE] = 1;
    }
}

// grid (1), one thread: result = (increment, loss), status = (status bits, steps)
__global__ __launch_bounds__(64) void ew_search_finish_kernel(const SearchState* __restrict__ st, int plateau, double* __restrict__ result,
                                                              int* __restrict__ status) {
    if (threadIdx.x != 0) return;
    result[0] = plateau ? st->d[ST_HI] : st->d[ST_BEST_INC];
    result[1] = plateau ? st->d[ST_PREV] : st->d[ST_BEST_LOSS];
    status[0] = st->i[SI_STATUS] | (plateau && !st->i[SI_DONE] ? EMD_SEARCH_UNFINISHED : 0);
    status[1] = st->i[SI_STEPS];
}

// ---- the refinement of crop centres and defocuses: a compass search whose polls are the candidates ------------

enum { RF_BEST = 0, RF_LOSS0 = 1, RF_STEP_XY = 2, RF_STEP_DF = 3, RF_COUNT = 4 };   // doubles of the refinement's state
enum { RI_STATUS = 0, RI_MOVES = 1, RI_COUNT = 2 };                                  // ints behind them

struct RefineState {
    double d[RF_COUNT];
    int i[RI_COUNT];
};

// Poll q of the compass search: parameter p = q / 2 = axis (N - 1) + j, the free images j in ascending k without the anchor; the
// entry of the state it moves (centres [N][2] = (x, y), defocus [N]) and its value, the state's plus (q even) or minus (q odd) the
// axis' step, one rounded operation.  The table and the decision both go through here, so the chosen candidate IS the polled one.
__device__ __forceinline__ double refine_poll(int q, int N, int anchor, const RefineState* st, const double* centres, const double* defocus,
                                              int& axis, int& k) {
#pragma clang fp contract(off)
    const int p = q >> 1, j = p % (N - 1);
    axis = p / (N - 1);
    k = j < anchor ? j : j + 1;
    const double v = axis == 2 ? defocus[k] : centres[2 * k + axis];
    const double step = st->d[axis == 2 ? RF_STEP_DF : RF_STEP_XY];
    return (q & 1) ? v - step : v + step;
}

// grid (1): the state starts as the seed
__global__ __launch_bounds__(64) void ew_refine_init_kernel(const double* __restrict__ centres0, const double* __restrict__ defocus0,
                                                            const double* __restrict__ steps0, int N, RefineState* __restrict__ st,
                                                            double* __restrict__ centres, double* __restrict__ defocus) {
    const int t = threadIdx.x;
    if (t < N) {
        centres[2 * t] = centres0[2 * t];
        centres[2 * t + 1] = centres0[2 * t + 1];
        defocus[t] = defocus0[t];
    }
    if (t != 0) return;
    st->d[RF_BEST] = st->d[RF_LOSS0] = __longlong_as_double(0x7FF0000000000000ll);
    st->d[RF_STEP_XY] = steps0[0];
    st->d[RF_STEP_DF] = steps0[1];
    for (int j = 0; j < RI_COUNT; ++j) st->i[j] = 0;
}

// grid (1), n <= 64 threads in use: row c of the tables is the state with poll q0 + c applied; q0 < 0 (n = 1): the state itself.
// steps_out (may be NULL): the steps this round polls with.
__global__ __launch_bounds__(64) void ew_refine_table_kernel(const RefineState* __restrict__ st, const double* __restrict__ centres,
                                                             const double* __restrict__ defocus, int N, int anchor, int q0, int n,
                                                             double* __restrict__ centres_table, double* __restrict__ defocus_table,
                                                             double* __restrict__ steps_out) {
    const int c = threadIdx.x;
    if (c == 0 && steps_out) {
        steps_out[0] = st->d[RF_STEP_XY];
        steps_out[1] = st->d[RF_STEP_DF];
    }
    if (c >= n) return;
    double* tc = centres_table + (long)c * N * 2;
    double* td = defocus_table + (long)c * N;
    for (int k = 0; k < N; ++k) {
        tc[2 * k] = centres[2 * k];
        tc[2 * k + 1] = centres[2 * k + 1];
        td[k] = defocus[k];
    }
    if (q0 < 0) return;
    int axis, k;
    const double v = refine_poll(q0 + c, N, anchor, st, centres, defocus, axis, k);
    if (axis == 2)
        td[k] = v;
    else
        tc[2 * k + axis] = v;
}

// grid (1), one thread: best = loss0 = the seed's worst loss; not finite: best = +inf and EMD_SEARCH_NONFINITE
__global__ __launch_bounds__(64) void ew_refine_seed_kernel(const double* __restrict__ worst, RefineState* __restrict__ st) {
    if (threadIdx.x != 0) return;
    const double l = worst[0];
    st->d[RF_LOSS0] = l;
    if (finite_d(l))
        st->d[RF_BEST] = l;
    else
        st->i[RI_STATUS] |= EMD_SEARCH_NONFINITE;
}

// grid (1), one thread: the round's decision from its Q worst losses
__global__ __launch_bounds__(64) void ew_refine_decide_kernel(const double* __restrict__ worst, int Q, int N, int anchor,
                                                              RefineState* __restrict__ st, double* __restrict__ centres,
                                                              double* __restrict__ defocus, int* __restrict__ choice) {
    if (threadIdx.x != 0) return;
    int best = -1;
    for (int q = 0; q < Q; ++q)
        if (finite_d(worst[q]) && (best < 0 || worst[q] < worst[best])) best = q;
    if (best < 0) {
        st->i[RI_STATUS] |= EMD_SEARCH_NONFINITE;
        choice[0] = -2;
    } else if (worst[best] < st->d[RF_BEST]) {
        int axis, k;
        const double v = refine_poll(best, N, anchor, st, centres, defocus, axis, k);
        if (axis == 2)
            defocus[k] = v;
        else
            centres[2 * k + axis] = v;
        st->d[RF_BEST] = worst[best];
        st->i[RI_MOVES] += 1;
        choice[0] = best;
    } else {
        st->d[RF_STEP_XY] = 0.5 * st->d[RF_STEP_XY];
        st->d[RF_STEP_DF] = 0.5 * st->d[RF_STEP_DF];
        choice[0] = -1;
    }
}

// grid (1): the state and its numbers into the caller's arrays
__global__ __launch_bounds__(64) void ew_refine_finish_kernel(const RefineState* __restrict__ st, const double* __restrict__ centres,
                                                              const double* __restrict__ defocus, int N, double* __restrict__ result_centres,
                                                              double* __restrict__ result_defocus, double* __restrict__ result,
                                                              int* __restrict__ status) {
    const int t = threadIdx.x;
    if (t < N) {
        result_centres[2 * t] = centres[2 * t];
        result_centres[2 * t + 1] = centres[2 * t + 1];
        result_defocus[t] = defocus[t];
    }
    if (t != 0) return;
    result[0] = st->d[RF_BEST];
    result[1] = st->d[RF_LOSS0];
    status[0] = st->i[RI_STATUS];
    status[1] = st->i[RI_MOVES];
}

// ---- host side -----------------------------------------------------------------------------------------------------------

// The entry points' arguments go through emd::check_ranges behind their shape checks.  No range is marked as an input: every overlap
// is refused, two inputs' included.  Complex doubles and the images are checked for 16-byte alignment, arrays of doubles for 8-byte.
using emd::Range;
constexpr const char* kAligned = "the inputs, the outputs and the workspace must be 16-byte aligned (arrays of doubles: 8-byte)";

template <int OP>
void launch_pass(const PassArgs& a, int B, hipStream_t st) {
    hipLaunchKernelGGL(ew_pass_kernel<OP>, dim3((unsigned)emd::tiles_of(a.nlines, kLines), (unsigned)B), dim3(256), (size_t)a.S * sizeof(cplx),
                       st, a);
}

void launch_twiddle(cplx* tw, int S, hipStream_t st) {
    hipLaunchKernelGGL(ew_twiddle_kernel, dim3((unsigned)emd::tiles_of(S, 256)), dim3(256), 0, st, tw, S);
}

PassArgs pass_args(const void* src, int src_real, long src_batch, long src_line, int n_in, cplx* dst, long dst_batch, long dst_line,
                   long dst_elem, int n_out, int nlines, int S, const cplx* tw) {
    PassArgs a{};
    a.src = src;
    a.src_real = src_real;
    a.src_batch = src_batch;
    a.src_line = src_line;
    a.n_in = n_in;
    a.dst = dst;
    a.dst_batch = dst_batch;
    a.dst_line = dst_line;
    a.dst_elem = dst_elem;
    a.n_out = n_out;
    a.nlines = nlines;
    a.S = S;
    a.tw = tw;
    return a;
}

// out[b] = ifft2(fft2(pad(src[b])) H(sign defocus[b]))[:s, :s], three launches.  src: [.][s][s], images src_batch apart (0: one
// wave to every focus); T: [B][S][s] (kx, then the s rows that are not zero); U: [B][s][S] (the s rows that are kept, then kx).
void launch_propagate(const void* src, int src_real, long src_batch, int B, int s, int S, const double* defocus, double sign, Optics o,
                      const cplx* tw, cplx* T, cplx* U, cplx* out, hipStream_t st) {
    launch_pass<OP_FWD>(pass_args(src, src_real, src_batch, s, s, T, (long)S * s, 1, s, S, s, S, tw), B, st);
    PassArgs c = pass_args(T, 0, (long)S * s, s, s, U, (long)s * S, 1, S, s, S, S, tw);
    c.defocus = defocus;
    c.sign = sign;
    c.o = o;
    launch_pass<OP_PROP>(c, B, st);
    launch_pass<OP_INV>(pass_args(U, 0, (long)s * S, S, S, out, (long)s * s, s, 1, s, s, S, tw), B, st);
}

static_assert(kMaxS / 256 <= 16, "the column kernel has an instance for every side up to kMaxS: NU = 16 is the largest");

// one stack (C = 1) on the kernel without the candidate dimension: the same work, measured faster
void launch_recon_cols(const cplx* Wt, long w_stride, cplx* G, cplx* Eh, int C, int N, int S, const cplx* tw, const double* table, Optics o,
                       hipStream_t st) {
    const size_t lds = (size_t)S * sizeof(cplx);
#define EW_COLS(NU)                                                                                                                     \
    if (C == 1)                                                                                                                         \
        hipLaunchKernelGGL(ew_recon_cols_kernel<NU>, dim3((unsigned)S), dim3(256), lds, st, Wt, G, Eh, N, S, tw, table, o);               \
    else                                                                                                                                \
        hipLaunchKernelGGL(ew_recon_cols_cand_kernel<NU>, dim3((unsigned)S, (unsigned)C), dim3(256), lds, st, Wt, w_stride, G, Eh, N, S, \
                           tw, table, o)
    switch (S / 256) {
        case 0:
        case 1: EW_COLS(1); break;
        case 2: EW_COLS(2); break;
        case 4: EW_COLS(4); break;
        case 8: EW_COLS(8); break;
        default: EW_COLS(16); break;
    }
#undef EW_COLS
}

struct PropLayout {
    size_t tw, T, U, bytes;
};

PropLayout prop_layout(int B, int s, int S) {
    PropLayout l{};
    size_t bytes = 0;
    l.tw = bytes;
    bytes += emd::round256((size_t)S * sizeof(cplx));
    l.T = bytes;
    bytes += emd::round256((size_t)B * S * s * sizeof(cplx));
    l.U = bytes;
    bytes += emd::round256((size_t)B * s * S * sizeof(cplx));
    l.bytes = bytes;
    return l;
}

constexpr int kMaxC = 64, kMaxRounds = 1024;

bool batch_ok(int B) { return B >= 0 && B <= 65535; }
bool cand_ok(int C, int N) { return C >= 1 && C <= kMaxC && N >= 1 && N <= kMaxN && (long)C * N <= 65535; }
bool search_ok(int method, int C) {
    return method == EMD_SEARCH_SECTION ? C >= 3 && C <= kMaxC : method == EMD_SEARCH_PLATEAU && C == 1;
}

// The workspace of a reconstruction of one stack under C defocus tables (one stack at its own defocuses is
// C = 1).  Fused (pad_periods == 0): W [C][N] (the rows' transforms, transposed; b_k at the end), G [C][N], Eh [C], the loss's sums
// [C][N].  Composed: psi, P (the propagated stack), the propagation's T and U and the loss's sums for one candidate, since the
// candidates run one after the other; spare_wave: an exit wave for a caller that passes none (the candidates' entry points).
struct ReconLayout {
    bool fused;
    size_t tw, A, Bf, Eh, T, U, part, resid, Ew, bytes;
};

ReconLayout recon_layout(int C, int N, int s, int S, bool spare_wave) {
    ReconLayout l{};
    l.fused = S == s && !emd::g_knobs.exitwave_composed;
    const size_t planes = (size_t)(l.fused ? C : 1) * N;
    size_t bytes = 0;
    l.tw = bytes;
    bytes += emd::round256((size_t)S * sizeof(cplx));
    l.A = bytes;    // fused: W; composed: psi
    bytes += emd::round256(planes * s * s * sizeof(cplx));
    l.Bf = bytes;   // fused: G; composed: P
    bytes += emd::round256(planes * s * s * sizeof(cplx));
    if (l.fused) {
        l.Eh = bytes;
        bytes += emd::round256((size_t)C * S * S * sizeof(cplx));
    } else {
        l.T = bytes;
        bytes += emd::round256((size_t)N * S * s * sizeof(cplx));
        l.U = bytes;
        bytes += emd::round256((size_t)N * s * S * sizeof(cplx));
    }
    l.part = bytes;
    bytes += emd::round256(planes * s * 2 * sizeof(double));
    l.resid = bytes;
    bytes += emd::round256(planes * s * sizeof(double));
    if (!l.fused && spare_wave) {
        l.Ew = bytes;
        bytes += emd::round256((size_t)s * s * sizeof(cplx));
    }
    l.bytes = bytes;
    return l;
}

// the refusals that emd_exitwave_candidates_f64 and emd_exitwave_search_f64 share, with the offending values
bool cand_refused(const char* who, int C, int N, int s, int S, int pad_periods, double px, int iterations) {
    if (!cand_ok(C, N) || !S || !(px > 0.0) || iterations < 1 || iterations > kMaxIter) {
        emd::set_error("%s: bad shape (1..%d candidates, 1..%d images, candidates x images <= 65535, s (1 + pad_periods) a power of two in "
                       "%d..%d, px > 0, 1..%d iterations; got %d candidates of %d x %d x %d, pad_periods %d, %d iterations)", who, kMaxC,
                       kMaxN, kMinS, kMaxS, kMaxIter, C, N, s, s, pad_periods, iterations);
        return true;
    }
    return false;
}

struct ReconArgs {
    const float* images;
    int C, N, s, S;
    const double* table;   // [C][N]
    Optics o;
    int iterations, fi;
    cplx *E, *stack;       // [C][s][s], [C][N][s][s]
    double *losses, *worst;   // [C][N], [C]; any of the four outputs may be NULL (the composed path needs E, or the layout's spare wave)
    int stacks;               // 0: images [N][s][s], one stack under every candidate; 1: [C][N][s][s], candidate c has its own (3.30)
};

// The iterations of the composed reconstruction of one candidate (pad_periods > 0, or the development knob), every one through the
// launches of propagate; b_k of the last iteration stays in P.  l is the composed layout; the twiddle table is already written.
void launch_composed(const ReconArgs& a, const double* defocus, cplx* Ew, char* ws, const ReconLayout& l, hipStream_t st) {
    const int N = a.N, s = a.s, S = a.S;
    const cplx* tw = reinterpret_cast<const cplx*>(ws + l.tw);
    cplx* A = reinterpret_cast<cplx*>(ws + l.A);
    cplx* Bf = reinterpret_cast<cplx*>(ws + l.Bf);
    cplx* T = reinterpret_cast<cplx*>(ws + l.T);
    cplx* U = reinterpret_cast<cplx*>(ws + l.U);
    const long ss = (long)s * s;
    const unsigned tiles = (unsigned)emd::tiles_of((int)ss, 256);
    for (int it = 0; it < a.iterations; ++it) {
        launch_propagate(it == 0 ? static_cast<const void*>(a.images) : A, it == 0 ? (a.fi ? 2 : 1) : 0, ss, N, s, S, defocus, -1.0, a.o, tw, T,
                         U, Bf, st);
        hipLaunchKernelGGL(ew_mean_kernel, dim3(tiles), dim3(256), 0, st, Bf, N, ss, Ew);
        launch_propagate(Ew, 0, 0, N, s, S, defocus, 1.0, a.o, tw, T, U, Bf, st);
        if (it < a.iterations - 1)
            hipLaunchKernelGGL(ew_modulus_cand_kernel, dim3(tiles, (unsigned)N), dim3(256), 0, st, Bf, a.images, ss, N, a.fi, A);
    }
}

// The iterations of the fused reconstruction of all candidates together: 2 iterations launches, + 1 for E, + 1 for b_k of the last
// iteration in real space, [C][N][s][s] over W, which is dead by then, if the stack or the losses are wanted.
void launch_fused(const ReconArgs& a, char* ws, const ReconLayout& l, hipStream_t st) {
    const int C = a.C, N = a.N, S = a.S;
    const long ss = (long)S * S;
    const cplx* tw = reinterpret_cast<const cplx*>(ws + l.tw);
    cplx* A = reinterpret_cast<cplx*>(ws + l.A);
    cplx* Bf = reinterpret_cast<cplx*>(ws + l.Bf);
    cplx* Eh = a.E ? reinterpret_cast<cplx*>(ws + l.Eh) : nullptr;
    // the rows of the images, transformed once into candidate 0's planes: psi_k starts as the image under every candidate, so
    // iteration 0 reads them with candidate stride 0; the first row pass then fills every candidate's planes, these included.
    // Candidate stacks: all C N images are transformed, iteration 0 reads with the candidate stride of every other iteration, and
    // the modulus takes image b mod (C N) = b
    const int nimg = a.stacks ? C * N : N;
    launch_pass<OP_FWD>(pass_args(a.images, a.fi ? 2 : 1, ss, S, S, A, ss, 1, S, S, S, S, tw), nimg, st);
    for (int it = 0; it < a.iterations; ++it) {
        const bool last = it == a.iterations - 1;
        launch_recon_cols(A, it == 0 && !a.stacks ? 0 : (long)N * ss, Bf, last ? Eh : nullptr, C, N, S, tw, a.table, a.o, st);
        if (!last) {
            PassArgs m = pass_args(Bf, 0, ss, S, S, A, ss, 1, S, S, S, S, tw);
            m.amp = a.images;
            m.from_intensity = a.fi;
            m.nimg = nimg;
            if (C == 1)   // b mod N == b: the instance without the division, 0.4 us a launch faster (profiles/exitwave_unify.txt)
                launch_pass<OP_MOD>(m, N, st);
            else
                launch_pass<OP_MODC>(m, C * N, st);
        }
    }
    if (a.E) launch_pass<OP_INV>(pass_args(Eh, 0, ss, S, S, a.E, ss, S, 1, S, S, S, tw), C, st);
    if (a.stack || a.losses) launch_pass<OP_INV>(pass_args(Bf, 0, ss, S, S, A, ss, S, 1, S, S, S, tw), C * N, st);
}

// The one reconstruction path of emd_exitwave_reconstruct_f64 (C = 1, the defocuses as a table of one row),
// emd_exitwave_candidates_f64 and emd_exitwave_search_f64.  Fused: every candidate in the same launches.  Composed: the candidates
// one after the other, with no host work between them.  Then, from b_k of the last iteration, the outputs that are asked for: the
// stack (1 launch), the losses (3) and the worst loss (1).  Candidate stacks: the kernels that take image b mod N get C N images
// on the fused path, and candidate c's own N images on the composed one.
void launch_recon(const ReconArgs& a, char* ws, const ReconLayout& l, hipStream_t st) {
    const int C = a.C, N = a.N, s = a.s;
    const long ss = (long)s * s;
    const int nimg = a.stacks && l.fused ? C * N : N;
    const unsigned tiles = (unsigned)emd::tiles_of((int)ss, 256);
    const cplx* bwave = reinterpret_cast<const cplx*>(ws + (l.fused ? l.A : l.Bf));   // b_k of the last iteration, [step][N][s][s]
    double* part = reinterpret_cast<double*>(ws + l.part);
    double* resid = reinterpret_cast<double*>(ws + l.resid);
    launch_twiddle(reinterpret_cast<cplx*>(ws + l.tw), a.S, st);
    const int step = l.fused ? C : 1;   // candidates per pass of this loop
    for (int c = 0; c < C; c += step) {
        const unsigned B = (unsigned)(step * N);
        ReconArgs ac = a;   // composed, candidate stacks: this candidate's images
        if (a.stacks && !l.fused) ac.images = a.images + (long)c * N * ss;
        const float* img = ac.images;
        if (l.fused)
            launch_fused(a, ws, l, st);
        else
            launch_composed(ac, a.table + (size_t)c * N, a.E ? a.E + c * ss : reinterpret_cast<cplx*>(ws + l.Ew), ws, l, st);
        if (a.stack)
            hipLaunchKernelGGL(ew_modulus_cand_kernel, dim3(tiles, B), dim3(256), 0, st, bwave, img, ss, nimg, a.fi, a.stack + (long)c * N * ss);
        if (a.losses) {
            hipLaunchKernelGGL(ew_loss_rows_cand_kernel, dim3((unsigned)s, B), dim3(256), 0, st, bwave, img, s, nimg, part);
            hipLaunchKernelGGL(ew_loss_resid_cand_kernel, dim3((unsigned)s, B), dim3(256), 0, st, bwave, img, s, nimg, part, resid);
            hipLaunchKernelGGL(ew_loss_final_kernel, dim3(B), dim3(256), 0, st, resid, s, a.losses + (size_t)c * N);
        }
    }
    if (a.worst) hipLaunchKernelGGL(ew_worst_kernel, dim3(1), dim3(64), 0, st, a.losses, C, N, a.worst);
}

// the search's state, its defocus table [C][N], the candidates' losses [C][N], a worst loss for the result's own reconstruction
struct SearchLayout {
    ReconLayout cand;
    size_t state, table, losses, worst, ws, bytes;
};

SearchLayout search_layout(int C, int N, int s, int S) {
    SearchLayout l{};
    l.cand = recon_layout(C, N, s, S, true);
    size_t bytes = 0;
    l.state = bytes;
    bytes += emd::round256(sizeof(SearchState));
    l.table = bytes;
    bytes += emd::round256((size_t)C * N * sizeof(double));
    l.losses = bytes;
    bytes += emd::round256((size_t)C * N * sizeof(double));
    l.worst = bytes;
    bytes += emd::round256(sizeof(double));
    l.ws = bytes;
    l.bytes = bytes + l.cand.bytes;
    return l;
}

}  // namespace

extern "C" int emd_transfer_function_f64(int S, int n, const double* defocus, double wavelength, double px, double cs, double* H,
                                         emd_stream_t stream) {
    if (!size_ok(S) || !batch_ok(n) || !(px > 0.0)) {
        emd::set_error("emd_transfer_function_f64: bad shape (S a power of two in %d..%d, 0..65535 defocuses, px > 0; got S = %d, n = %d)",
                       kMinS, kMaxS, S, n);
        return EMD_E_INVALID;
    }
    if (n == 0) return EMD_OK;
    const Range rg[] = {{H, (size_t)n * S * S * sizeof(cplx), 16}, {defocus, (size_t)n * sizeof(double), 8}};
    const int rc = emd::check_ranges("emd_transfer_function_f64", rg, 2, kAligned);
    if (rc != EMD_OK) return rc;
    hipLaunchKernelGGL(ew_transfer_kernel, dim3((unsigned)emd::tiles_of(S * S, 256), (unsigned)n), dim3(256), 0,
                       static_cast<hipStream_t>(stream), reinterpret_cast<cplx*>(H), S, defocus, optics(wavelength, px, cs, S));
    return emd::check_launch("emd_transfer_function_f64");
}

extern "C" size_t emd_cfft2_workspace_bytes(int B, int S) {
    if (B < 1 || !batch_ok(B) || !size_ok(S)) return 0;
    return emd::round256((size_t)S * sizeof(cplx)) + emd::round256((size_t)B * S * S * sizeof(cplx));
}

extern "C" int emd_cfft2_f64(const double* x, int B, int S, int inverse, double* out, void* workspace, size_t workspace_bytes,
                             emd_stream_t stream) {
    if (!batch_ok(B) || !size_ok(S)) {
        emd::set_error("emd_cfft2_f64: bad shape (batch 0..65535, S a power of two in %d..%d; got %d x %d x %d)", kMinS, kMaxS, B, S, S);
        return EMD_E_INVALID;
    }
    if (B == 0) return EMD_OK;
    const size_t nx = (size_t)B * S * S * sizeof(cplx);
    const Range rg[] = {{workspace, emd_cfft2_workspace_bytes(B, S), 16}, {x, nx, 16}, {out, nx, 16}};
    const int rc = emd::check_ranges("emd_cfft2_f64", rg, 3, kAligned, &workspace_bytes);
    if (rc != EMD_OK) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    cplx* tw = static_cast<cplx*>(workspace);
    cplx* T = reinterpret_cast<cplx*>(static_cast<char*>(workspace) + emd::round256((size_t)S * sizeof(cplx)));
    launch_twiddle(tw, S, st);
    const long SS = (long)S * S;
    // rows, written transposed; then the columns, written transposed again
    const PassArgs r = pass_args(x, 0, SS, S, S, T, SS, 1, S, S, S, S, tw);
    const PassArgs c = pass_args(T, 0, SS, S, S, reinterpret_cast<cplx*>(out), SS, 1, S, S, S, S, tw);
    if (inverse) {
        launch_pass<OP_INV>(r, B, st);
        launch_pass<OP_INV>(c, B, st);
    } else {
        launch_pass<OP_FWD>(r, B, st);
        launch_pass<OP_FWD>(c, B, st);
    }
    return emd::check_launch("emd_cfft2_f64");
}

extern "C" size_t emd_propagate_workspace_bytes(int B, int s, int pad_periods) {
    const int S = padded_side(s, pad_periods);
    if (B < 1 || !batch_ok(B) || !S) return 0;
    return prop_layout(B, s, S).bytes;
}

extern "C" int emd_propagate_f64(const void* psi, int psi_is_real_f32, int B, int s, int pad_periods, const double* defocus,
                                 double wavelength, double px, double cs, double* out, void* workspace, size_t workspace_bytes,
                                 emd_stream_t stream) {
    const int S = padded_side(s, pad_periods);
    if (!batch_ok(B) || !S || !(px > 0.0)) {
        emd::set_error("emd_propagate_f64: bad shape (batch 0..65535, s (1 + pad_periods) a power of two in %d..%d, px > 0; got %d x %d x %d, "
                       "pad_periods %d)", kMinS, kMaxS, B, s, s, pad_periods);
        return EMD_E_INVALID;
    }
    if (B == 0) return EMD_OK;
    const PropLayout l = prop_layout(B, s, S);
    const size_t ne = (size_t)B * s * s;
    const Range rg[] = {{workspace, l.bytes, 16}, {psi, ne * (psi_is_real_f32 ? sizeof(float) : sizeof(cplx)), 16}, {out, ne * sizeof(cplx), 16},
                       {defocus, (size_t)B * sizeof(double), 8}};
    const int rc = emd::check_ranges("emd_propagate_f64", rg, 4, kAligned, &workspace_bytes);
    if (rc != EMD_OK) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    char* ws = static_cast<char*>(workspace);
    cplx* tw = reinterpret_cast<cplx*>(ws + l.tw);
    launch_twiddle(tw, S, st);
    launch_propagate(psi, psi_is_real_f32 ? 1 : 0, (long)s * s, B, s, S, defocus, 1.0, optics(wavelength, px, cs, S), tw,
                     reinterpret_cast<cplx*>(ws + l.T), reinterpret_cast<cplx*>(ws + l.U), reinterpret_cast<cplx*>(out), st);
    return emd::check_launch("emd_propagate_f64");
}

extern "C" size_t emd_exitwave_workspace_bytes(int N, int s, int pad_periods) {
    const int S = padded_side(s, pad_periods);
    if (N < 1 || N > kMaxN || !S) return 0;
    return recon_layout(1, N, s, S, false).bytes;
}

extern "C" int emd_exitwave_reconstruct_f64(const float* images, int N, int s, int pad_periods, const double* defocus, double wavelength,
                                            double px, double cs, int iterations, int flags, double* E, double* stack, double* losses,
                                            void* workspace, size_t workspace_bytes, emd_stream_t stream) {
    const int S = padded_side(s, pad_periods);
    if (N < 1 || N > kMaxN || !S || !(px > 0.0) || iterations < 1 || iterations > kMaxIter) {
        emd::set_error("emd_exitwave_reconstruct_f64: bad shape (1..%d images, s (1 + pad_periods) a power of two in %d..%d, px > 0, "
                       "1..%d iterations; got %d x %d x %d, pad_periods %d, %d iterations)", kMaxN, kMinS, kMaxS, kMaxIter, N, s, s,
                       pad_periods, iterations);
        return EMD_E_INVALID;
    }
    const ReconLayout l = recon_layout(1, N, s, S, false);
    const size_t ne = (size_t)N * s * s;
    const Range rg[] = {{workspace, l.bytes, 16},
                       {images, ne * sizeof(float), 16},
                       {E, (size_t)s * s * sizeof(cplx), 16},
                       {stack, ne * sizeof(cplx), 16, true},
                       {losses, (size_t)N * sizeof(double), 8, true},
                       {defocus, (size_t)N * sizeof(double), 8}};
    const int rc = emd::check_ranges("emd_exitwave_reconstruct_f64", rg, 6, kAligned, &workspace_bytes);
    if (rc != EMD_OK) return rc;
    // one candidate, whose table is the defocuses; E always, no worst loss
    const ReconArgs a{images, 1, N, s, S, defocus, optics(wavelength, px, cs, S), iterations, (flags & EMD_EXITWAVE_FROM_INTENSITY) ? 1 : 0,
                      reinterpret_cast<cplx*>(E), reinterpret_cast<cplx*>(stack), losses, nullptr};
    launch_recon(a, static_cast<char*>(workspace), l, static_cast<hipStream_t>(stream));
    return emd::check_launch("emd_exitwave_reconstruct_f64");
}

extern "C" size_t emd_exitwave_candidates_workspace_bytes(int C, int N, int s, int pad_periods) {
    const int S = padded_side(s, pad_periods);
    if (!cand_ok(C, N) || !S) return 0;
    return recon_layout(C, N, s, S, true).bytes;
}

extern "C" int emd_exitwave_candidates_f64(const float* images, int C, int N, int s, int pad_periods, const double* defocus_table,
                                           double wavelength, double px, double cs, int iterations, int flags, double* losses,
                                           double* worst, double* E, double* stack, void* workspace, size_t workspace_bytes,
                                           emd_stream_t stream) {
    const char* who = "emd_exitwave_candidates_f64";
    const int S = padded_side(s, pad_periods);
    if (cand_refused(who, C, N, s, S, pad_periods, px, iterations)) return EMD_E_INVALID;
    const ReconLayout l = recon_layout(C, N, s, S, true);
    const size_t ne = (size_t)N * s * s, nt = (size_t)C * N * sizeof(double);
    const Range rg[] = {{workspace, l.bytes, 16},
                       {images, ne * sizeof(float), 16},
                       {E, (size_t)C * s * s * sizeof(cplx), 16, true},
                       {stack, C * ne * sizeof(cplx), 16, true},
                       {losses, nt, 8},
                       {worst, (size_t)C * sizeof(double), 8},
                       {defocus_table, nt, 8}};
    const int rc = emd::check_ranges(who, rg, 7, kAligned, &workspace_bytes);
    if (rc != EMD_OK) return rc;
    const ReconArgs a{images, C, N, s, S, defocus_table, optics(wavelength, px, cs, S), iterations,
                      (flags & EMD_EXITWAVE_FROM_INTENSITY) ? 1 : 0, reinterpret_cast<cplx*>(E), reinterpret_cast<cplx*>(stack), losses, worst};
    launch_recon(a, static_cast<char*>(workspace), l, static_cast<hipStream_t>(stream));
    return emd::check_launch(who);
}

extern "C" size_t emd_exitwave_search_workspace_bytes(int method, int C, int N, int s, int pad_periods) {
    const int S = padded_side(s, pad_periods);
    if (!search_ok(method, C) || !cand_ok(C, N) || !S) return 0;
    return search_layout(C, N, s, S).bytes;
}

extern "C" int emd_exitwave_search_f64(const float* images, int N, int s, int pad_periods, const double* ramp, const double* seed,
                                       int method, int C, int rounds, double wavelength, double px, double cs, int iterations, int flags,
                                       double* result, double* history_increments, double* history_losses, int* status, double* E,
                                       void* workspace, size_t workspace_bytes, emd_stream_t stream) {
    const char* who = "emd_exitwave_search_f64";
    const int S = padded_side(s, pad_periods);
    if (!search_ok(method, C) || rounds < 1 || rounds > kMaxRounds) {
        emd::set_error("%s: bad search (method %d = section: 3..%d candidates; method %d = plateau: 1 candidate; 1..%d rounds or steps; got "
                       "method %d, %d candidates, %d rounds)", who, EMD_SEARCH_SECTION, kMaxC, EMD_SEARCH_PLATEAU, kMaxRounds, method, C, rounds);
        return EMD_E_INVALID;
    }
    if (cand_refused(who, C, N, s, S, pad_periods, px, iterations)) return EMD_E_INVALID;
    const SearchLayout l = search_layout(C, N, s, S);
    const int plateau = method == EMD_SEARCH_PLATEAU;
    const size_t nh = (size_t)rounds * C * sizeof(double);
    const Range rg[] = {{workspace, l.bytes, 16},
                        {images, (size_t)N * s * s * sizeof(float), 16},
                        {E, (size_t)s * s * sizeof(cplx), 16, true},
                        {result, 2 * sizeof(double), 8},
                        {history_increments, nh, 8},
                        {history_losses, nh, 8},
                        {status, 2 * sizeof(int), 8},
                        {ramp, (size_t)N * sizeof(double), 8},
                        {seed, (plateau ? 3 : 2) * sizeof(double), 8}};
    const int rc = emd::check_ranges(who, rg, 9, kAligned, &workspace_bytes);
    if (rc != EMD_OK) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    char* ws = static_cast<char*>(workspace);
    SearchState* state = reinterpret_cast<SearchState*>(ws + l.state);
    double* table = reinterpret_cast<double*>(ws + l.table);
    double* losses = reinterpret_cast<double*>(ws + l.losses);
    ReconArgs a{images, C, N, s, S, table, optics(wavelength, px, cs, S), iterations, (flags & EMD_EXITWAVE_FROM_INTENSITY) ? 1 : 0,
                nullptr, nullptr, losses, nullptr};
    hipLaunchKernelGGL(ew_search_init_kernel, dim3(1), dim3(64), 0, st, seed, plateau, state);
    for (int r = 0; r < rounds; ++r) {
        double* inc = history_increments + (size_t)r * C;
        a.worst = history_losses + (size_t)r * C;
        hipLaunchKernelGGL(ew_search_table_kernel, dim3(1), dim3(64), 0, st, state, ramp, C, N, plateau, inc, table);
        launch_recon(a, ws + l.ws, l.cand, st);
        if (plateau)
            hipLaunchKernelGGL(ew_plateau_decide_kernel, dim3(1), dim3(64), 0, st, inc, a.worst, state);
        else
            hipLaunchKernelGGL(ew_section_decide_kernel, dim3(1), dim3(64), 0, st, inc, a.worst, C, state);
    }
    hipLaunchKernelGGL(ew_search_finish_kernel, dim3(1), dim3(64), 0, st, state, plateau, result, status);
    if (E) {   // the exit wave at the result: one more reconstruction, of one candidate
        hipLaunchKernelGGL(ew_search_table_kernel, dim3(1), dim3(64), 0, st, state, ramp, -1, N, plateau, static_cast<double*>(nullptr), table);
        a.C = 1;
        a.E = reinterpret_cast<cplx*>(E);
        a.worst = reinterpret_cast<double*>(ws + l.worst);
        launch_recon(a, ws + l.ws, l.cand, st);
    }
    return emd::check_launch(who);
}

extern "C" size_t emd_exitwave_candidate_stacks_workspace_bytes(int C, int N, int s, int pad_periods) {
    return emd_exitwave_candidates_workspace_bytes(C, N, s, pad_periods);
}

extern "C" int emd_exitwave_candidate_stacks_f64(const float* images, int C, int N, int s, int pad_periods, const double* defocus_table,
                                                 double wavelength, double px, double cs, int iterations, int flags, double* losses,
                                                 double* worst, double* E, double* stack, void* workspace, size_t workspace_bytes,
                                                 emd_stream_t stream) {
    const char* who = "emd_exitwave_candidate_stacks_f64";
    const int S = padded_side(s, pad_periods);
    if (cand_refused(who, C, N, s, S, pad_periods, px, iterations)) return EMD_E_INVALID;
    const ReconLayout l = recon_layout(C, N, s, S, true);
    const size_t ne = (size_t)C * N * s * s, nt = (size_t)C * N * sizeof(double);
    const Range rg[] = {{workspace, l.bytes, 16},
                        {images, ne * sizeof(float), 4},   // a chunk of candidates of a larger array starts at any image
                        {E, (size_t)C * s * s * sizeof(cplx), 16, true},
                        {stack, ne * sizeof(cplx), 16, true},
                        {losses, nt, 8},
                        {worst, (size_t)C * sizeof(double), 8},
                        {defocus_table, nt, 8}};
    const int rc = emd::check_ranges(who, rg, 7, "the outputs and the workspace must be 16-byte aligned, arrays of doubles 8-byte, the images 4-byte",
                                     &workspace_bytes);
    if (rc != EMD_OK) return rc;
    const ReconArgs a{images, C, N, s, S, defocus_table, optics(wavelength, px, cs, S), iterations,
                      (flags & EMD_EXITWAVE_FROM_INTENSITY) ? 1 : 0, reinterpret_cast<cplx*>(E), reinterpret_cast<cplx*>(stack), losses, worst, 1};
    launch_recon(a, static_cast<char*>(workspace), l, static_cast<hipStream_t>(stream));
    return emd::check_launch(who);
}

namespace {

constexpr int kMaxS0 = 4096;   // the side of the frames the crops are cut from (register.hip's limit)

// the refinement's state (RefineState, centres [N][2], defocus [N]), the tables of a chunk (centres [C][N][2], defocus [C][N]), its
// crops [C][N][s][s] float32 and losses [C][N], a worst loss for the seed's and the result's own reconstruction
struct RefineLayout {
    ReconLayout cand;
    size_t state, centres, defocus, ctable, dtable, crops, losses, worst, ws, bytes;
};

RefineLayout refine_layout(int C, int N, int s, int S) {
    RefineLayout l{};
    l.cand = recon_layout(C, N, s, S, true);
    size_t bytes = 0;
    l.state = bytes;
    bytes += emd::round256(sizeof(RefineState));
    l.centres = bytes;
    bytes += emd::round256((size_t)N * 2 * sizeof(double));
    l.defocus = bytes;
    bytes += emd::round256((size_t)N * sizeof(double));
    l.ctable = bytes;
    bytes += emd::round256((size_t)C * N * 2 * sizeof(double));
    l.dtable = bytes;
    bytes += emd::round256((size_t)C * N * sizeof(double));
    l.crops = bytes;
    bytes += emd::round256((size_t)C * N * s * s * sizeof(float));
    l.losses = bytes;
    bytes += emd::round256((size_t)C * N * sizeof(double));
    l.worst = bytes;
    bytes += emd::round256(sizeof(double));
    l.ws = bytes;
    l.bytes = bytes + l.cand.bytes;
    return l;
}

bool refine_ok(int N, int S0, int side, int anchor, int C, int rounds) {
    return N >= 2 && N <= kMaxN && S0 >= 1 && S0 <= kMaxS0 && side >= 1 && side <= S0 && anchor >= 0 && anchor < N && C >= 1 && C <= kMaxC &&
           rounds >= 1 && rounds <= kMaxRounds;
}

}  // namespace

extern "C" size_t emd_exitwave_refine_workspace_bytes(int C, int N, int side, int pad_periods) {
    const int S = padded_side(side, pad_periods);
    if (N < 2 || !cand_ok(C, N) || !S) return 0;
    return refine_layout(C, N, side, S).bytes;
}

extern "C" int emd_exitwave_refine_f64(const float* images, int N, int S0, int side, int pad_periods, float pad_val, const double* centres0,
                                       const double* defocus0, const double* steps0, int anchor, int C, int rounds, double wavelength,
                                       double px, double cs, int iterations, int flags, double* result_centres, double* result_defocus,
                                       double* result, int* status, double* history_losses, int* history_choice, double* history_steps,
                                       double* E, void* workspace, size_t workspace_bytes, emd_stream_t stream) {
    const char* who = "emd_exitwave_refine_f64";
    if (!refine_ok(N, S0, side, anchor, C, rounds)) {
        emd::set_error("%s: bad refinement (2..%d images of side 1..%d, 1 <= side <= S0, 0 <= anchor < images, 1..%d candidates a chunk, "
                       "1..%d rounds; got %d images of side %d, side %d, anchor %d, %d candidates, %d rounds)", who, kMaxN, kMaxS0, kMaxC,
                       kMaxRounds, N, S0, side, anchor, C, rounds);
        return EMD_E_INVALID;
    }
    const int s = side, S = padded_side(s, pad_periods);
    if (cand_refused(who, C, N, s, S, pad_periods, px, iterations)) return EMD_E_INVALID;
    const RefineLayout l = refine_layout(C, N, s, S);
    const int Q = 6 * (N - 1);
    const Range rg[] = {{workspace, l.bytes, 16},
                        {images, (size_t)N * S0 * S0 * sizeof(float), 4},
                        {E, (size_t)s * s * sizeof(cplx), 16, true},
                        {result_centres, (size_t)N * 2 * sizeof(double), 8},
                        {result_defocus, (size_t)N * sizeof(double), 8},
                        {result, 2 * sizeof(double), 8},
                        {status, 2 * sizeof(int), 8},
                        {history_losses, (size_t)rounds * Q * sizeof(double), 8},
                        {history_choice, (size_t)rounds * sizeof(int), 4},
                        {history_steps, (size_t)rounds * 2 * sizeof(double), 8},
                        {centres0, (size_t)N * 2 * sizeof(double), 8},
                        {defocus0, (size_t)N * sizeof(double), 8},
                        {steps0, 2 * sizeof(double), 8}};
    const int rc = emd::check_ranges(who, rg, 13,
                                     "the workspace and E must be 16-byte aligned, arrays of doubles and status 8-byte, the images and "
                                     "history_choice 4-byte", &workspace_bytes);
    if (rc != EMD_OK) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    char* ws = static_cast<char*>(workspace);
    RefineState* state = reinterpret_cast<RefineState*>(ws + l.state);
    double* centres = reinterpret_cast<double*>(ws + l.centres);
    double* defocus = reinterpret_cast<double*>(ws + l.defocus);
    double* ctable = reinterpret_cast<double*>(ws + l.ctable);
    double* dtable = reinterpret_cast<double*>(ws + l.dtable);
    float* crops = reinterpret_cast<float*>(ws + l.crops);
    double* worst1 = reinterpret_cast<double*>(ws + l.worst);
    ReconArgs a{crops, 1, N, s, S, dtable, optics(wavelength, px, cs, S), iterations, (flags & EMD_EXITWAVE_FROM_INTENSITY) ? 1 : 0,
                nullptr, nullptr, reinterpret_cast<double*>(ws + l.losses), worst1, 1};
    // n candidates from poll q0 on (q0 < 0: the state itself): their tables, their crops, their reconstructions
    auto evaluate = [&](int q0, int n, double* steps_out) {
        hipLaunchKernelGGL(ew_refine_table_kernel, dim3(1), dim3(64), 0, st, state, centres, defocus, N, anchor, q0, n, ctable, dtable,
                           steps_out);
        emd::launch_crop_candidates(images, N, S0, ctable, n, s, pad_val, crops, st);
        a.C = n;
        launch_recon(a, ws + l.ws, l.cand, st);
    };
    hipLaunchKernelGGL(ew_refine_init_kernel, dim3(1), dim3(64), 0, st, centres0, defocus0, steps0, N, state, centres, defocus);
    evaluate(-1, 1, nullptr);
    hipLaunchKernelGGL(ew_refine_seed_kernel, dim3(1), dim3(64), 0, st, worst1, state);
    for (int r = 0; r < rounds; ++r) {
        double* hl = history_losses + (size_t)r * Q;
        for (int q0 = 0; q0 < Q; q0 += C) {
            a.worst = hl + q0;
            evaluate(q0, Q - q0 < C ? Q - q0 : C, q0 == 0 ? history_steps + 2 * (size_t)r : nullptr);
        }
        hipLaunchKernelGGL(ew_refine_decide_kernel, dim3(1), dim3(64), 0, st, hl, Q, N, anchor, state, centres, defocus, history_choice + r);
    }
    hipLaunchKernelGGL(ew_refine_finish_kernel, dim3(1), dim3(64), 0, st, state, centres, defocus, N, result_centres, result_defocus, result,
                       status);
    if (E) {   // the exit wave at the result: one more reconstruction, of one candidate, without its losses
        a.E = reinterpret_cast<cplx*>(E);
        a.losses = a.worst = nullptr;
        evaluate(-1, 1, nullptr);
    }
    return emd::check_launch(who);
}
