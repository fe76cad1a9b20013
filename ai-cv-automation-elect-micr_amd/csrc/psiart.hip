// The exit wave and the aberrations of a focal series by gradient descent (psi-art.py; include/emdenoise.h "Exit wave and aberrations
// by gradient descent"), in double: psi = A exp(i P) goes through fft2, the contrast transfer function C_k of every
// image (14 aberration amplitudes, 11 azimuths, the focal-spread envelope, the defocus offset), ifft2 and the modulus; the weighted
// mean-squared distance from the roots of the images is differentiated by a hand-written reverse pass and A, P and the 27 scalars
// take one TF-Adam step.  S a power of two, 8..2048; 1 <= N <= 64.  The 1-D transform is fft_line.hpp's, the inverse by conjugation.
//
//   pa_twiddle_kernel        exp(-2 pi i k / S), written into the workspace on every call
//   pa_ctf_kernel            C [n][S][S] for the public ctf; the other kernels compute C on the fly and never read it
//   pa_rows_kernel<OP>       a workgroup owns 8 consecutive lines of one plane, one after the other (ew_pass_kernel's shape).  PSI: psi
//                            formed on load from A and P, forward, transposed store.  MOD: inverse, b_k stored, the row sums of |b_k|
//                            and of the target r_k.  GB: G_b formed on load from b_k, r_k and the loss's scalars, forward, transposed
//                            store.  GRAD: inverse, dL/dA and dL/dP and (step) Adam on A and P in place
//   pa_fwd_cols_kernel<NU>   one workgroup per frequency of the second axis: the line is transformed once, psi^ and (chi_base / pi, T)
//                            are kept and written to the workspace; for every k, C_k psi^ in LDS, inverse, transposed store
//   pa_loss_kernel, pa_loss_final_kernel   d = c_k |b_k| - r_k: the row sums of d^2 and d |b_k| (and the predictions); loss_k, c_k, L
//   pa_bwd_cols_kernel<NU>   for k ascending: transform the line of F_k, accumulate conj(C_k) F_k and the three sums of
//                            z_k = conj(F_k / n) C_k psi^ in registers; then the inverse of the accumulator, transposed store; then
//                            the 27 basis values once per element and a fixed-order workgroup sum into partial[line][27]
//   pa_scalars_kernel        one workgroup: partial summed over the lines in ascending order, the chain rule of the offset, Adam
//
// A step is these 10 launches, the twiddle table included (6 when only the losses are asked for).  No floating-point atomics, every
// sum in a fixed order: bitwise reproducible.  Launches only; parameters, ramp, weights, rates and the step counter are read on the
// device.
//
// Per-image sub-pixel shifts (the emd_psiart_shift_* entry points): the SHIFT instances of the two column kernels add
// 2 (i' d0_k + j' d1_k) / S to the argument of sincospi (i', j' the signed indices), which multiplies C_k by the linear phase of a
// circular shift of image k by (d0_k, d1_k) pixels.  dL/dd0_k = sum Im z_k 2 pi i' / S and dL/dd1_k = sum Im z_k 2 pi j' / S are sums
// per image: pa_bwd_cols_kernel reduces them over the workgroup inside its loop over k, into partial_shift[line][k][2], and the SHIFT
// instance of pa_scalars_kernel sums the lines and applies Adam with one rate per image.  The instances without SHIFT are what the
// entry points without shifts launch, unchanged.
//
// An all-zero wave under EMD_PSIART_NORMALISE: mean|b_k| = 0, so c_k = mean(r_k) / 0 is inf or NaN, and loss_k, L and the predictions
// are NaN.  Nothing of it reaches the parameters: G_b is 0 where |b_k| = 0, that is everywhere, so every gradient is exactly 0 and a
// step's Adam update sees g = 0 and stays finite.  It is not refused: the wave is on the device.
#include <cmath>

#include "fft_line.hpp"
#include "stencil_rows.hpp"

namespace {

constexpr int kMinS = 8, kMaxS = 2048, kMaxN = 64;
// lines per workgroup of pa_rows_kernel.  They are transformed one after the other, so a transposed store writes single 16-byte
// elements S * 16 bytes apart; the eight lines' elements fill each 128-byte run only over the eight passes, where the L2 merges them
constexpr int kLines = 8;
constexpr int kNP = EMD_PSIART_NPARAM;
constexpr int kA20 = 2, kSpread = 25, kOffset = 26;
constexpr double kPi = 3.14159265358979323846;

enum { R_PSI = 0, R_MOD = 1, R_GB = 2, R_GRAD = 3 };

bool size_ok(int S) { return S >= kMinS && S <= kMaxS && (S & (S - 1)) == 0; }

struct Geom {
    double df, lam;   // 1 / (S sampling), as numpy.fft.fftfreq forms it; the wavelength
    int S;
};

Geom geom(int S, double wavelength, double sampling) {
    Geom g;
    g.df = 1.0 / ((double)S * sampling);
    g.lam = wavelength;
    g.S = S;
    return g;
}

// theta and phi at the unshifted indices: i along the first axis (kx), j along the second (ky)
__device__ __forceinline__ void polar(int i, int j, Geom g, double& th, double& phi) {
    const int h = g.S >> 1;
    const double kx = (double)(i < h ? i : i - g.S) * g.df, ky = (double)(j < h ? j : j - g.S) * g.df;
    th = g.lam * sqrt(kx * kx + ky * ky);
    phi = atan2(ky, kx);
}

// chi_base / pi: every term of get_chi but a20's, (2 / lam) sum_n theta^n / n sum_m a_nm cos(m (phi - phi_nm)).  GRAD: also
// g[p] += w d chi / d p for every coefficient but a20, whose basis function (pi / lam) theta^2 is returned through b20.
template <bool GRAD>
__device__ __forceinline__ double chi_base(const double* __restrict__ par, double th, double phi, double lam, double w, double* g,
                                           double& b20) {
    const double th2 = th * th, th3 = th2 * th, th4 = th2 * th2, th5 = th4 * th, th6 = th3 * th3;
    const double kchi = 2.0 * kPi / lam;
    double sum = 0.0;
#define PA_TERM(ia, ip, n, thn, m)                                        \
    {                                                                     \
        double s, c;                                                      \
        const double r = (thn) / (double)(n), a = par[ia];                \
        if (GRAD) {                                                       \
            sincos((double)(m) * (phi - par[ip]), &s, &c);                \
            g[ia] += w * (kchi * r * c);                                  \
            g[ip] += w * (kchi * r * a * (double)(m) * s);                \
        } else {                                                          \
            c = cos((double)(m) * (phi - par[ip]));                       \
        }                                                                 \
        sum += a * c * r;                                                 \
    }
#define PA_TERM0(ia, n, thn)                     \
    {                                            \
        const double r = (thn) / (double)(n);    \
        if (GRAD) g[ia] += w * (kchi * r);       \
        sum += par[ia] * r;                      \
    }
    PA_TERM(0, 1, 2, th2, 2)
    PA_TERM(3, 4, 3, th3, 3)
    PA_TERM(5, 6, 3, th3, 1)
    PA_TERM(7, 8, 4, th4, 4)
    PA_TERM(9, 10, 4, th4, 2)
    PA_TERM0(11, 4, th4)
    PA_TERM(12, 13, 5, th5, 5)
    PA_TERM(14, 15, 5, th5, 3)
    PA_TERM(16, 17, 5, th5, 1)
    PA_TERM(18, 19, 6, th6, 6)
    PA_TERM(20, 21, 6, th6, 4)
    PA_TERM(22, 23, 6, th6, 2)
    PA_TERM0(24, 6, th6)
#undef PA_TERM
#undef PA_TERM0
    b20 = kchi * (th2 / 2.0);
    return (2.0 / lam) * sum;
}

// T = exp(-sign(D) (0.5 pi / lam D theta^2)^2): exactly 1 at D = 0
__device__ __forceinline__ double envelope(double spread, double th, double lam) {
    const double x = 0.5 * kPi / lam * spread * th * th;
    const double sg = spread > 0.0 ? 1.0 : (spread < 0.0 ? -1.0 : 0.0);
    return exp(-sg * x * x);
}

// off = scale tanh(u / scale) (super_tanh)
__device__ __forceinline__ double offset_of(const double* __restrict__ par, double scale) { return scale * tanh(par[kOffset] / scale); }

// C_k = (cospi(t) - i sinpi(t)) T with t = chi_k / pi = tbase + a20_k theta^2 / lam
__device__ __forceinline__ cplx ctf_of(double tbase, double q, double T, double a20k) {
    double s, c;
    sincospi(tbase + a20k * q, &s, &c);
    return make_double2(c * T, -s * T);
}

// 2 (i' d0 + j' d1) / S with jd1 = j' d1 and two_inv = 2 / S: every operation rounds on its own, so that the forward and the reverse
// kernel form the same bits, and all of it is +-0 when both shifts are 0
__device__ __forceinline__ double shift_term(int i, int S, double d0, double jd1, double two_inv) {
    const double ip = (double)(i < (S >> 1) ? i : i - S);
    return __dmul_rn(__fma_rn(ip, d0, jd1), two_inv);
}

// ctf_of with the shift's term added to t once tbase + a20_k q is formed: with sh = +-0 the bits of ctf_of
__device__ __forceinline__ cplx ctf_shifted(double tbase, double q, double T, double a20k, double sh) {
    double s, c;
    sincospi(__dadd_rn(tbase + a20k * q, sh), &s, &c);
    return make_double2(c * T, -s * T);
}

__device__ __forceinline__ double target_of(float x, int amplitudes) {
    const double v = (double)x;
    return amplitudes ? fabs(v) : sqrt(fmax(v, 0.0));
}

__device__ __forceinline__ double modulus(cplx b) { return sqrt(b.x * b.x + b.y * b.y); }

// lr sqrt(1 - beta2^t) / (1 - beta1^t) without the lr, t the 1-based step of this update
__device__ __forceinline__ double adam_correction(int t, double beta1, double beta2) {
    return sqrt(1.0 - pow(beta2, (double)t)) / (1.0 - pow(beta1, (double)t));
}

__device__ __forceinline__ void adam_update(double* __restrict__ x, double* __restrict__ m, double* __restrict__ v, long e, double g,
                                            double lr_t, double beta1, double beta2, double eps) {
    const double mi = beta1 * m[e] + (1.0 - beta1) * g, vi = beta2 * v[e] + (1.0 - beta2) * g * g;
    m[e] = mi;
    v[e] = vi;
    x[e] = x[e] - lr_t * mi / (sqrt(vi) + eps);
}

struct AdamArgs {
    double *m_amp, *v_amp, *m_phase, *v_phase, *m_par, *v_par;
    int* step;
    const double* rates;   // [29]: A, P, the 27 scalars
    double beta1, beta2, eps;
    int update;
};

__global__ __launch_bounds__(256) void pa_twiddle_kernel(cplx* __restrict__ tw, int S) { twiddle_entry(tw, S); }

// grid (S * S / 256, n)
__global__ __launch_bounds__(256) void pa_ctf_kernel(cplx* __restrict__ C, Geom g, const double* __restrict__ par,
                                                     const double* __restrict__ ramp, double scale) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)g.S * g.S) return;
    double th, phi, b20;
    polar((int)(e / g.S), (int)(e % g.S), g, th, phi);
    const double tb = chi_base<false>(par, th, phi, g.lam, 0.0, nullptr, b20);
    const double a20k = par[kA20] * ramp[blockIdx.y] + offset_of(par, scale);
    C[(long)blockIdx.y * g.S * g.S + e] = ctf_of(tb, th * th / g.lam, envelope(par[kSpread], th, g.lam), a20k);
}

struct RowArgs {
    int S, flags;
    const cplx* tw;
    double *amp, *phase;      // PSI (read), GRAD (read; updated in place by a step)
    const cplx* src;          // MOD, GB, GRAD: planes [B][S][S] of contiguous lines
    cplx* dst;                // PSI, GB: [B][S][S] written transposed; MOD: written straight
    const float* images;      // MOD, GB
    const double* scal;       // GB: [N][4] = c_k, M_k, sum d m, loss_k
    const double* weights;    // GB
    double* part;             // MOD: [B][S][2] = the row sums of |b| and of r
    double *g_amp, *g_phase;  // GRAD, or NULL
    AdamArgs adam;
};

// grid (S / 8, B), S * 16 bytes of LDS.  A thread reads and rewrites only the elements tid + 256 u of the line outside fft_line, whose
// first and last statements are barriers.
template <int OP>
__global__ __launch_bounds__(256) void pa_rows_kernel(RowArgs a) {
    extern __shared__ __align__(16) unsigned char smem[];
    __shared__ double sh[4];
    cplx* line = reinterpret_cast<cplx*>(smem);
    const int tid = threadIdx.x, S = a.S;
    const long b = blockIdx.y, SS = (long)S * S;
    const double inv = 1.0 / (double)S, npx = (double)S * (double)S;
    const int l0 = blockIdx.x * kLines, l1 = min(l0 + kLines, S);
    const int amplitudes = (a.flags & EMD_PSIART_AMPLITUDES) ? 1 : 0;
    double lr_a = 0.0, lr_p = 0.0;
    if (OP == R_GRAD && a.adam.update) {
        const double corr = adam_correction(a.adam.step[0] + 1, a.adam.beta1, a.adam.beta2);
        lr_a = a.adam.rates[0] * corr;
        lr_p = a.adam.rates[1] * corr;
    }
    for (int l = l0; l < l1; ++l) {
        const long row = b * SS + (long)l * S;
        if (OP == R_PSI) {
            for (int i = tid; i < S; i += 256) {
                double s, c;
                const double am = a.amp[row + i];
                sincos(a.phase[row + i], &s, &c);
                line[swz(i)] = make_double2(am * c, am * s);
            }
        } else if (OP == R_GB) {
            const double c = a.scal[4 * b], M = a.scal[4 * b + 1], sdm = a.scal[4 * b + 2];
            const double f = a.weights[b] * (2.0 * c / npx);
            const double shift = (a.flags & EMD_PSIART_NORMALISE) ? sdm / (npx * M) : 0.0;
            for (int i = tid; i < S; i += 256) {
                const cplx v = a.src[row + i];
                const double m = modulus(v);
                const double gm = f * ((c * m - target_of(a.images[row + i], amplitudes)) - shift);
                line[swz(i)] = m > 0.0 ? make_double2(gm * v.x / m, gm * v.y / m) : make_double2(0.0, 0.0);
            }
        } else {
            for (int i = tid; i < S; i += 256) {
                const cplx v = a.src[row + i];
                line[swz(i)] = make_double2(v.x, -v.y);
            }
        }
        fft_line(line, S, a.tw);
        if (OP == R_PSI || OP == R_GB) {
            cplx* d = a.dst + b * SS + l;
            for (int i = tid; i < S; i += 256) d[(long)i * S] = line[swz(i)];
        } else if (OP == R_MOD) {
            double sm = 0.0, sr = 0.0;
            for (int i = tid; i < S; i += 256) {
                const cplx v = line[swz(i)];
                const cplx bk = make_double2(v.x * inv, -v.y * inv);
                a.dst[row + i] = bk;
                sm += modulus(bk);
                sr += target_of(a.images[row + i], amplitudes);
            }
            sm = block_sum_thread0(sm, sh);
            sr = block_sum_thread0(sr, sh);
            if (tid == 0) {
                a.part[2 * (b * S + l)] = sm;
                a.part[2 * (b * S + l) + 1] = sr;
            }
        } else {
            for (int i = tid; i < S; i += 256) {
                const cplx v = line[swz(i)];
                const double gx = v.x * inv, gy = -v.y * inv;
                const long e = row + i;
                double s, c;
                const double am = a.amp[e];
                sincos(a.phase[e], &s, &c);
                const double ga = c * gx + s * gy, gp = am * (c * gy - s * gx);
                if (a.g_amp) a.g_amp[e] = ga;
                if (a.g_phase) a.g_phase[e] = gp;
                if (lr_a != 0.0) adam_update(a.amp, a.adam.m_amp, a.adam.v_amp, e, ga, lr_a, a.adam.beta1, a.adam.beta2, a.adam.eps);
                if (lr_p != 0.0) adam_update(a.phase, a.adam.m_phase, a.adam.v_phase, e, gp, lr_p, a.adam.beta1, a.adam.beta2, a.adam.eps);
            }
        }
    }
}

// grid (S), S * 16 bytes of LDS; NU = max(S / 256, 1) elements of the line per thread.  W: [j][i] (the rows' transforms, transposed);
// PH: [j][i] = psi^; CT: [j][i] = (chi_base / pi, T); G: [N][i][j] (C_k psi^, inverse-transformed along the first axis only).
// SHIFT: shifts [N][2] in pixels, read per image.
template <int NU, bool SHIFT>
__global__ __launch_bounds__(256) void pa_fwd_cols_kernel(const cplx* __restrict__ W, cplx* __restrict__ PH, double2* __restrict__ CT,
                                                          cplx* __restrict__ G, int N, Geom g, const cplx* __restrict__ tw,
                                                          const double* __restrict__ par, const double* __restrict__ ramp, double scale,
                                                          const double* __restrict__ shifts) {
    extern __shared__ __align__(16) unsigned char smem[];
    cplx* line = reinterpret_cast<cplx*>(smem);
    const int tid = threadIdx.x, j = blockIdx.x, S = g.S;
    const double inv = 1.0 / (double)S;
    const long base = (long)j * S;
#pragma unroll
    for (int u = 0; u < NU; ++u) {
        const int i = tid + 256 * u;
        if (i < S) line[swz(i)] = W[base + i];
    }
    fft_line(line, S, tw);
    cplx ph[NU];
    double tb[NU], q[NU], T[NU];
#pragma unroll
    for (int u = 0; u < NU; ++u) {
        const int i = tid + 256 * u;
        if (i < S) {
            double th, phi, b20;
            polar(i, j, g, th, phi);
            ph[u] = line[swz(i)];
            tb[u] = chi_base<false>(par, th, phi, g.lam, 0.0, nullptr, b20);
            q[u] = th * th / g.lam;
            T[u] = envelope(par[kSpread], th, g.lam);
            PH[base + i] = ph[u];
            CT[base + i] = make_double2(tb[u], T[u]);
        }
    }
    const double a20 = par[kA20], off = offset_of(par, scale);
    for (int k = 0; k < N; ++k) {
        const double a20k = a20 * ramp[k] + off;
        double d0 = 0.0, jd1 = 0.0;
        if (SHIFT) {
            d0 = shifts[2 * k];
            jd1 = __dmul_rn((double)(j < (S >> 1) ? j : j - S), shifts[2 * k + 1]);
        }
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            const int i = tid + 256 * u;
            if (i < S) {
                const cplx C = SHIFT ? ctf_shifted(tb[u], q[u], T[u], a20k, shift_term(i, S, d0, jd1, 2.0 * inv))
                                     : ctf_of(tb[u], q[u], T[u], a20k);
                const cplx v = cmul(ph[u], C);
                line[swz(i)] = make_double2(v.x, -v.y);
            }
        }
        fft_line(line, S, tw);
        cplx* dst = G + (long)k * S * S + j;
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

// grid (S, N): c_k from the rows' sums of pa_rows_kernel<MOD>, then part2[k][y] = the row's sums of d^2 and of d m, d = c_k m - r_k;
// pred (or NULL) [N][S][S] = c_k m
__global__ __launch_bounds__(256) void pa_loss_kernel(const cplx* __restrict__ Bw, const float* __restrict__ images, int S, int flags,
                                                      const double* __restrict__ part, double* __restrict__ part2,
                                                      double* __restrict__ pred) {
    __shared__ double sh[256];
    const long k = blockIdx.y, row = (k * S + blockIdx.x) * S;
    const double npx = (double)S * (double)S;
    const double M = block_sum_fixed(part + 2 * k * S, S, 2, sh) / npx, R = block_sum_fixed(part + 2 * k * S + 1, S, 2, sh) / npx;
    const double c = (flags & EMD_PSIART_NORMALISE) ? R / M : 1.0;
    const int amplitudes = (flags & EMD_PSIART_AMPLITUDES) ? 1 : 0;
    double s2 = 0.0, sm = 0.0;
    for (int i = threadIdx.x; i < S; i += 256) {
        const double m = modulus(Bw[row + i]);
        const double p = c * m, d = p - target_of(images[row + i], amplitudes);
        if (pred) pred[row + i] = p;
        s2 += d * d;
        sm += d * m;
    }
    s2 = block_tree_sum(s2, sh);
    sm = block_tree_sum(sm, sh);
    if (threadIdx.x == 0) {
        part2[2 * (k * S + blockIdx.x)] = s2;
        part2[2 * (k * S + blockIdx.x) + 1] = sm;
    }
}

// one workgroup: scal[k] = (c_k, M_k, sum d m, loss_k), losses[k] = loss_k, losses[N] = L = sum_k w_k loss_k in ascending k
__global__ __launch_bounds__(256) void pa_loss_final_kernel(const double* __restrict__ part, const double* __restrict__ part2, int N, int S,
                                                            int flags, const double* __restrict__ weights, double* __restrict__ scal,
                                                            double* __restrict__ losses) {
    __shared__ double sh[256];
    const double npx = (double)S * (double)S;
    double L = 0.0;
    for (int k = 0; k < N; ++k) {
        const long o = 2L * k * S;
        const double M = block_sum_fixed(part + o, S, 2, sh) / npx, R = block_sum_fixed(part + o + 1, S, 2, sh) / npx;
        const double s2 = block_sum_fixed(part2 + o, S, 2, sh), sm = block_sum_fixed(part2 + o + 1, S, 2, sh);
        const double loss = s2 / npx;
        L += weights[k] * loss;
        if (threadIdx.x == 0) {
            scal[4 * k] = (flags & EMD_PSIART_NORMALISE) ? R / M : 1.0;
            scal[4 * k + 1] = M;
            scal[4 * k + 2] = sm;
            scal[4 * k + 3] = loss;
            losses[k] = loss;
        }
    }
    if (threadIdx.x == 0) losses[N] = L;
}

// grid (S), S * 16 bytes of LDS.  Tt: [N][j][i] (the rows' transforms of G_b, transposed); PH, CT as pa_fwd_cols_kernel wrote them;
// U: [i][j] (sum_k conj(C_k) F_k, inverse-transformed along the first axis only); partial: [j][27].  HOLD: psi^ stays in registers
// (NU <= 4); otherwise it is read again for every image.  SHIFT: C_k carries the shift's phase, and for every image the workgroup's
// sums of Im z_k i' and of Im z_k go through wave_sum_lane0 and four LDS slots, so that no register lives across the loop for them;
// partial_shift: [j][N][2] = (2 pi / S) (sum Im z_k i', j' sum Im z_k).
template <int NU, bool HOLD, bool SHIFT>
__global__ __launch_bounds__(256) void pa_bwd_cols_kernel(const cplx* __restrict__ Tt, const cplx* __restrict__ PH,
                                                          const double2* __restrict__ CT, cplx* __restrict__ U, double* __restrict__ partial,
                                                          int N, Geom g, const cplx* __restrict__ tw, const double* __restrict__ par,
                                                          const double* __restrict__ ramp, double scale,
                                                          const double* __restrict__ shifts, double* __restrict__ partial_shift) {
    extern __shared__ __align__(16) unsigned char smem[];
    __shared__ double red[4][kNP];
    __shared__ double sred[SHIFT ? 4 : 1][SHIFT ? kMaxN : 1][2];
    cplx* line = reinterpret_cast<cplx*>(smem);
    const int tid = threadIdx.x, j = blockIdx.x, S = g.S;
    const double inv = 1.0 / (double)S, invn = inv * inv;
    const long base = (long)j * S;
    cplx acc[NU], ph[HOLD ? NU : 1];
    double tb[NU], q[NU], T[NU], s_im[NU], s_ramp[NU], s_re[NU];
#pragma unroll
    for (int u = 0; u < NU; ++u) {
        const int i = tid + 256 * u;
        acc[u] = make_double2(0.0, 0.0);
        s_im[u] = s_ramp[u] = s_re[u] = 0.0;
        tb[u] = q[u] = T[u] = 0.0;
        if (i < S) {
            double th, phi;
            polar(i, j, g, th, phi);
            const double2 ct = CT[base + i];
            tb[u] = ct.x;
            T[u] = ct.y;
            q[u] = th * th / g.lam;
            if (HOLD) ph[u] = PH[base + i];
        }
    }
    const double a20 = par[kA20], off = offset_of(par, scale);
    for (int k = 0; k < N; ++k) {
        const cplx* src = Tt + ((long)k * S + j) * S;
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            const int i = tid + 256 * u;
            if (i < S) line[swz(i)] = src[i];
        }
        fft_line(line, S, tw);
        const double rk = ramp[k], a20k = a20 * rk + off;
        double d0 = 0.0, jd1 = 0.0, sz_i = 0.0, sz = 0.0;
        if (SHIFT) {
            d0 = shifts[2 * k];
            jd1 = __dmul_rn((double)(j < (S >> 1) ? j : j - S), shifts[2 * k + 1]);
        }
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            const int i = tid + 256 * u;
            if (i < S) {
                const cplx F = line[swz(i)];
                const cplx C = SHIFT ? ctf_shifted(tb[u], q[u], T[u], a20k, shift_term(i, S, d0, jd1, 2.0 * inv))
                                     : ctf_of(tb[u], q[u], T[u], a20k);
                const cplx p = HOLD ? ph[u] : PH[base + i];
                acc[u] = cadd(acc[u], cmul(F, make_double2(C.x, -C.y)));
                const cplx y = cmul(C, p);                                          // z = conj(F / n) C psi^
                const double zr = (F.x * y.x + F.y * y.y) * invn, zi = (F.x * y.y - F.y * y.x) * invn;
                s_im[u] += zi;
                s_ramp[u] += rk * zi;
                s_re[u] += zr;
                if (SHIFT) {
                    sz_i += zi * (double)(i < (S >> 1) ? i : i - S);
                    sz += zi;
                }
            }
        }
        if (SHIFT) {
            sz_i = wave_sum_lane0(sz_i);
            sz = wave_sum_lane0(sz);
            if ((tid & 63) == 0) {
                sred[tid >> 6][k][0] = sz_i;
                sred[tid >> 6][k][1] = sz;
            }
        }
    }
    // the transform of the accumulator first: the line is free for it, and the gradient sums below need no LDS of the line's
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
            U[(long)i * S + j] = make_double2(v.x * inv, -v.y * inv);
        }
    }
    double gsum[kNP];
#pragma unroll
    for (int p = 0; p < kNP; ++p) gsum[p] = 0.0;
    const double spread = par[kSpread];
#pragma unroll
    for (int u = 0; u < NU; ++u) {
        const int i = tid + 256 * u;
        if (i < S) {
            double th, phi, b20;
            polar(i, j, g, th, phi);
            chi_base<true>(par, th, phi, g.lam, s_im[u], gsum, b20);
            gsum[kA20] += s_ramp[u] * b20;
            gsum[kOffset] += s_im[u] * b20;
            const double y = 0.5 * kPi * th * th / g.lam;
            gsum[kSpread] += s_re[u] * (-2.0 * fabs(spread) * y * y);
        }
    }
#pragma unroll
    for (int p = 0; p < kNP; ++p) {
        const double v = wave_sum_lane0(gsum[p]);
        if ((tid & 63) == 0) red[tid >> 6][p] = v;
    }
    __syncthreads();
    if (tid < kNP) partial[(long)j * kNP + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
    if (SHIFT && tid < 2 * N) {
        const int k = tid >> 1, c = tid & 1;
        const double s = ((sred[0][k][c] + sred[1][k][c]) + sred[2][k][c]) + sred[3][k][c];
        partial_shift[((long)j * N + k) * 2 + c] = (2.0 * kPi * inv) * (c ? (double)(j < (S >> 1) ? j : j - S) * s : s);
    }
}

struct ShiftArgs {
    const double* partial;   // [S][N][2]
    double *x, *m, *v;       // [N][2]: the shifts and their moments (a step), or NULL
    const double* rates;     // [N], one per image for both axes (a step)
    double* g;               // [N][2] or NULL
    int N;
};

// one workgroup: g[p] = sum over the lines of partial[.][p] in ascending order; d off / d u = sech^2(u / scale); Adam on the scalars
// and the step counter.  SHIFT (256 threads; 64 without): the threads 64 .. 64 + 2 N sum partial_shift over the lines in the same
// order and apply Adam to the shifts with the same step and correction.  They start at the second wave on purpose: both sums are
// chains of S dependent loads, and in one wave the two branches would run one after the other (measured: the step 14-28 % slower).
template <bool SHIFT>
__global__ __launch_bounds__(SHIFT ? 256 : 64) void pa_scalars_kernel(const double* __restrict__ partial, int S, double* __restrict__ par,
                                                                      double scale, double* __restrict__ g_params, AdamArgs ad,
                                                                      ShiftArgs sa) {
    const int p = threadIdx.x;
    const int t = ad.update ? ad.step[0] + 1 : 0;
    if (p < kNP) {
        double g = 0.0;
        for (int l = 0; l < S; ++l) g += partial[(long)l * kNP + p];
        if (p == kOffset) {
            const double th = tanh(par[kOffset] / scale);
            g *= 1.0 - th * th;
        }
        if (g_params) g_params[p] = g;
        if (ad.update) {
            const double lr_t = ad.rates[2 + p] * adam_correction(t, ad.beta1, ad.beta2);
            if (lr_t != 0.0) adam_update(par, ad.m_par, ad.v_par, p, g, lr_t, ad.beta1, ad.beta2, ad.eps);
        }
    }
    if (SHIFT && p >= 64 && p < 64 + 2 * sa.N) {
        const int e = p - 64;
        double g = 0.0;
        for (int l = 0; l < S; ++l) g += sa.partial[(long)l * 2 * sa.N + e];
        if (sa.g) sa.g[e] = g;
        if (ad.update) {
            const double lr_t = sa.rates[e >> 1] * adam_correction(t, ad.beta1, ad.beta2);
            if (lr_t != 0.0) adam_update(sa.x, sa.m, sa.v, e, g, lr_t, ad.beta1, ad.beta2, ad.eps);
        }
    }
    __syncthreads();   // every thread has read the counter
    if (ad.update && p == 0) ad.step[0] = t;
}

// ---- host side -----------------------------------------------------------------------------------------------------------

struct Layout {
    size_t tw, W, PH, CT, G, Bw, part, part2, scal, partial, partial_shift, bytes;
};

// shift: the layout without it, then partial_shift
Layout layout(int N, int S, bool shift = false) {
    Layout l{};
    const size_t plane = emd::round256((size_t)S * S * sizeof(cplx)), stack = emd::round256((size_t)N * S * S * sizeof(cplx));
    size_t bytes = 0;
    l.tw = bytes;
    bytes += emd::round256((size_t)S * sizeof(cplx));
    l.W = bytes;    // the rows' transforms of psi; later U
    bytes += plane;
    l.PH = bytes;
    bytes += plane;
    l.CT = bytes;
    bytes += plane;
    l.G = bytes;    // C_k psi^ back along the first axis; later the rows' transforms of G_b
    bytes += stack;
    l.Bw = bytes;
    bytes += stack;
    l.part = bytes;
    bytes += emd::round256((size_t)N * S * 2 * sizeof(double));
    l.part2 = bytes;
    bytes += emd::round256((size_t)N * S * 2 * sizeof(double));
    l.scal = bytes;
    bytes += emd::round256((size_t)N * 4 * sizeof(double));
    l.partial = bytes;
    bytes += emd::round256((size_t)S * kNP * sizeof(double));
    l.partial_shift = bytes;
    if (shift) bytes += emd::round256((size_t)S * N * 2 * sizeof(double));
    l.bytes = bytes;
    return l;
}

template <int OP>
void launch_rows(const RowArgs& a, int B, hipStream_t st) {
    hipLaunchKernelGGL(pa_rows_kernel<OP>, dim3((unsigned)emd::tiles_of(a.S, kLines), (unsigned)B), dim3(256), (size_t)a.S * sizeof(cplx), st, a);
}

struct Call {
    const float* images;
    int N, S, flags;
    double *amp, *phase, *par;
    const double *ramp, *weights;
    double wavelength, sampling, scale;
    double *losses, *pred, *g_amp, *g_phase, *g_params;
    AdamArgs adam;
    bool shift;              // the SHIFT instances; the fields below are theirs
    double* shifts;          // [N][2], read only without an update
    double *m_shifts, *v_shifts, *g_shifts;
    const double* shift_rates;
};

void run(const Call& c, void* workspace, hipStream_t st) {
    const int N = c.N, S = c.S;
    const Layout l = layout(N, S, c.shift);
    char* ws = static_cast<char*>(workspace);
    cplx* tw = reinterpret_cast<cplx*>(ws + l.tw);
    cplx* W = reinterpret_cast<cplx*>(ws + l.W);
    cplx* PH = reinterpret_cast<cplx*>(ws + l.PH);
    double2* CT = reinterpret_cast<double2*>(ws + l.CT);
    cplx* G = reinterpret_cast<cplx*>(ws + l.G);
    cplx* Bw = reinterpret_cast<cplx*>(ws + l.Bw);
    double* part = reinterpret_cast<double*>(ws + l.part);
    double* part2 = reinterpret_cast<double*>(ws + l.part2);
    double* scal = reinterpret_cast<double*>(ws + l.scal);
    double* partial = reinterpret_cast<double*>(ws + l.partial);
    double* partial_shift = reinterpret_cast<double*>(ws + l.partial_shift);
    const Geom g = geom(S, c.wavelength, c.sampling);
    const size_t lds = (size_t)S * sizeof(cplx);
    hipLaunchKernelGGL(pa_twiddle_kernel, dim3((unsigned)emd::tiles_of(S, 256)), dim3(256), 0, st, tw, S);
    RowArgs r{};
    r.S = S;
    r.flags = c.flags;
    r.tw = tw;
    r.amp = c.amp;
    r.phase = c.phase;
    r.images = c.images;
    r.scal = scal;
    r.weights = c.weights;
    r.part = part;
    r.dst = W;
    launch_rows<R_PSI>(r, 1, st);
#define PA_FWD(NU)                                                                                                                    \
    if (c.shift)                                                                                                                      \
        hipLaunchKernelGGL((pa_fwd_cols_kernel<NU, true>), dim3((unsigned)S), dim3(256), lds, st, W, PH, CT, G, N, g, tw, c.par, c.ramp, \
                           c.scale, c.shifts);                                                                                        \
    else                                                                                                                              \
        hipLaunchKernelGGL((pa_fwd_cols_kernel<NU, false>), dim3((unsigned)S), dim3(256), lds, st, W, PH, CT, G, N, g, tw, c.par, c.ramp, \
                           c.scale, nullptr)
    switch (S / 256) {
        case 0:
        case 1: PA_FWD(1); break;
        case 2: PA_FWD(2); break;
        case 4: PA_FWD(4); break;
        default: PA_FWD(8); break;
    }
#undef PA_FWD
    r.src = G;
    r.dst = Bw;
    launch_rows<R_MOD>(r, N, st);
    hipLaunchKernelGGL(pa_loss_kernel, dim3((unsigned)S, (unsigned)N), dim3(256), 0, st, Bw, c.images, S, c.flags, part, part2, c.pred);
    hipLaunchKernelGGL(pa_loss_final_kernel, dim3(1), dim3(256), 0, st, part, part2, N, S, c.flags, c.weights, scal, c.losses);
    if (!c.adam.update && !c.g_amp && !c.g_phase && !c.g_params && !c.g_shifts) return;
    r.src = Bw;
    r.dst = G;
    launch_rows<R_GB>(r, N, st);
#define PA_BWD(NU, HOLD)                                                                                                              \
    if (c.shift)                                                                                                                      \
        hipLaunchKernelGGL((pa_bwd_cols_kernel<NU, HOLD, true>), dim3((unsigned)S), dim3(256), lds, st, G, PH, CT, W, partial, N, g, tw, \
                           c.par, c.ramp, c.scale, c.shifts, partial_shift);                                                          \
    else                                                                                                                              \
        hipLaunchKernelGGL((pa_bwd_cols_kernel<NU, HOLD, false>), dim3((unsigned)S), dim3(256), lds, st, G, PH, CT, W, partial, N, g, tw, \
                           c.par, c.ramp, c.scale, nullptr, nullptr)
    switch (S / 256) {
        case 0:
        case 1: PA_BWD(1, true); break;
        case 2: PA_BWD(2, true); break;
        case 4: PA_BWD(4, true); break;
        default: PA_BWD(8, false); break;
    }
#undef PA_BWD
    if (c.adam.update || c.g_amp || c.g_phase) {
        r.src = W;
        r.g_amp = c.g_amp;
        r.g_phase = c.g_phase;
        r.adam = c.adam;
        launch_rows<R_GRAD>(r, 1, st);
    }
    if (!c.adam.update && !c.g_params && !c.g_shifts) return;
    if (c.shift) {
        const ShiftArgs sa{partial_shift, c.shifts, c.m_shifts, c.v_shifts, c.shift_rates, c.g_shifts, N};
        hipLaunchKernelGGL(pa_scalars_kernel<true>, dim3(1), dim3(256), 0, st, partial, S, c.par, c.scale, c.g_params, c.adam, sa);
    } else {
        hipLaunchKernelGGL(pa_scalars_kernel<false>, dim3(1), dim3(64), 0, st, partial, S, c.par, c.scale, c.g_params, c.adam, ShiftArgs{});
    }
}

bool shape_ok(const char* who, int N, int S, double wavelength, double sampling, double scale, int flags) {
    if (N < 1 || N > kMaxN || !size_ok(S)) {
        emd::set_error("%s: bad shape (1..%d images, S a power of two in %d..%d: S = 4096 is refused, its column kernels would spill "
                       "registers; got %d x %d x %d)", who, kMaxN, kMinS, kMaxS, N, S, S);
        return false;
    }
    if (!(wavelength > 0.0) || !(sampling > 0.0) || !(scale > 0.0)) {
        emd::set_error("%s: wavelength, sampling and offset_scale must be positive (got %g, %g, %g)", who, wavelength, sampling, scale);
        return false;
    }
    if (flags & ~(EMD_PSIART_NORMALISE | EMD_PSIART_AMPLITUDES)) {
        emd::set_error("%s: unknown flag (%d)", who, flags);
        return false;
    }
    return true;
}

const char* const kAligned = "the workspace must be 16-byte aligned, arrays of doubles 8-byte, the images and the step counter 4-byte";

}  // namespace

extern "C" int emd_psiart_ctf_f64(int S, int n, const double* params, const double* ramp, double wavelength, double sampling,
                                  double offset_scale, double* C, emd_stream_t stream) {
    if (!size_ok(S) || n < 0 || n > 65535) {
        emd::set_error("emd_psiart_ctf_f64: bad shape (S a power of two in %d..%d, 0..65535 functions; got S = %d, n = %d)", kMinS, kMaxS, S, n);
        return EMD_E_INVALID;
    }
    if (n == 0) return EMD_OK;
    if (!shape_ok("emd_psiart_ctf_f64", 1, S, wavelength, sampling, offset_scale, 0)) return EMD_E_INVALID;
    const emd::Range rg[] = {{C, (size_t)n * S * S * sizeof(cplx), 16, false, false},
                             {params, kNP * sizeof(double), 8, false, true},
                             {ramp, (size_t)n * sizeof(double), 8, false, true}};
    const int rc = emd::check_ranges("emd_psiart_ctf_f64", rg, 3, "C must be 16-byte aligned, params and ramp 8-byte");
    if (rc != EMD_OK) return rc;
    hipLaunchKernelGGL(pa_ctf_kernel, dim3((unsigned)emd::tiles_of(S * S, 256), (unsigned)n), dim3(256), 0, static_cast<hipStream_t>(stream),
                       reinterpret_cast<cplx*>(C), geom(S, wavelength, sampling), params, ramp, offset_scale);
    return emd::check_launch("emd_psiart_ctf_f64");
}

extern "C" size_t emd_psiart_workspace_bytes(int N, int S) {
    if (N < 1 || N > kMaxN || !size_ok(S)) return 0;
    return layout(N, S).bytes;
}

extern "C" int emd_psiart_loss_grad_f64(const float* images, int N, int S, const double* amp, const double* phase, const double* params,
                                        const double* ramp, const double* weights, double wavelength, double sampling, double offset_scale,
                                        int flags, double* losses, double* pred, double* g_amp, double* g_phase, double* g_params,
                                        void* workspace, size_t workspace_bytes, emd_stream_t stream) {
    const char* who = "emd_psiart_loss_grad_f64";
    if (!shape_ok(who, N, S, wavelength, sampling, offset_scale, flags)) return EMD_E_INVALID;
    const size_t field = (size_t)S * S * sizeof(double);
    const emd::Range rg[] = {{workspace, layout(N, S).bytes, 16, false, false},
                             {images, (size_t)N * S * S * sizeof(float), 4, false, true},
                             {amp, field, 8, false, true},
                             {phase, field, 8, false, true},
                             {params, kNP * sizeof(double), 8, false, true},
                             {ramp, (size_t)N * sizeof(double), 8, false, true},
                             {weights, (size_t)N * sizeof(double), 8, false, true},
                             {losses, (size_t)(N + 1) * sizeof(double), 8, false, false},
                             {pred, (size_t)N * field, 8, true, false},
                             {g_amp, field, 8, true, false},
                             {g_phase, field, 8, true, false},
                             {g_params, kNP * sizeof(double), 8, true, false}};
    const int rc = emd::check_ranges(who, rg, 12, kAligned, &workspace_bytes);
    if (rc != EMD_OK) return rc;
    Call c{};
    c.images = images;
    c.N = N;
    c.S = S;
    c.flags = flags;
    c.amp = const_cast<double*>(amp);      // read only without an update
    c.phase = const_cast<double*>(phase);
    c.par = const_cast<double*>(params);
    c.ramp = ramp;
    c.weights = weights;
    c.wavelength = wavelength;
    c.sampling = sampling;
    c.scale = offset_scale;
    c.losses = losses;
    c.pred = pred;
    c.g_amp = g_amp;
    c.g_phase = g_phase;
    c.g_params = g_params;
    run(c, workspace, static_cast<hipStream_t>(stream));
    return emd::check_launch(who);
}

extern "C" int emd_psiart_step_f64(const float* images, int N, int S, double* amp, double* phase, double* params, const double* ramp,
                                   const double* weights, double wavelength, double sampling, double offset_scale, int flags, double* m_amp,
                                   double* v_amp, double* m_phase, double* v_phase, double* m_params, double* v_params, int* step,
                                   const double* rates, double beta1, double beta2, double epsilon, double* losses, double* pred,
                                   double* g_amp, double* g_phase, double* g_params, void* workspace, size_t workspace_bytes,
                                   emd_stream_t stream) {
    const char* who = "emd_psiart_step_f64";
    if (!shape_ok(who, N, S, wavelength, sampling, offset_scale, flags)) return EMD_E_INVALID;
    if (!(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && epsilon > 0.0)) {
        emd::set_error("%s: 0 <= beta1, beta2 < 1 and epsilon > 0 (got %g, %g, %g)", who, beta1, beta2, epsilon);
        return EMD_E_INVALID;
    }
    const size_t field = (size_t)S * S * sizeof(double), vec = kNP * sizeof(double);
    const emd::Range rg[] = {{workspace, layout(N, S).bytes, 16, false, false},
                             {images, (size_t)N * S * S * sizeof(float), 4, false, true},
                             {ramp, (size_t)N * sizeof(double), 8, false, true},
                             {weights, (size_t)N * sizeof(double), 8, false, true},
                             {rates, (kNP + 2) * sizeof(double), 8, false, true},
                             {amp, field, 8, false, false},
                             {phase, field, 8, false, false},
                             {params, vec, 8, false, false},
                             {m_amp, field, 8, false, false},
                             {v_amp, field, 8, false, false},
                             {m_phase, field, 8, false, false},
                             {v_phase, field, 8, false, false},
                             {m_params, vec, 8, false, false},
                             {v_params, vec, 8, false, false},
                             {step, sizeof(int), 4, false, false},
                             {losses, (size_t)(N + 1) * sizeof(double), 8, false, false},
                             {pred, (size_t)N * field, 8, true, false},
                             {g_amp, field, 8, true, false},
                             {g_phase, field, 8, true, false},
                             {g_params, vec, 8, true, false}};
    const int rc = emd::check_ranges(who, rg, 20, kAligned, &workspace_bytes);
    if (rc != EMD_OK) return rc;
    Call c{};
    c.images = images;
    c.N = N;
    c.S = S;
    c.flags = flags;
    c.amp = amp;
    c.phase = phase;
    c.par = params;
    c.ramp = ramp;
    c.weights = weights;
    c.wavelength = wavelength;
    c.sampling = sampling;
    c.scale = offset_scale;
    c.losses = losses;
    c.pred = pred;
    c.g_amp = g_amp;
    c.g_phase = g_phase;
    c.g_params = g_params;
    c.adam = AdamArgs{m_amp, v_amp, m_phase, v_phase, m_params, v_params, step, rates, beta1, beta2, epsilon, 1};
    run(c, workspace, static_cast<hipStream_t>(stream));
    return emd::check_launch(who);
}

// ---- with per-image shifts: the same checks, the SHIFT instances -------------------------------------------------------------------

extern "C" size_t emd_psiart_shift_workspace_bytes(int N, int S) {
    if (N < 1 || N > kMaxN || !size_ok(S)) return 0;
    return layout(N, S, true).bytes;
}

extern "C" int emd_psiart_shift_loss_grad_f64(const float* images, int N, int S, const double* amp, const double* phase,
                                              const double* params, const double* shifts, const double* ramp, const double* weights,
                                              double wavelength, double sampling, double offset_scale, int flags, double* losses,
                                              double* pred, double* g_amp, double* g_phase, double* g_params, double* g_shifts,
                                              void* workspace, size_t workspace_bytes, emd_stream_t stream) {
    const char* who = "emd_psiart_shift_loss_grad_f64";
    if (!shape_ok(who, N, S, wavelength, sampling, offset_scale, flags)) return EMD_E_INVALID;
    const size_t field = (size_t)S * S * sizeof(double), pairs = (size_t)N * 2 * sizeof(double);
    const emd::Range rg[] = {{workspace, layout(N, S, true).bytes, 16, false, false},
                             {images, (size_t)N * S * S * sizeof(float), 4, false, true},
                             {amp, field, 8, false, true},
                             {phase, field, 8, false, true},
                             {params, kNP * sizeof(double), 8, false, true},
                             {shifts, pairs, 8, false, true},
                             {ramp, (size_t)N * sizeof(double), 8, false, true},
                             {weights, (size_t)N * sizeof(double), 8, false, true},
                             {losses, (size_t)(N + 1) * sizeof(double), 8, false, false},
                             {pred, (size_t)N * field, 8, true, false},
                             {g_amp, field, 8, true, false},
                             {g_phase, field, 8, true, false},
                             {g_params, kNP * sizeof(double), 8, true, false},
                             {g_shifts, pairs, 8, true, false}};
    const int rc = emd::check_ranges(who, rg, 14, kAligned, &workspace_bytes);
    if (rc != EMD_OK) return rc;
    Call c{};
    c.images = images;
    c.N = N;
    c.S = S;
    c.flags = flags;
    c.amp = const_cast<double*>(amp);      // read only without an update
    c.phase = const_cast<double*>(phase);
    c.par = const_cast<double*>(params);
    c.ramp = ramp;
    c.weights = weights;
    c.wavelength = wavelength;
    c.sampling = sampling;
    c.scale = offset_scale;
    c.losses = losses;
    c.pred = pred;
    c.g_amp = g_amp;
    c.g_phase = g_phase;
    c.g_params = g_params;
    c.shift = true;
    c.shifts = const_cast<double*>(shifts);
    c.g_shifts = g_shifts;
    run(c, workspace, static_cast<hipStream_t>(stream));
    return emd::check_launch(who);
}

extern "C" int emd_psiart_shift_step_f64(const float* images, int N, int S, double* amp, double* phase, double* params, double* shifts,
                                         const double* ramp, const double* weights, double wavelength, double sampling,
                                         double offset_scale, int flags, double* m_amp, double* v_amp, double* m_phase, double* v_phase,
                                         double* m_params, double* v_params, double* m_shifts, double* v_shifts, int* step,
                                         const double* rates, const double* shift_rates, double beta1, double beta2, double epsilon,
                                         double* losses, double* pred, double* g_amp, double* g_phase, double* g_params, double* g_shifts,
                                         void* workspace, size_t workspace_bytes, emd_stream_t stream) {
    const char* who = "emd_psiart_shift_step_f64";
    if (!shape_ok(who, N, S, wavelength, sampling, offset_scale, flags)) return EMD_E_INVALID;
    if (!(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && epsilon > 0.0)) {
        emd::set_error("%s: 0 <= beta1, beta2 < 1 and epsilon > 0 (got %g, %g, %g)", who, beta1, beta2, epsilon);
        return EMD_E_INVALID;
    }
    const size_t field = (size_t)S * S * sizeof(double), vec = kNP * sizeof(double), pairs = (size_t)N * 2 * sizeof(double);
    const emd::Range rg[] = {{workspace, layout(N, S, true).bytes, 16, false, false},
                             {images, (size_t)N * S * S * sizeof(float), 4, false, true},
                             {ramp, (size_t)N * sizeof(double), 8, false, true},
                             {weights, (size_t)N * sizeof(double), 8, false, true},
                             {rates, (kNP + 2) * sizeof(double), 8, false, true},
                             {shift_rates, (size_t)N * sizeof(double), 8, false, true},
                             {amp, field, 8, false, false},
                             {phase, field, 8, false, false},
                             {params, vec, 8, false, false},
                             {shifts, pairs, 8, false, false},
                             {m_amp, field, 8, false, false},
                             {v_amp, field, 8, false, false},
                             {m_phase, field, 8, false, false},
                             {v_phase, field, 8, false, false},
                             {m_params, vec, 8, false, false},
                             {v_params, vec, 8, false, false},
                             {m_shifts, pairs, 8, false, false},
                             {v_shifts, pairs, 8, false, false},
                             {step, sizeof(int), 4, false, false},
                             {losses, (size_t)(N + 1) * sizeof(double), 8, false, false},
                             {pred, (size_t)N * field, 8, true, false},
                             {g_amp, field, 8, true, false},
                             {g_phase, field, 8, true, false},
                             {g_params, vec, 8, true, false},
                             {g_shifts, pairs, 8, true, false}};
    const int rc = emd::check_ranges(who, rg, 25, kAligned, &workspace_bytes);
    if (rc != EMD_OK) return rc;
    Call c{};
    c.images = images;
    c.N = N;
    c.S = S;
    c.flags = flags;
    c.amp = amp;
    c.phase = phase;
    c.par = params;
    c.ramp = ramp;
    c.weights = weights;
    c.wavelength = wavelength;
    c.sampling = sampling;
    c.scale = offset_scale;
    c.losses = losses;
    c.pred = pred;
    c.g_amp = g_amp;
    c.g_phase = g_phase;
    c.g_params = g_params;
    c.adam = AdamArgs{m_amp, v_amp, m_phase, v_phase, m_params, v_params, step, rates, beta1, beta2, epsilon, 1};
    c.shift = true;
    c.shifts = shifts;
    c.m_shifts = m_shifts;
    c.v_shifts = v_shifts;
    c.g_shifts = g_shifts;
    c.shift_rates = shift_rates;
    run(c, workspace, static_cast<hipStream_t>(stream));
    return emd::check_launch(who);
}
