// 2-D orthogonal wavelet transform and wavelet-shrinkage denoising on the device: the "Wavelet" column of the
// reference's comparison table (misc_py/err_hist_maker.py:27), built as skimage.restoration.denoise_wavelet's arithmetic at its
// defaults (BayesShrink, soft threshold, noise estimated from the finest diagonal band).
//
//   emd_wavelet_forward_f32   one launch per level: the input tile plus its half-sample-symmetric halo into LDS, the analysis pair
//                             along H from LDS into LDS, along W from LDS; four bands out, and per-tile double sums of d^2 per band
//   emd_wavelet_inverse_f32   one launch per level: the four bands' tile into LDS (soft-thresholded as it is loaded, when asked to),
//                             synthesis along W from LDS into LDS, along H from LDS
//   emd_filter_wavelet_f32    forward, the noise estimate (exact median of the non-zero |dd_1| by a four-pass radix selection on
//                             integer histograms: counts are order-free, so the result is the same bits on every run), one tiny
//                             launch for the thresholds, inverse with the threshold applied on load
//
// Images are float32 [B,H,W]; every image on its own; grid (tiles, B); a lane is an output column, a wave owns a strip of rows.
// No float atomics.
#include <cfloat>
#include <climits>
#include <cmath>

#include "radix_select.hpp"
#include "stencil_rows.hpp"

namespace {

constexpr int kTW = 64;          // tile columns = lanes of a wave
constexpr int kWaves = 4;
constexpr int kMaxTaps = 8;
constexpr int kMaxLevels = 15;   // H, W <= 32768
constexpr int kMaxExtent = 32768;
constexpr int kATH = 16;         // analysis: output rows per tile (a wave: 4)
constexpr int kSTH = 32;         // synthesis: output rows per tile (a wave: 8)
constexpr int kSelChunk = 4096;  // selection: coefficients per workgroup and pass
constexpr double kMadToSigma = 0.6744897501960817;   // the 75 % quantile of the standard normal

struct WTaps {
    float dec_lo[kMaxTaps], dec_hi[kMaxTaps], rec_lo[kMaxTaps], rec_hi[kMaxTaps];
};

// Half-sample symmetric extension (pywt's "symmetric"): ... x1 x0 | x0 x1 ... x[N-1] | x[N-1] x[N-2] ..., period 2N.  Any i.
__device__ __forceinline__ int sym_index(int i, int N) {
    int m = i % (2 * N);
    if (m < 0) m += 2 * N;
    return m < N ? m : 2 * N - 1 - m;
}

// The input rows r0 .. r0 + IR - 1 and columns c0 .. c0 + IC - 1 of one image (row stride W) into xs (row stride IC), positions
// outside the image by the half-sample symmetric extension: every address read lies inside the image.
__device__ __forceinline__ void load_tile_symmetric(float* __restrict__ xs, const float* __restrict__ xb, int H, int W, int r0, int c0,
                                                    int IR, int IC) {
    for (int i = threadIdx.x; i < IR * IC; i += 256) {
        const int r = i / IC, c = i - r * IC;
        xs[i] = xb[(long)sym_index(r0 + r, H) * W + sym_index(c0 + c, W)];
    }
}

// a * b + c with the product rounded on its own.  Where the symmetric border pairs a sample with its own mirror image, Haar's high
// pass is h x - h x: two rounded products cancel exactly, a fused multiply-add would leave the product's rounding error.  The noise
// estimate drops exact zeros (as skimage does), so those coefficients must be exact zeros here as they are on the host.
__device__ __forceinline__ float mul_add(float a, float b, float c) {
#pragma clang fp contract(off)
    const float p = a * b;
    return p + c;
}

// ---- analysis: one level; grid (tiles, B) ---------------------------------------------------------------------------------
// x [B] images of H x W (image stride xstride) -> ca (image stride castride) and the bands ad, da, dd of nH x nW each, contiguous
// from det (image stride dstride).  c[i] = sum_k dec[k] x~[2i + 1 - k], along H first, then along W.
// part (optional): part[(b * 3 + band) * tiles + tile] = the tile's sum of d^2 in double, lanes then waves in a fixed order.
template <int L>
__global__ __launch_bounds__(256) void wavelet_analysis_kernel(const float* __restrict__ x, long xstride, int H, int W,
                                                               float* __restrict__ ca, long castride, float* __restrict__ det,
                                                               long dstride, int nH, int nW, int tiles_x, WTaps taps,
                                                               double* __restrict__ part) {
    constexpr int TH = kATH, RW = TH / kWaves, IR = 2 * TH + L - 2, IC = 2 * kTW + L - 2;
    __shared__ float xs[IR * IC];
    __shared__ float tl[TH * IC];
    __shared__ float th[TH * IC];
    __shared__ double sh[3][kWaves];
    const int tile = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r0 = (tile / tiles_x) * TH, c0 = (tile % tiles_x) * kTW;
    const long b = blockIdx.y;
    // output row r0 + o reads the input rows 2 (r0 + o) + 1 - k: the tile's first input row is 2 r0 - L + 2
    load_tile_symmetric(xs, x + b * xstride, H, W, 2 * r0 - L + 2, 2 * c0 - L + 2, IR, IC);
    __syncthreads();
#pragma unroll
    for (int q = 0; q < RW; ++q) {
        const int o = wave * RW + q;
        for (int c = lane; c < IC; c += 64) {
            float lo = 0.f, hi = 0.f;
#pragma unroll
            for (int k = 0; k < L; ++k) {
                const float v = xs[(2 * o + L - 1 - k) * IC + c];
                lo = mul_add(taps.dec_lo[k], v, lo);
                hi = mul_add(taps.dec_hi[k], v, hi);
            }
            tl[o * IC + c] = lo;
            th[o * IC + c] = hi;
        }
    }
    __syncthreads();
    double s_ad = 0.0, s_da = 0.0, s_dd = 0.0;
    const int gc = c0 + lane;
    const long plane = (long)nH * nW;
    float* cab = ca + b * castride;
    float* db = det + b * dstride;
#pragma unroll
    for (int q = 0; q < RW; ++q) {
        const int o = wave * RW + q, gr = r0 + o;
        float a = 0.f, ad = 0.f, da = 0.f, dd = 0.f;
#pragma unroll
        for (int k = 0; k < L; ++k) {
            const float vl = tl[o * IC + 2 * lane + L - 1 - k], vh = th[o * IC + 2 * lane + L - 1 - k];
            a = mul_add(taps.dec_lo[k], vl, a);
            ad = mul_add(taps.dec_hi[k], vl, ad);
            da = mul_add(taps.dec_lo[k], vh, da);
            dd = mul_add(taps.dec_hi[k], vh, dd);
        }
        if (gr < nH && gc < nW) {
            const long i = (long)gr * nW + gc;
            cab[i] = a;
            db[i] = ad;
            db[plane + i] = da;
            db[2 * plane + i] = dd;
            s_ad += (double)ad * (double)ad;
            s_da += (double)da * (double)da;
            s_dd += (double)dd * (double)dd;
        }
    }
    if (part) {
        s_ad = wave_sum_lane0(s_ad);
        s_da = wave_sum_lane0(s_da);
        s_dd = wave_sum_lane0(s_dd);
        if (lane == 0) {
            sh[0][wave] = s_ad;
            sh[1][wave] = s_da;
            sh[2][wave] = s_dd;
        }
        __syncthreads();
        if (threadIdx.x < 3) {
            const double* s = sh[threadIdx.x];
            part[(b * 3 + threadIdx.x) * gridDim.x + tile] = ((s[0] + s[1]) + s[2]) + s[3];
        }
    }
}

// ---- synthesis: one level; grid (tiles, B) --------------------------------------------------------------------------------
// ca (image stride castride) and the bands from det, nH x nW each -> out, oH x oW (oH <= 2 nH - L + 2, oW <= 2 nW - L + 2: the
// crop).  x[j] = sum_i a[i] rec_lo[j + L - 2 - 2i] + d[i] rec_hi[j + L - 2 - 2i]: for j = 2 jh + p the L/2 terms
// i = jh + L/2 - 1 - m with tap p + 2m.  Along W first, then along H.
// thr (optional): thr[b * thr_stride + band] = the soft threshold of image b's band (ad, da, dd), applied as the tile is loaded.
template <int L>
__global__ __launch_bounds__(256) void wavelet_synthesis_kernel(const float* __restrict__ ca, long castride,
                                                                const float* __restrict__ det, long dstride, int nH, int nW,
                                                                float* __restrict__ out, long ostride, int oH, int oW, int tiles_x,
                                                                WTaps taps, const float* __restrict__ thr, int thr_stride) {
    constexpr int TH = kSTH, RW = TH / kWaves, HL = L / 2, CR = TH / 2 + HL - 1, CC = kTW / 2 + HL - 1;
    __shared__ float cs[4][CR * CC];
    __shared__ float tl[CR * kTW];
    __shared__ float th[CR * kTW];
    const int tile = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r0 = (tile / tiles_x) * TH, c0 = (tile % tiles_x) * kTW;
    const long b = blockIdx.y;
    const long plane = (long)nH * nW;
    const float* cab = ca + b * castride;
    const float* db = det + b * dstride;
    float t0 = 0.f, t1 = 0.f, t2 = 0.f;
    if (thr) {
        t0 = thr[b * thr_stride];
        t1 = thr[b * thr_stride + 1];
        t2 = thr[b * thr_stride + 2];
    }
    auto soft = [](float d, float t) { return copysignf(fmaxf(fabsf(d) - t, 0.f), d); };
    for (int i = threadIdx.x; i < CR * CC; i += 256) {
        const int r = i / CC, c = i - r * CC;
        const int gi = r0 / 2 + r, gj = c0 / 2 + c;
        float a = 0.f, ad = 0.f, da = 0.f, dd = 0.f;
        if (gi < nH && gj < nW) {
            const long g = (long)gi * nW + gj;
            a = cab[g];
            ad = soft(db[g], t0);
            da = soft(db[plane + g], t1);
            dd = soft(db[2 * plane + g], t2);
        }
        cs[0][i] = a;
        cs[1][i] = ad;
        cs[2][i] = da;
        cs[3][i] = dd;
    }
    const int p = lane & 1, jh = lane >> 1;
    float rlo[HL], rhi[HL];
#pragma unroll
    for (int m = 0; m < HL; ++m) {
        rlo[m] = p ? taps.rec_lo[2 * m + 1] : taps.rec_lo[2 * m];
        rhi[m] = p ? taps.rec_hi[2 * m + 1] : taps.rec_hi[2 * m];
    }
    __syncthreads();
    for (int r = wave; r < CR; r += kWaves) {
        float lo = 0.f, hi = 0.f;
#pragma unroll
        for (int m = 0; m < HL; ++m) {
            const int i = r * CC + jh + HL - 1 - m;
            lo = fmaf(cs[0][i], rlo[m], lo);
            lo = fmaf(cs[1][i], rhi[m], lo);
            hi = fmaf(cs[2][i], rlo[m], hi);
            hi = fmaf(cs[3][i], rhi[m], hi);
        }
        tl[r * kTW + lane] = lo;
        th[r * kTW + lane] = hi;
    }
    __syncthreads();
    const int gc = c0 + lane;
    float* ob = out + b * ostride;
#pragma unroll
    for (int q = 0; q < RW; ++q) {
        const int ro = wave * RW + q, gr = r0 + ro, ih = ro >> 1;   // r0 and wave * RW are even: the row's parity is q's
        float v = 0.f;
#pragma unroll
        for (int m = 0; m < HL; ++m) {
            const int i = (ih + HL - 1 - m) * kTW + lane;
            v = fmaf(tl[i], taps.rec_lo[(q & 1) + 2 * m], v);
            v = fmaf(th[i], taps.rec_hi[(q & 1) + 2 * m], v);
        }
        if (gr < oH && gc < oW) ob[(long)gr * oW + gc] = v;
    }
}

// ---- the noise estimate: exact median of the non-zero |d| by radix selection (radix_select.hpp) ------------------------------
// The key is |d|'s bit pattern, and the exact zeros are left out (as skimage drops them): the count is what pass 0 counted.  Pass
// q > 0 resolves pass q - 1 at the head of every workgroup; the threshold kernel resolves pass 3.
// grid (chunks, B): one pass over d[b * stride + 0 .. n - 1]
__global__ __launch_bounds__(256) void wavelet_select_kernel(const float* __restrict__ d, long stride, long n, unsigned* __restrict__ hist,
                                                             unsigned* __restrict__ state, int pass) {
    __shared__ unsigned h[2][256];
    __shared__ unsigned sc[2][256];
    __shared__ unsigned st[kStateWords];
    const int tid = threadIdx.x;
    const long b = blockIdx.y;
    unsigned* hb = hist + select_hist_at(b, pass);
    unsigned* sb = state + select_state_at(b, pass);
    h[0][tid] = 0;
    h[1][tid] = 0;
    unsigned prefix0 = 0, prefix1 = 0;
    if (pass > 0) {
        select_resolve(hb - kSelHistWords, sb - kStateWords, pass - 1, sc, st);
        if (blockIdx.x == 0 && tid < kStateWords) sb[tid] = st[tid];
        prefix0 = st[0];
        prefix1 = st[1];
    } else {
        __syncthreads();
    }
    const long begin = (long)blockIdx.x * kSelChunk, end = begin + kSelChunk < n ? begin + kSelChunk : n;
    const float* db = d + b * stride;
    for (long i = begin + tid; i < end; i += 256) {
        const unsigned key = magnitude_key(db[i]);
        if (key == 0) continue;   // +0 and -0: skimage drops the exact zeros
        if (pass == 0)
            select_count_first(h, key);
        else
            select_count(h, key, pass, prefix0, prefix1);
    }
    __syncthreads();
    select_flush<2>(h, hb);
}

// ---- sigma and the thresholds: grid (B) -----------------------------------------------------------------------------------
struct LevelSums {
    int levels;
    int tiles[kMaxLevels];    // [l - 1]: tiles of level l's analysis launch
    long off[kMaxLevels];     // part + off: level l's sums, [B][3][tiles]
    double count[kMaxLevels]; // coefficients per band
};
// method 0 (BayesShrink): t = var / sqrt(max(mean(d^2) - var, FLT_EPSILON)) per band; 1 (VisuShrink): t = sigma * visu for all.
// sigma < 0: the selection's result, median / 0.6745 (0 when every coefficient is 0).  thr: [B][levels][3].
__global__ __launch_bounds__(256) void wavelet_threshold_kernel(LevelSums ls, const double* __restrict__ part,
                                                                const unsigned* __restrict__ hist, const unsigned* __restrict__ state,
                                                                float sigma, int method, double visu, float* __restrict__ sigma_used,
                                                                float* __restrict__ thr) {
    __shared__ double sh[256];
    __shared__ unsigned sc[2][256];
    __shared__ unsigned st[kStateWords];
    const long b = blockIdx.x;
    if (sigma < 0.f) {
        select_resolve(hist + select_hist_at(b, 3), state + select_state_at(b, 3), 3, sc, st);
        const float med = (__uint_as_float(st[0]) + __uint_as_float(st[1])) * 0.5f;   // nothing counted: the keys are 0, +0.0f
        sigma = (float)((double)med / kMadToSigma);
    }
    if (sigma_used && threadIdx.x == 0) sigma_used[b] = sigma;
    const double var = (double)sigma * (double)sigma;
    for (int l = 0; l < ls.levels; ++l) {
        for (int band = 0; band < 3; ++band) {
            double t = (double)sigma * visu;
            if (method == 0) {
                const double mean = block_sum_fixed(part + ls.off[l] + (b * 3 + band) * ls.tiles[l], ls.tiles[l], 1, sh) / ls.count[l];
                t = var / sqrt(fmax(mean - var, (double)FLT_EPSILON));
            }
            if (threadIdx.x == 0) thr[(b * ls.levels + l) * 3 + band] = (float)t;
        }
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------------

bool taps_ok(int ntaps) { return ntaps >= 2 && ntaps <= kMaxTaps && ntaps % 2 == 0; }

// floor(log2(min(H, W) / (L - 1))): the largest k with (L - 1) 2^k <= min(H, W); < 1: no level fits
int max_levels(int H, int W, int L) {
    const long m = H < W ? H : W;
    int k = -1;
    while (((long)(L - 1) << (k + 1)) <= m) ++k;
    return k;
}

// Everything a call needs to know about where things lie.  Pyramid of one image (floats): cA_n, then ad, da, dd of level n, of
// level n - 1, ..., of level 1.  Workspace: the approximations of the levels below n for the whole batch, then the per-tile
// sums; the denoiser's adds the pyramids, the thresholds and the selection's histograms and states.
struct Geometry {
    int levels, nH[kMaxLevels + 1], nW[kMaxLevels + 1];   // [0]: the image
    long det[kMaxLevels + 1];                             // [l]: offset of level l's ad in an image's pyramid
    long pyramid;                                         // floats per image
    size_t scratch[kMaxLevels + 1];                       // [l], 1 <= l < levels: byte offset of the batch's cA_l, [B][nH][nW]
    size_t part[kMaxLevels + 1];                          // [l]: byte offset of level l's sums
    size_t transform_bytes;
    size_t pyr_off, thr_off, hist_off, state_off, filter_bytes;
};

bool shape_ok(int B, int H, int W) { return B >= 0 && B <= 65535 && H >= 1 && W >= 1 && H <= kMaxExtent && W <= kMaxExtent; }

// false: refused (the caller says why)
bool geometry(int B, int H, int W, int L, int levels, Geometry* g) {
    if (!shape_ok(B, H, W) || !taps_ok(L) || levels < 1 || levels > max_levels(H, W, L) || levels > kMaxLevels) return false;
    g->levels = levels;
    g->nH[0] = H;
    g->nW[0] = W;
    for (int l = 1; l <= levels; ++l) {
        g->nH[l] = (g->nH[l - 1] + L - 1) / 2;
        g->nW[l] = (g->nW[l - 1] + L - 1) / 2;
    }
    long off = (long)g->nH[levels] * g->nW[levels];
    for (int l = levels; l >= 1; --l) {
        g->det[l] = off;
        off += 3L * g->nH[l] * g->nW[l];
    }
    g->pyramid = off;
    size_t bytes = 0;
    for (int l = 1; l < levels; ++l) {
        g->scratch[l] = bytes;
        bytes += emd::round256((size_t)B * g->nH[l] * g->nW[l] * sizeof(float));
    }
    for (int l = 1; l <= levels; ++l) {
        g->part[l] = bytes;
        bytes += emd::round256((size_t)B * 3 * emd::tiles_of(g->nH[l], kATH) * emd::tiles_of(g->nW[l], kTW) * sizeof(double));
    }
    g->transform_bytes = bytes;
    g->pyr_off = bytes;
    bytes += emd::round256((size_t)B * g->pyramid * sizeof(float));
    g->thr_off = bytes;
    bytes += emd::round256((size_t)B * levels * 3 * sizeof(float));
    g->hist_off = bytes;
    bytes += select_hist_bytes(B);
    g->state_off = bytes;
    bytes += select_state_bytes(B);
    g->filter_bytes = bytes;
    return true;
}

// dec_lo[k] = rec_lo[L-1-k]; dec_hi[k] = (-1)^(k+1) rec_lo[k]; rec_hi[k] = dec_hi[L-1-k]; each rounded to float32 once
WTaps make_taps(const double* rec_lo, int L) {
    WTaps t{};
    for (int k = 0; k < L; ++k) {
        t.rec_lo[k] = (float)rec_lo[k];
        t.dec_lo[k] = (float)rec_lo[L - 1 - k];
        t.dec_hi[k] = (float)((k % 2) ? rec_lo[k] : -rec_lo[k]);
        const int j = L - 1 - k;
        t.rec_hi[k] = (float)((j % 2) ? rec_lo[j] : -rec_lo[j]);
    }
    return t;
}

#define EMD_WAVELET_CASES(LAUNCH) \
    switch (L) {                  \
        case 2: LAUNCH(2) break;  \
        case 4: LAUNCH(4) break;  \
        case 6: LAUNCH(6) break;  \
        case 8: LAUNCH(8) break;  \
    }

// x -> the pyramids (image stride pyr_stride) through the scratch approximations; sums != 0: the per-tile sums of d^2 as well
int run_forward(const Geometry& g, const float* x, float* pyr, char* ws, int B, int L, const WTaps& taps, bool sums, hipStream_t st) {
    for (int l = 1; l <= g.levels; ++l) {
        const float* in = l == 1 ? x : reinterpret_cast<const float*>(ws + g.scratch[l - 1]);
        const long in_stride = (long)g.nH[l - 1] * g.nW[l - 1];
        float* ca = l == g.levels ? pyr : reinterpret_cast<float*>(ws + g.scratch[l]);
        const long ca_stride = l == g.levels ? g.pyramid : (long)g.nH[l] * g.nW[l];
        double* part = sums ? reinterpret_cast<double*>(ws + g.part[l]) : nullptr;
        const int tiles_x = emd::tiles_of(g.nW[l], kTW);
        const dim3 grid((unsigned)(tiles_x * emd::tiles_of(g.nH[l], kATH)), (unsigned)B);
#define EMD_LAUNCH(LL)                                                                                                              \
    hipLaunchKernelGGL((wavelet_analysis_kernel<LL>), grid, dim3(256), 0, st, in, in_stride, g.nH[l - 1], g.nW[l - 1], ca, ca_stride, \
                       pyr + g.det[l], g.pyramid, g.nH[l], g.nW[l], tiles_x, taps, part);
        EMD_WAVELET_CASES(EMD_LAUNCH)
#undef EMD_LAUNCH
        const int rc = emd::check_launch("wavelet_analysis_kernel");
        if (rc != EMD_OK) return rc;
    }
    return EMD_OK;
}

// the pyramids -> out [B,H,W]; thr != NULL: [B][levels][3] soft thresholds applied as the coefficients are loaded
int run_inverse(const Geometry& g, const float* pyr, float* out, char* ws, int B, int L, const WTaps& taps, const float* thr,
                hipStream_t st) {
    for (int l = g.levels; l >= 1; --l) {
        const float* ca = l == g.levels ? pyr : reinterpret_cast<const float*>(ws + g.scratch[l]);
        const long ca_stride = l == g.levels ? g.pyramid : (long)g.nH[l] * g.nW[l];
        float* o = l == 1 ? out : reinterpret_cast<float*>(ws + g.scratch[l - 1]);
        const int oH = g.nH[l - 1], oW = g.nW[l - 1];
        const int tiles_x = emd::tiles_of(oW, kTW);
        const dim3 grid((unsigned)(tiles_x * emd::tiles_of(oH, kSTH)), (unsigned)B);
        const float* t = thr ? thr + (l - 1) * 3 : nullptr;
#define EMD_LAUNCH(LL)                                                                                                             \
    hipLaunchKernelGGL((wavelet_synthesis_kernel<LL>), grid, dim3(256), 0, st, ca, ca_stride, pyr + g.det[l], g.pyramid, g.nH[l],  \
                       g.nW[l], o, (long)oH * oW, oH, oW, tiles_x, taps, t, g.levels * 3);
        EMD_WAVELET_CASES(EMD_LAUNCH)
#undef EMD_LAUNCH
        const int rc = emd::check_launch("wavelet_synthesis_kernel");
        if (rc != EMD_OK) return rc;
    }
    return EMD_OK;
}

// what the three entry points check first; *g is filled when the arguments are accepted
int check_call(const char* who, const void* a, const void* b, int B, int H, int W, const double* rec_lo, int L, int levels, Geometry* g) {
    if (!a || !b || !rec_lo) {
        emd::set_error("%s: null pointer", who);
        return EMD_E_INVALID;
    }
    if (!shape_ok(B, H, W)) {
        emd::set_error("%s: bad shape (batch 0..65535, 1 <= H, W <= %d; got %d x %d x %d)", who, kMaxExtent, B, H, W);
        return EMD_E_INVALID;
    }
    if (!taps_ok(L)) {
        emd::set_error("%s: the tap count must be even, 2..%d (got %d)", who, kMaxTaps, L);
        return EMD_E_INVALID;
    }
    for (int k = 0; k < L; ++k) {
        if (!std::isfinite(rec_lo[k])) {
            emd::set_error("%s: tap %d is not finite", who, k);
            return EMD_E_INVALID;
        }
    }
    if (!geometry(B, H, W, L, levels, g)) {
        emd::set_error("%s: levels must be 1..floor(log2(min(H,W) / (taps - 1))) = %d (got %d; image %d x %d, %d taps)", who,
                       max_levels(H, W, L), levels, H, W, L);
        return EMD_E_INVALID;
    }
    return EMD_OK;
}

int check_workspace(const char* who, const void* ws, size_t have, size_t need, int B) {
    if (!ws) {
        emd::set_error("%s: null pointer (workspace)", who);
        return EMD_E_INVALID;
    }
    if (B > 0 && have < need) {
        emd::set_error("%s: workspace too small (%zu bytes, needs %zu)", who, have, need);
        return EMD_E_INVALID;
    }
    if (!emd::aligned16(ws)) {
        emd::set_error("%s: workspace must be 16-byte aligned", who);
        return EMD_E_ALIGN;
    }
    return EMD_OK;
}

}  // namespace

extern "C" size_t emd_wavelet_pyramid_floats(int H, int W, int ntaps, int levels, long* bands) {
    Geometry g;
    if (!geometry(1, H, W, ntaps, levels, &g)) return 0;
    if (bands) {
        bands[0] = 0;
        bands[1] = g.nH[levels];
        bands[2] = g.nW[levels];
        int i = 1;
        for (int l = levels; l >= 1; --l) {
            for (int band = 0; band < 3; ++band, ++i) {
                bands[3 * i] = g.det[l] + (long)band * g.nH[l] * g.nW[l];
                bands[3 * i + 1] = g.nH[l];
                bands[3 * i + 2] = g.nW[l];
            }
        }
    }
    return (size_t)g.pyramid;
}

extern "C" size_t emd_wavelet_workspace_bytes(int B, int H, int W, int ntaps, int levels) {
    Geometry g;
    if (B < 1 || !geometry(B, H, W, ntaps, levels, &g)) return 0;
    return g.transform_bytes;
}

extern "C" size_t emd_filter_wavelet_workspace_bytes(int B, int H, int W, int ntaps, int levels) {
    Geometry g;
    if (B < 1 || !geometry(B, H, W, ntaps, levels, &g)) return 0;
    return g.filter_bytes;
}

extern "C" int emd_wavelet_forward_f32(const float* x, float* pyramid, int B, int H, int W, const double* rec_lo_host, int ntaps,
                                       int levels, void* workspace, size_t workspace_bytes, emd_stream_t stream) {
    const char* who = "emd_wavelet_forward_f32";
    Geometry g;
    int rc = check_call(who, x, pyramid, B, H, W, rec_lo_host, ntaps, levels, &g);
    if (rc != EMD_OK) return rc;
    rc = check_workspace(who, workspace, workspace_bytes, g.transform_bytes, B);
    if (rc != EMD_OK || B == 0) return rc;
    const size_t nx = (size_t)B * H * W * sizeof(float), np = (size_t)B * g.pyramid * sizeof(float);
    EMD_REQUIRE(!emd::overlap(x, nx, pyramid, np), EMD_E_INVALID, "emd_wavelet_forward_f32: pyramid may not alias x");
    EMD_REQUIRE(!emd::overlap(workspace, g.transform_bytes, x, nx) && !emd::overlap(workspace, g.transform_bytes, pyramid, np), EMD_E_INVALID,
                "emd_wavelet_forward_f32: the workspace may not alias x or pyramid");
    return run_forward(g, x, pyramid, static_cast<char*>(workspace), B, ntaps, make_taps(rec_lo_host, ntaps), false,
                       static_cast<hipStream_t>(stream));
}

extern "C" int emd_wavelet_inverse_f32(const float* pyramid, float* out, int B, int H, int W, const double* rec_lo_host, int ntaps,
                                       int levels, void* workspace, size_t workspace_bytes, emd_stream_t stream) {
    const char* who = "emd_wavelet_inverse_f32";
    Geometry g;
    int rc = check_call(who, pyramid, out, B, H, W, rec_lo_host, ntaps, levels, &g);
    if (rc != EMD_OK) return rc;
    rc = check_workspace(who, workspace, workspace_bytes, g.transform_bytes, B);
    if (rc != EMD_OK || B == 0) return rc;
    const size_t nx = (size_t)B * H * W * sizeof(float), np = (size_t)B * g.pyramid * sizeof(float);
    EMD_REQUIRE(!emd::overlap(out, nx, pyramid, np), EMD_E_INVALID, "emd_wavelet_inverse_f32: out may not alias pyramid");
    EMD_REQUIRE(!emd::overlap(workspace, g.transform_bytes, out, nx) && !emd::overlap(workspace, g.transform_bytes, pyramid, np), EMD_E_INVALID,
                "emd_wavelet_inverse_f32: the workspace may not alias pyramid or out");
    return run_inverse(g, pyramid, out, static_cast<char*>(workspace), B, ntaps, make_taps(rec_lo_host, ntaps), nullptr,
                       static_cast<hipStream_t>(stream));
}

extern "C" int emd_filter_wavelet_f32(const float* x, float* out, int B, int H, int W, const double* rec_lo_host, int ntaps, int levels,
                                      int method, float sigma, float* sigma_used, void* workspace, size_t workspace_bytes,
                                      emd_stream_t stream) {
    const char* who = "emd_filter_wavelet_f32";
    Geometry g;
    int rc = check_call(who, x, out, B, H, W, rec_lo_host, ntaps, levels, &g);
    if (rc != EMD_OK) return rc;
    EMD_REQUIRE(method == EMD_WAVELET_BAYES || method == EMD_WAVELET_VISU, EMD_E_INVALID,
                "emd_filter_wavelet_f32: unknown method (EMD_WAVELET_BAYES or EMD_WAVELET_VISU)");
    EMD_REQUIRE(sigma == sigma && sigma <= FLT_MAX, EMD_E_INVALID, "emd_filter_wavelet_f32: sigma is NaN or infinite");
    rc = check_workspace(who, workspace, workspace_bytes, g.filter_bytes, B);
    if (rc != EMD_OK || B == 0) return rc;
    const size_t nx = (size_t)B * H * W * sizeof(float);
    EMD_REQUIRE(!emd::overlap(x, nx, out, nx), EMD_E_INVALID, "emd_filter_wavelet_f32: out may not alias x");
    EMD_REQUIRE(!emd::overlap(workspace, g.filter_bytes, x, nx) && !emd::overlap(workspace, g.filter_bytes, out, nx), EMD_E_INVALID,
                "emd_filter_wavelet_f32: the workspace may not alias x or out");
    EMD_REQUIRE(!sigma_used || (!emd::overlap(sigma_used, (size_t)B * sizeof(float), workspace, g.filter_bytes) &&
                                !emd::overlap(sigma_used, (size_t)B * sizeof(float), out, nx)),
                EMD_E_INVALID, "emd_filter_wavelet_f32: sigma_used may not alias out or the workspace");
    hipStream_t st = static_cast<hipStream_t>(stream);
    char* ws = static_cast<char*>(workspace);
    const WTaps taps = make_taps(rec_lo_host, ntaps);
    float* pyr = reinterpret_cast<float*>(ws + g.pyr_off);
    float* thr = reinterpret_cast<float*>(ws + g.thr_off);
    unsigned* hist = reinterpret_cast<unsigned*>(ws + g.hist_off);
    unsigned* state = reinterpret_cast<unsigned*>(ws + g.state_off);
    rc = run_forward(g, x, pyr, ws, B, ntaps, taps, true, st);
    if (rc != EMD_OK) return rc;
    if (sigma < 0.f) {
        const hipError_t e = hipMemsetAsync(hist, 0, select_hist_bytes(B), st);
        if (e != hipSuccess) {
            emd::set_error("emd_filter_wavelet_f32: hipMemsetAsync: %s", hipGetErrorString(e));
            return EMD_E_LAUNCH;
        }
        const long n = (long)g.nH[1] * g.nW[1];
        const dim3 grid((unsigned)((n + kSelChunk - 1) / kSelChunk), (unsigned)B);
        for (int pass = 0; pass < 4; ++pass) {
            hipLaunchKernelGGL(wavelet_select_kernel, grid, dim3(256), 0, st, pyr + g.det[1] + 2 * n, g.pyramid, n, hist, state, pass);
            rc = emd::check_launch("wavelet_select_kernel");
            if (rc != EMD_OK) return rc;
        }
    }
    LevelSums ls{};
    ls.levels = levels;
    for (int l = 1; l <= levels; ++l) {
        ls.tiles[l - 1] = emd::tiles_of(g.nH[l], kATH) * emd::tiles_of(g.nW[l], kTW);
        ls.off[l - 1] = (long)((g.part[l] - g.part[1]) / sizeof(double));
        ls.count[l - 1] = (double)g.nH[l] * (double)g.nW[l];
    }
    hipLaunchKernelGGL(wavelet_threshold_kernel, dim3((unsigned)B), dim3(256), 0, st, ls, reinterpret_cast<const double*>(ws + g.part[1]),
                       hist, state, sigma, method, std::sqrt(2.0 * std::log((double)H * (double)W)), sigma_used, thr);
    rc = emd::check_launch("wavelet_threshold_kernel");
    if (rc != EMD_OK) return rc;
    return run_inverse(g, pyr, out, ws, B, ntaps, taps, thr, st);
}
