// Implicit-GEMM convolution on the matrix cores: pointwise 1x1, strided 1x1 and the four output
// phases of the 3x3 stride-2 transposed convolution, all with a fused per-channel epilogue.
//
// replaces (TensorFlow ops called by machine_learning/denoiser.py):
//   the pointwise half of slim.separable_convolution2d (:113-131) + its normalizer BN (:123) +
//     batch_then_activ (:134)                                  -> emd_conv1x1_f32
//   slim.conv2d(kernel_size=1[, stride=2]) + bias + BN + relu6 (:91-97, :159-164, :208-214,
//     :220-227)                                                -> emd_conv1x1_f32
//   slim.conv2d_transpose(k=3, stride=2, 'same') + bias + BN + relu6 (:141-148)
//                                                              -> emd_deconv3x3s2_f32
//   the residual "+=" that follows them (:264, :279, :294, :309, :322, :246, :360, :372, :384)
//     and tf.concat (:203, :353, :365: outputs are written straight into channel slices).
//
// C[M,N] = epilogue( A[M,K] * W[K,N] ):  M = B*Hg*Wg output positions, K = taps*Cin, N = Cout.
//   A is never materialised: row m = (b,i,j) reads, for tap t, source pixel (b, i*sa+dy_t, j*sa+dx_t)
//   of the NHWC fp32 activation tensor (zero outside the image), channels contiguous.
//   W is pre-packed once on the host (emd_pack_weights_bf16) as two bf16 planes (hi, lo) in
//   [Npad][taps*Cpad] order, i.e. K-contiguous per output channel, zero padded.
//
// Numerics ("split-bf16", PASSES=3): fp32 activations are split in-kernel into bf16 hi + bf16 lo
// (a = hi + lo + O(2^-17 a)) and  acc += Ahi*Whi + Ahi*Wlo + Alo*Whi  in fp32 on
// v_mfma_f32_32x32x16_bf16: ~2^-16 relative per product, which is what keeps a ~60-layer network
// inside the 1e-3 relative-L2 parity bar (plain bf16 inputs, PASSES=1, is ~2^-9 per layer and is
// offered as the fast mode).
//
// Block = 256 threads = 4 waves; block tile 128 x BN (BN 128 or 64), K step 64; each wave owns a
// 64x64 (or 32x64) sub-tile as 32x32 MFMA tiles.  A: global fp32 -> registers (issued one K step
// ahead) -> split -> LDS bf16 planes; W: global bf16 -> registers -> LDS.  LDS rows are 144 B
// (128 + 16 pad): the ds_read_b128 fragment reads and the ds_write_b64/b128 staging writes (one full
// row per lane group) are bank-conflict free.  The epilogue stages the fp32 tile through LDS so that
// stores and residual loads are 16 B per lane, a whole pixel's channel run per 32 lanes.
// Block index -> tile mapping is XCD-aware: the N-tiles of one M-tile (which re-read the same
// activation rows) get consecutive indices inside one XCD's share of the grid.
#include <type_traits>

#include "conv_plan.hpp"
#include "bn_chain_dev.hpp"
#include "f4_math.hpp"

namespace {

using namespace emd;

__device__ __attribute__((aligned(16))) float g_zero16[4];   // what padding rows and channel tails load

// Block tile 128 x BN (BN = 128: 2x2 waves of 64x64; BN = 64: 4x1 waves of 32x64), K step 64.
template <int BN, int PASSES, bool FLAT, bool UP = false>
__global__ __launch_bounds__(256, 2) void gemm_conv_kernel(const std::conditional_t<UP, GemmUpParams, GemmParams> p) {
    static_assert(!UP || FLAT, "the upsampled shift is a mode of the plain pointwise instance");
    constexpr int BM = 128, BK = 64;
    constexpr int LDK = BK + 8;                      // bf16 elements per LDS row: 144 B, conflict-free b128 reads
    constexpr int WM = BN == 128 ? 2 : 4, WN = 4 / WM;
    constexpr int TM = BM / WM / 32, TN = BN / WN / 32;
    constexpr int NPL = PASSES == 3 ? 2 : 1;         // bf16 planes kept in LDS
    constexpr int A_PASSES = BM / 16;                // 16 float4 per 64-float row -> 16 rows per pass
    constexpr int W_PASSES = BN / 32;                // 8 x 16-B chunks per 64-bf16 row -> 32 rows per pass
    constexpr int LDS_STAGE = BN + 4;                // fp32 epilogue staging row (floats)
    constexpr int A_BYTES = NPL * BM * LDK * 2, B_BYTES = NPL * BN * LDK * 2;
    constexpr int STAGE_BYTES = BM * LDS_STAGE * 4;
    constexpr int TILE_BYTES = A_BYTES + B_BYTES > STAGE_BYTES ? A_BYTES + B_BYTES : STAGE_BYTES;

    // ONE LDS object, carved by hand (tiles | row maps); the epilogue staging overlays the tiles
    __shared__ __attribute__((aligned(16))) unsigned char smem[TILE_BYTES + 2 * BM * 8];
    auto As = reinterpret_cast<uint16_t(*)[BM][LDK]>(smem);
    auto Bs = reinterpret_cast<uint16_t(*)[BN][LDK]>(smem + A_BYTES);
    float(*stage)[LDS_STAGE] = reinterpret_cast<float(*)[LDS_STAGE]>(smem);
    long long* rowA = reinterpret_cast<long long*>(smem + TILE_BYTES);  // element offset of the source pixel (-1: zero row)
    long long* rowP = rowA + BM;                                        // destination pixel index (-1: beyond M)

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wv = tid >> 6;
    const int wm = wv / WN, wn = wv % WN;

    // XCD-aware tile mapping (bijective for any grid size): the N-tiles of one M-tile are neighbours in one XCD
    const int nblk = p.n_mtiles * p.n_ntiles;
    int bid = blockIdx.x;
    {
        const int q = nblk >> 3, r = nblk & 7, xcd = bid & 7, loc = bid >> 3;
        bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + loc;
    }
    const int mt = bid / p.n_ntiles, nt = bid % p.n_ntiles;
    const long m0 = (long)mt * BM;
    const int n0 = nt * BN;

    auto map_rows = [&](int tap, bool with_dest) {
        if (tid < BM) {
            const long m = m0 + tid;
            long long src = -1, dst = -1;
            if (m < p.M) {
                if (FLAT) {
                    src = dst = m;
                } else {
                    const int j = (int)(m % p.Wg);
                    const long t = m / p.Wg;
                    const int i = (int)(t % p.Hg);
                    const long b = t / p.Hg;
                    const int dy = (int)((p.dyp >> (7 * tap)) & 127) - 64;
                    const int dx = (int)((p.dxp >> (7 * tap)) & 127) - 64;
                    const int iy = i * p.sa + dy, ix = j * p.sa + dx;
                    if (iy >= 0 && iy < p.Ha && ix >= 0 && ix < p.Wa) src = (b * p.Ha + iy) * (long)p.Wa + ix;
                    dst = (b * p.Hc + (i * p.sc + p.py)) * (long)p.Wc + (j * p.sc + p.px);
                }
            }
            rowA[tid] = src < 0 ? -1 : src * p.lda;
            if (with_dest) rowP[tid] = dst;
        }
    };
    const bool rows_all_valid = m0 + BM <= p.M;   // block-uniform

    // global -> register staging, one K step ahead.  The loop starts at it = -1 (stage tile 0 only) so that
    // the load code and the LDS-store code each exist once, straight-line and fully unrolled.
    f32x4 areg[A_PASSES];
    u32x4 whreg[W_PASSES], wlreg[W_PASSES];
    const int a_col = (tid & 15) * 4;     // first of this thread's 4 consecutive channels in the K step
    const int a_row = tid >> 4;           // + 16 per pass
    const int w_col = (tid & 7) * 8;
    const int w_row = tid >> 3;           // + 32 per pass
    const int Ktot = p.ntaps * p.Cpad;
    const uint16_t* __restrict__ whi = p.Whi + (long)(n0 + w_row) * Ktot + w_col;
    const uint16_t* __restrict__ wlo = NPL == 2 ? p.Wlo + (long)(n0 + w_row) * Ktot + w_col : nullptr;
    const long w_pass_stride = 32L * Ktot;
    const float* __restrict__ Ab = p.A + a_col;

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    const int ksteps = p.Cpad / BK;
    const int total = p.ntaps * ksteps;
    map_rows(0, true);
    __syncthreads();
    const int fr = lane & 31, fh = lane >> 5;
    // this thread's 8 source-row offsets live in registers for a whole tap: re-reading them from LDS before
    // every load put 8 serial LDS round trips + 8 divergent branches in front of each K step's loads
    long long aoff[A_PASSES];
#pragma unroll
    for (int q = 0; q < A_PASSES; ++q) aoff[q] = rowA[a_row + q * 16];

    for (int it = -1; it < total; ++it) {
        if (it >= 0) {
            // registers (tile `it`) -> LDS, splitting the activations into bf16 hi/lo on the way
#pragma unroll
            for (int q = 0; q < A_PASSES; ++q) {
                const int r = a_row + q * 16;
                unsigned h0, l0, h1, l1;
                split2(areg[q][0], areg[q][1], h0, l0);
                split2(areg[q][2], areg[q][3], h1, l1);
                *reinterpret_cast<u32x2*>(&As[0][r][a_col]) = u32x2{h0, h1};
                if (NPL == 2) *reinterpret_cast<u32x2*>(&As[NPL - 1][r][a_col]) = u32x2{l0, l1};
            }
#pragma unroll
            for (int q = 0; q < W_PASSES; ++q) {
                const int r = w_row + q * 32;
                *reinterpret_cast<u32x4*>(&Bs[0][r][w_col]) = whreg[q];
                if (NPL == 2) *reinterpret_cast<u32x4*>(&Bs[NPL - 1][r][w_col]) = wlreg[q];
            }
            __syncthreads();  // tile `it` visible
        }
        {
            // stage tile it+1 (the last iteration re-loads its own tile: keeps this path branch-free)
            const int nx = it + 1 < total ? it + 1 : it;
            const int tap = nx / ksteps, c0 = (nx - tap * ksteps) * BK;
            if (c0 == 0 && !FLAT && nx != it && nx > 0) {  // tap change: new source rows (block-uniform)
                map_rows(tap, false);
                __syncthreads();
#pragma unroll
                for (int q = 0; q < A_PASSES; ++q) aoff[q] = rowA[a_row + q * 16];
            }
            const bool kok = c0 + a_col < p.Cin;  // Cin % 4 == 0: a float4 is all inside or all outside
            {   // (round 4: the plain 1x1 forms had a fast path -- all rows real, plain loads -- beside a masked one that selected on the LOADED
                // value; the compiler joined the two with copies of the loaded registers, i.e. uses: s_waitcnt vmcnt(0) right behind the
                // loads in the steady state, the next K step's latency exposed in front of this step's MFMAs.  One path, select on the address.)
                // forms with taps / strides: a row without a source pixel for this tap (padding) or a channel group beyond Cin
                // reads 16 zero bytes.  The select is on the ADDRESS -- a select on the loaded value makes the wave wait for the
                // load right here instead of a whole MFMA phase later (measured: the 3x3 / transposed-conv phases of graph D
                // 6 - 12 % faster).
#pragma unroll
                for (int q = 0; q < A_PASSES; ++q) {
                    const float* src = (aoff[q] >= 0 && kok) ? Ab + aoff[q] + c0 : g_zero16;
                    areg[q] = *reinterpret_cast<const f32x4*>(src);
                }
            }
            const long kk = (long)tap * p.Cpad + c0;
#pragma unroll
            for (int q = 0; q < W_PASSES; ++q) {
                whreg[q] = *reinterpret_cast<const u32x4*>(whi + kk + q * w_pass_stride);
                if (NPL == 2) wlreg[q] = *reinterpret_cast<const u32x4*>(wlo + kk + q * w_pass_stride);
            }
        }
        if (it < 0) continue;
        // 16-wide K sub-steps that hold real channels in this tile (the last tile of Cin = 728 has 24 of 64:
        // the all-padding sub-steps are skipped, block-uniformly)
        const int kvalid = p.Cin - (it % ksteps) * BK;
#pragma unroll
        for (int ks = 0; ks < BK / 16; ++ks) {
            if (ks * 16 >= kvalid) break;
            bf16x8 ah[TM], al[TM], bh[TN], bl[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                const int r = wm * (BM / WM) + i * 32 + fr;
                ah[i] = *reinterpret_cast<const bf16x8*>(&As[0][r][ks * 16 + fh * 8]);
                if (NPL == 2) al[i] = *reinterpret_cast<const bf16x8*>(&As[NPL - 1][r][ks * 16 + fh * 8]);
            }
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const int r = wn * (BN / WN) + j * 32 + fr;
                bh[j] = *reinterpret_cast<const bf16x8*>(&Bs[0][r][ks * 16 + fh * 8]);
                if (NPL == 2) bl[j] = *reinterpret_cast<const bf16x8*>(&Bs[NPL - 1][r][ks * 16 + fh * 8]);
            }

#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    if (PASSES == 3) {  // small terms first
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[i], bh[j], acc[i][j], 0, 0, 0);
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bl[j], acc[i][j], 0, 0, 0);
                    }
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bh[j], acc[i][j], 0, 0, 0);
                }

        }
        __syncthreads();  // all fragment reads of tile `it` done before it is overwritten
    }

    // ---- epilogue.  The accumulators (C/D layout of mfma_32x32: col = lane&31, row = (e&3)+8*(e>>2)+4*(lane>>5))
    // go through an fp32 staging tile in LDS so that global traffic is 16 B per lane along the channel axis:
    // one 512-B (BN=128) run per output pixel for the stores and for the residual loads.
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int r = wm * (BM / WM) + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * fh;
                stage[r][wn * (BN / WN) + j * 32 + fr] = acc[i][j][e];
            }
    if constexpr (UP) {
        // (image, oy, ox) of each row, one division chain per row instead of one per (row, thread): rowA is free after the K loop
        if (tid < BM) {
            const long long pix = rowP[tid];
            if (pix >= 0) {
                const long long t = pix / p.Wc;
                rowA[tid] = ((t / p.Hc) << 40) | ((t % p.Hc) << 20) | (pix % p.Wc);   // Hc, Wc <= 2^20 (checked at the entry)
            }
        }
    }
    __syncthreads();
    constexpr int C4 = BN / 4;            // float4 chunks per staged row
    constexpr int ROWS_PER_PASS = 256 / C4;
    constexpr int NROWS = BM / ROWS_PER_PASS;
    const int ec = (tid % C4) * 4, er = tid / C4;
    const int n = n0 + ec;
    double ssum[4] = {0.0, 0.0, 0.0, 0.0}, ssq[4] = {0.0, 0.0, 0.0, 0.0};
    static_assert(ROWS_PER_PASS * BN * 2 * 8 <= TILE_BYTES && 2 * BN <= 256, "the statistics reduction reuses the tile memory");
    if (n < p.N) {                        // N % 4 == 0: a chunk is all inside or all outside
        const f32x4 s1 = *reinterpret_cast<const f32x4*>(p.scale1 + n);
        const f32x4 t1 = UP ? f32x4{0.f, 0.f, 0.f, 0.f} : *reinterpret_cast<const f32x4*>(p.shift1 + n);   // UP: sampled per pixel below
        f32x4 s2 = {1.f, 1.f, 1.f, 1.f}, t2 = {0.f, 0.f, 0.f, 0.f};
        if (p.scale2) {
            s2 = *reinterpret_cast<const f32x4*>(p.scale2 + n);
            t2 = *reinterpret_cast<const f32x4*>(p.shift2 + n);
        }
        float* __restrict__ outp = p.C;
        // one clamp form for every activation code: v = min(max(max(v, lo), slope*v), hi) -- (lo, slope, hi) = none: (-inf, 1, inf); relu6: (0, 1, 6);
        // relu: (0, 1, inf); leaky relu (graph G): (-inf, 0.2, inf); a clamped negative comes out as +0, as tf.nn.relu6 gives it
        const float hi = p.act == 1 ? 6.f : __builtin_inff();
        const float hi2 = p.act == 2 ? __builtin_inff() : 6.f;   // second stage (extra BN): relu6, or relu with act code relu
        const float slope = p.act == 4 ? 0.2f : 1.f, lo = (p.act == 1 || p.act == 2) ? 0.f : -__builtin_inff();
        const bool two = p.scale2 != nullptr;
        auto finish = [&](f32x4 v) {
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                float u = fmaf(v[c], s1[c], t1[c]);
                u = fminf(fmaxf(fmaxf(u, lo), slope * u), hi);
                if (two) u = fminf(fmaxf(fmaf(u, s2[c], t2[c]), 0.f), hi2);
                v[c] = u;
            }
            return v;
        };
        if constexpr (UP) {
            // y = act(fmaf(acc, scale1, up(pixel, n))): no second affine, no residual (refused at the entry).  Four rows at a time: their
            // 16 taps (16 bytes each, this thread's channel quad) are requested before the first is used; a row beyond M reads zeros.
            constexpr int G = 4;
            static_assert(NROWS % G == 0, "rows per thread come in groups of four");
            const UpSample& u = p.u;
#pragma unroll 1
            for (int g = 0; g < NROWS; g += G) {
                f32x4 tp[G][4];
                float ly[G], lx[G];
                long long pixv[G];
#pragma unroll
                for (int k = 0; k < G; ++k) {
                    const int r = er + (g + k) * ROWS_PER_PASS;
                    const long long pix = rowP[r], q = rowA[r];
                    pixv[k] = pix;
                    int y0, y1, x0, x1;
                    resize_src((int)((q >> 20) & 0xfffff), u.sy, u.Hu, y0, y1, ly[k]);
                    resize_src((int)(q & 0xfffff), u.sx, u.Wu, x0, x1, lx[k]);
                    const float* ub = u.up + ((q >> 40) * u.Hu) * (long)u.Wu * u.ldup + n;
                    const bool ok = pix >= 0;
                    tp[k][0] = *reinterpret_cast<const f32x4*>(ok ? ub + ((long)y0 * u.Wu + x0) * u.ldup : g_zero16);
                    tp[k][1] = *reinterpret_cast<const f32x4*>(ok ? ub + ((long)y0 * u.Wu + x1) * u.ldup : g_zero16);
                    tp[k][2] = *reinterpret_cast<const f32x4*>(ok ? ub + ((long)y1 * u.Wu + x0) * u.ldup : g_zero16);
                    tp[k][3] = *reinterpret_cast<const f32x4*>(ok ? ub + ((long)y1 * u.Wu + x1) * u.ldup : g_zero16);
                }
#pragma unroll
                for (int k = 0; k < G; ++k) {
                    if (pixv[k] < 0) continue;
                    const int r = er + (g + k) * ROWS_PER_PASS;
                    f32x4 v = *reinterpret_cast<const f32x4*>(&stage[r][ec]);
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const float sh = lerpf(lerpf(tp[k][0][c], tp[k][1][c], lx[k]), lerpf(tp[k][2][c], tp[k][3][c], lx[k]), ly[k]);
                        const float a = fmaf(v[c], s1[c], sh);
                        v[c] = fminf(fmaxf(fmaxf(a, lo), slope * a), hi);
                    }
                    *reinterpret_cast<f32x4*>(outp + pixv[k] * p.ldc + n) = v;
                }
            }
        } else if (p.res) {
            // all residual values of this thread's rows are requested before the first one is used
            f32x4 rv[NROWS];
#pragma unroll
            for (int k = 0; k < NROWS; ++k) {
                const long long pix = rowP[er + k * ROWS_PER_PASS];
                rv[k] = pix >= 0 ? *reinterpret_cast<const f32x4*>(p.res + pix * p.ldres + n) : f32x4{0.f, 0.f, 0.f, 0.f};
            }
#pragma unroll
            for (int k = 0; k < NROWS; ++k) {
                const int r = er + k * ROWS_PER_PASS;
                const long long pix = rowP[r];
                if (pix >= 0) *reinterpret_cast<f32x4*>(outp + pix * p.ldc + n) = finish(*reinterpret_cast<const f32x4*>(&stage[r][ec])) + rv[k];
            }
        } else if (p.stats_part) {
            // batch statistics of the output gathered while the tile is in hand (as gemm_split.hip's: per-thread double sums over its
            // rows here, row groups -> 1 below, one partial per (M tile, channel) for the fixed-order final reduction bn_stats_final)
#pragma unroll 4
            for (int r = er; r < BM; r += ROWS_PER_PASS) {
                const long long pix = rowP[r];
                if (pix < 0) continue;
                const f32x4 v = finish(*reinterpret_cast<const f32x4*>(&stage[r][ec]));
                *reinterpret_cast<f32x4*>(outp + pix * p.ldc + n) = v;
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const double d = (double)v[c];
                    ssum[c] += d;
                    ssq[c] += d * d;
                }
            }
        } else {
#pragma unroll 4
            for (int r = er; r < BM; r += ROWS_PER_PASS) {
                const long long pix = rowP[r];
                if (pix < 0) continue;
                *reinterpret_cast<f32x4*>(outp + pix * p.ldc + n) = finish(*reinterpret_cast<const f32x4*>(&stage[r][ec]));
            }
        }
    }
    if (p.stats_part) {   // block-uniform
        __syncthreads();  // the staging tile has been read out
        double(*red)[BN][2] = reinterpret_cast<double(*)[BN][2]>(smem);   // [row groups][BN channels][sum, sum of squares]
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            red[er][ec + c][0] = ssum[c];
            red[er][ec + c][1] = ssq[c];
        }
        __syncthreads();
        if (tid < 2 * BN) {
            const int which = tid / BN, col = tid % BN;
            if (n0 + col < p.N) {
                double t = 0.0;
#pragma unroll
                for (int k = 0; k < ROWS_PER_PASS; ++k) t += red[k][col][which];
                const long slab = p.stats_nph ? ((long)(mt / p.stats_tpi) * p.stats_nph + p.stats_ph) * p.stats_tpi + mt % p.stats_tpi : mt;
                p.stats_part[(slab * 2 + which) * p.N + n0 + col] = t;
            }
        }
    }
}


template <int BN, int PASSES>
int launch(const emd::ConvPlan& pl, const GemmParams& p, const UpSample* up, hipStream_t st) {
    if (up) {
        GemmUpParams pu;
        static_cast<GemmParams&>(pu) = p;
        pu.u = *up;
        hipLaunchKernelGGL((gemm_conv_kernel<BN, PASSES, true, true>), pl.grid, dim3(256), 0, st, pu);
        return emd::check_launch("gemm_conv_kernel (upsampled shift)");
    }
    if (pl.form) hipLaunchKernelGGL((gemm_conv_kernel<BN, PASSES, true>), pl.grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL((gemm_conv_kernel<BN, PASSES, false>), pl.grid, dim3(256), 0, st, p);
    return emd::check_launch("gemm_conv_kernel");
}

}  // namespace

// plan -> instance (conv_entry.hip made the plan and filled p.n_mtiles / p.n_ntiles from it)
extern "C" int gemm_conv_launch(const emd::ConvPlan& pl, const GemmParams& p, const UpSample* up, hipStream_t st) {
    if (pl.bn == 64) return pl.passes == 3 ? launch<64, 3>(pl, p, up, st) : launch<64, 1>(pl, p, up, st);
    return pl.passes == 3 ? launch<128, 3>(pl, p, up, st) : launch<128, 1>(pl, p, up, st);
}
