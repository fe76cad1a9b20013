// Fused separable convolution: depthwise 3x3 (stride 1, rate 1, TF SAME) -> 1x1 on the matrix cores ->
// folded batch norms + relu6 (+ second affine + relu6, + residual), in ONE kernel.
// replaces: slim.separable_convolution2d + _batch_norm_fn + batch_then_activ, i.e. the whole
//           strided_conv_block of machine_learning/denoiser.py:110-136 (for stride 1), and the "+=" after it.
//
// Why: for the layers whose Cout fits one N-tile (<= 128) and that run at 256x256 / 512x512 the unfused
// pair (emd_dw3x3_f32 + emd_conv1x1_f32) is HBM-bound and moves the depthwise result through HBM twice
// (write, then read): in + dw + dw + out bytes.  Fused, the depthwise result only ever exists as the bf16
// hi/lo A-operand planes in LDS: in(+halo) + out bytes.
//
// Block = 256 threads = 4 waves; output tile = 8 x 16 pixels (128 GEMM rows) x all Cout (BN = 64 or 128).
// Per 32-channel chunk of Cin:
//   1. the (8+2) x (16+2) pixel fp32 input patch of the chunk is staged global -> registers (one chunk
//      ahead; unconditional loads, padding pixels read a zero buffer) -> LDS; pixel pitch 40 floats so the
//      depthwise reads below are bank-conflict free; the chunk's 9 x 32 depthwise weights take the same route;
//      GEN instances rebuild the chunk from a one-value-per-pixel tensor instead (emd_sep3x3_fused_gen_f32);
//   2. thread (pixel group of 4 along W, 4 channels) reads 3 x 6 patch vectors (18 ds_read_b128 for 16
//      outputs), accumulates the 9 taps in fp32, splits to bf16 hi/lo and writes the A planes;
//   3. v_mfma_f32_32x32x16_bf16, split-bf16 (3 passes) as in gemm_conv.hip; W tile staged like there.
// Epilogue identical to gemm_conv.hip (fp32 LDS staging, 16-byte stores / residual loads).  A workgroup walks up to 8
// tiles side by side with the staging pipeline running on across them; DESIGN.md 3.3 has the measurements.
#include <cstdlib>
#include <type_traits>

#include "sep_params.hpp"

using namespace emd;

namespace {

// source of the zero-padding pixels: the patch loads are unconditional (a select on the loaded value would make the wave wait for
// the load where it is issued instead of a whole depthwise + MFMA phase later)
__device__ __attribute__((aligned(16))) float g_zero_px[4096];

// BN = columns of the workgroup's GEMM tile: 64 / 128 (one output), or with DUAL the two outputs side by side: 128 = 64 | 64 on an
// 8 x 16 pixel tile, 256 = 128 | 128 on a 4 x 16 pixel tile (TH = 4: the accumulators of both outputs fit the same registers).
// WRES (BN = 64, Cin <= 64): the whole pointwise weight matrix (at most two 32-channel chunks, 10 KB each with the lo plane) is put into
// LDS once per workgroup instead of once per (tile, chunk): with a generated input it was 90 % of the bytes the loader moved.
template <int BN, int PASSES, bool GEN, int TH = 8, bool DUAL = false, bool WRES = false>
__global__ __launch_bounds__(256, 2) void sep_fused_kernel(const SepParams p) {
    constexpr int TW = 16, BM = TH * TW, BK = 32;
    constexpr int PH = TH + 2, PW = TW + 2, NPX = PH * PW;  // 10 x 18 = 180 patch pixels (6 x 18 = 108 for TH = 4)
    constexpr int PLD = 40;                                 // floats per patch pixel (32 + 8 pad)
    constexpr int LDK = BK + 8;                             // bf16 per A/B row (80 B)
    constexpr int WN = BN / 64, WM = 4 / WN;                // every wave owns 64 columns: 4 x 1, 2 x 2 or 1 x 4 waves
    constexpr int TM = BM / WM / 32, TN = BN / WN / 32;
    constexpr int NPL = PASSES == 3 ? 2 : 1;
    constexpr int P_PASSES = (NPX * 8 + 255) / 256;          // 1440 float4 -> 6 passes (864 -> 4)
    constexpr int W_PASSES = BN / 64;                        // BN rows x 4 chunks of 16 B
    constexpr int NPT = BM / 32;                             // pixels per thread along W in the depthwise role (4 or 2)
    static_assert(TM >= 1 && TN == 2 && (!DUAL || (!GEN && PASSES == 3 && WN >= 2)), "tile shape");
    constexpr int LDS_STAGE = BN + 4;
    constexpr int B_CHUNK = NPL * BN * LDK * 2;               // one chunk's W tile (hi [+ lo] plane)
    constexpr int PATCH_BYTES = NPX * PLD * 4, A_BYTES = NPL * BM * LDK * 2, B_BYTES = B_CHUNK * (WRES ? 2 : 1);
    static_assert(!WRES || (BN == 64 && !DUAL), "the resident-W form is the 64-column single-output instance");
    constexpr int STAGE_BYTES = BM * LDS_STAGE * 4;
    constexpr int DW_BYTES = 9 * BK * 4;                     // the chunk's depthwise weights [9][32]
    constexpr int DW_OFF = PATCH_BYTES + A_BYTES + B_BYTES > STAGE_BYTES ? PATCH_BYTES + A_BYTES + B_BYTES : STAGE_BYTES;   // clear of the staging tile
    constexpr int TILE_BYTES = DW_OFF + DW_BYTES;

    __shared__ __attribute__((aligned(16))) unsigned char smem[TILE_BYTES];
    float* patch = reinterpret_cast<float*>(smem);
    auto As = reinterpret_cast<uint16_t(*)[BM][LDK]>(smem + PATCH_BYTES);
    auto Bs = reinterpret_cast<uint16_t(*)[BN][LDK]>(smem + PATCH_BYTES + A_BYTES);
    float(*stage)[LDS_STAGE] = reinterpret_cast<float(*)[LDS_STAGE]>(smem);
    float* wks = reinterpret_cast<float*>(smem + DW_OFF);

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wv = tid >> 6;
    const int wm = wv / WN, wn = wv % WN;
    // Workgroups are handed to the 8 XCDs round-robin (id mod 8), so in launch order the tile under this one -- which shares two of
    // its ten patch rows -- runs on another XCD and the halo is fetched once per L2.  p.xcd: XCD k takes the k-th eighth of the tiles.
    int bx = blockIdx.x, by = blockIdx.y, bz = blockIdx.z;
    xcd_remap(p.xcd, bx, by, bz);   // the tile count is a multiple of 8 (host check)
    const int xbase = bx * p.tpw * TW, y0 = by * TH;
    int x0 = xbase;       // tile whose chunks are being computed (the epilogue's tile)
    const long img = (long)bz * p.H * p.W;  // pixel index of this image's (0,0)

    // ---- patch loader role: float4 #idx of the patch = (patch pixel idx/8, channel group idx%8)
    const float* psrc[P_PASSES];  // source pixel + channel group of chunk 0, or the zero buffer (padding / unused slots)
    bool pok[P_PASSES];           // generated input only: a real pixel (not padding)
    auto set_tile = [&](int xt) {
#pragma unroll
        for (int q = 0; q < P_PASSES; ++q) {
            const int idx = tid + q * 256;
            const float* o = GEN ? p.x : g_zero_px;
            bool ok = false;
            if (idx < NPX * 8) {
                const int ppx = idx >> 3, py = ppx / PW, px = ppx - py * PW;
                int gy = y0 - 1 + py, gx = xt - 1 + px;
                if (p.reflect) {  // index -1 -> 1, H -> H-2
                    gy = gy < 0 ? -gy : (gy >= p.H ? 2 * p.H - 2 - gy : gy);
                    gx = gx < 0 ? -gx : (gx >= p.W ? 2 * p.W - 2 - gx : gx);
                }
                if (gy >= 0 && gy < p.H && gx >= 0 && gx < p.W) {
                    o = p.x + (img + (long)gy * p.W + gx) * p.ldx + (GEN ? 0 : (idx & 7) * 4);
                    ok = true;
                }
            }
            psrc[q] = o;
            pok[q] = ok;
        }
    };
    set_tile(xbase);
    int ptile = 0;             // tile the patch offsets belong to
    // ---- W loader role
    const int w_col = (tid & 3) * 8, w_row = tid >> 2;  // + 64 rows per pass
    const uint16_t* __restrict__ whi = p.Whi + (long)w_row * p.Cpad + w_col;
    const uint16_t* __restrict__ wlo = NPL == 2 ? p.Wlo + (long)w_row * p.Cpad + w_col : nullptr;
    // DUAL: the second half of the B tile's rows are the 1x1 projection's weights
    const uint16_t* __restrict__ w2hi = DUAL ? p.W2hi + (long)w_row * p.Cpad + w_col : nullptr;
    const uint16_t* __restrict__ w2lo = DUAL ? p.W2lo + (long)w_row * p.Cpad + w_col : nullptr;
    // ---- depthwise role: NPT consecutive pixels of tile row ty, 4 channels
    const int c4 = tid & 7, pg = tid >> 3;
    const int ty = pg / (TW / NPT), tx0 = (pg % (TW / NPT)) * NPT;

    f32x4 preg[P_PASSES];
    f32x4 gga = {0.f, 0.f, 0.f, 0.f}, ggt = gga;   // generated input: the chunk's a / t vectors
    u32x4 wh[W_PASSES], wl[W_PASSES];
#pragma unroll
    for (int q = 0; q < W_PASSES; ++q) wh[q] = wl[q] = u32x4{0, 0, 0, 0};
    f32x4 wkreg = {0.f, 0.f, 0.f, 0.f};

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    const int nchunks = p.Cin / BK;
    if constexpr (WRES) {   // both chunks' W tiles, once (visible after the loop's first barrier)
        for (int c = 0; c < nchunks; ++c) {
            auto Bc = reinterpret_cast<uint16_t(*)[BN][LDK]>(smem + PATCH_BYTES + A_BYTES + c * B_CHUNK);
            *reinterpret_cast<u32x4*>(&Bc[0][w_row][w_col]) = *reinterpret_cast<const u32x4*>(whi + c * BK);
            if (NPL == 2) *reinterpret_cast<u32x4*>(&Bc[NPL - 1][w_row][w_col]) = *reinterpret_cast<const u32x4*>(wlo + c * BK);
        }
    }
    const int total = p.tpw * nchunks;   // (tile, chunk) steps of this workgroup: the staging pipeline runs on across tiles, so
                                         // a tile's epilogue overlaps the loads of the next tile's first chunk
    const int fr = lane & 31, fh = lane >> 5;

    constexpr bool EARLY_RES = BN == 64 && !DUAL;
    constexpr int E_C4 = BN / 4, E_RPP = 256 / E_C4, E_NROWS = BM / E_RPP;
    f32x4 rve[EARLY_RES ? E_NROWS : 1];
#pragma unroll
    for (int k = 0; k < (EARLY_RES ? E_NROWS : 1); ++k) rve[k] = f32x4{0.f, 0.f, 0.f, 0.f};

    long long ph[8] = {0, 0, 0, 0, 0, 0, 0, 0}, tprev = 0;
    if (p.stamps) tprev = __builtin_amdgcn_s_memtime();
#define SEP_STAMP(i) if (p.stamps) { const long long t_ = __builtin_amdgcn_s_memtime(); ph[i] += t_ - tprev; tprev = t_; }
    for (int it = -1; it < total; ++it) {
        if (it >= 0) {
            // staged registers (chunk `it`) -> LDS
            if (GEN) {
                const float ghi = p.gen_act == 1 ? 6.f : __builtin_inff();
                const float gsl = p.gen_act == 4 ? 0.2f : 1.f, glo = (p.gen_act == 1 || p.gen_act == 2) ? 0.f : -__builtin_inff();
#pragma unroll
                for (int q = 0; q < P_PASSES; ++q) {
                    const float dv = preg[q][0];
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const float u = fmaf(dv, gga[c], ggt[c]);
                        preg[q][c] = pok[q] ? fminf(fmaxf(fmaxf(u, glo), gsl * u), ghi) : 0.f;
                    }
                }
            }
#pragma unroll
            for (int q = 0; q < P_PASSES; ++q) {
                const int idx = tid + q * 256;
                if (idx < NPX * 8) *reinterpret_cast<f32x4*>(patch + (idx >> 3) * PLD + (idx & 7) * 4) = preg[q];
            }
            if (tid < 72) *reinterpret_cast<f32x4*>(wks + tid * 4) = wkreg;
            if constexpr (!WRES) {
#pragma unroll
                for (int q = 0; q < W_PASSES; ++q) {
                    *reinterpret_cast<u32x4*>(&Bs[0][w_row + 64 * q][w_col]) = wh[q];
                    if (NPL == 2) *reinterpret_cast<u32x4*>(&Bs[NPL - 1][w_row + 64 * q][w_col]) = wl[q];
                }
            }
            __syncthreads();  // (1) patch + W tile of chunk `it` visible
        }
        SEP_STAMP(0)
        // stage chunk it+1 (the last iteration re-loads its own chunk: branch-free).  Issued BEFORE the
        // depthwise work below so the loads have the depthwise + MFMA phases (not just the MFMAs) to land.
        const int nx = it + 1 < total ? it + 1 : it;
        const int ntile = nx / nchunks;
        const int c0n = (nx - ntile * nchunks) * BK;
        if (ntile != ptile) {   // block-uniform: the next step belongs to the next tile, 16 pixels to the right
            const int xt = xbase + ntile * TW;
            // between two tiles that both lie off the image's left and right edges only the x origin changes: every real source
            // pixel moves 16 pixels on, the padding rows above / below the image stay padding
            if (xt - TW > 0 && xt + TW < p.W) {
                const long step = (long)TW * p.ldx;
#pragma unroll
                for (int q = 0; q < P_PASSES; ++q) psrc[q] += pok[q] ? step : 0;
            } else {
                set_tile(xt);
            }
            ptile = ntile;
        }
        if (GEN) {   // the chunk is generated from the one-value-per-pixel tensor when it is written to LDS
            gga = *reinterpret_cast<const f32x4*>(p.gen_a + c0n + (tid & 7) * 4);
            ggt = *reinterpret_cast<const f32x4*>(p.gen_t + c0n + (tid & 7) * 4);
#pragma unroll
            for (int q = 0; q < P_PASSES; ++q) preg[q][0] = *psrc[q];
        } else {
#pragma unroll
            for (int q = 0; q < P_PASSES; ++q) preg[q] = *reinterpret_cast<const f32x4*>(psrc[q] + c0n);
        }
        // the chunk's 9 x 32 depthwise weights travel through LDS too: one 16-byte load for 72 threads instead of nine for every thread
        if (tid < 72) wkreg = *reinterpret_cast<const f32x4*>(p.dw + ((long)(tid >> 3) * p.Cin + c0n) + (tid & 7) * 4);
        if constexpr (!WRES)
#pragma unroll
        for (int q = 0; q < W_PASSES; ++q) {
            constexpr int HALF = W_PASSES / 2;
            if (DUAL && q >= HALF) {
                wh[q] = *reinterpret_cast<const u32x4*>(w2hi + (long)(q - HALF) * 64 * p.Cpad + c0n);
                wl[q] = *reinterpret_cast<const u32x4*>(w2lo + (long)(q - HALF) * 64 * p.Cpad + c0n);
            } else {
                wh[q] = *reinterpret_cast<const u32x4*>(whi + (long)q * 64 * p.Cpad + c0n);
                if (NPL == 2) wl[q] = *reinterpret_cast<const u32x4*>(wlo + (long)q * 64 * p.Cpad + c0n);
            }
        }
        // 64-column instances: a thread's 8 residual vectors (32 registers) of the CURRENT tile are requested here, at the start of the
        // tile's last chunk: they land under its depthwise and MFMA phases (the 128-column instances have no room: they ask four
        // rows at a time in the epilogue, two exposed round trips per tile)
        if (EARLY_RES && p.res && it >= 0 && (it + 1) % nchunks == 0) {
            const int ecol = (tid % E_C4) * 4, eer = tid / E_C4;
            if (ecol < p.N) {
                const float* __restrict__ rt = p.res + (img + (long)y0 * p.W) * p.ldres + ecol;
#pragma unroll
                for (int k = 0; k < E_NROWS; ++k) {
                    const int r = eer + k * E_RPP;
                    rve[k] = *reinterpret_cast<const f32x4*>(rt + ((r >> 4) * p.W + (r & 15) + x0) * p.ldres);
                }
            }
        }
        SEP_STAMP(1)
        if (it >= 0) {
            // depthwise 3x3 from the LDS patch -> bf16 hi/lo A planes
            f32x4 wk[9];
#pragma unroll
            for (int k = 0; k < 9; ++k) wk[k] = *reinterpret_cast<const f32x4*>(wks + k * BK + c4 * 4);
            f32x4 o[NPT];
#pragma unroll
            for (int j = 0; j < NPT; ++j) o[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                f32x4 pr[NPT + 2];
#pragma unroll
                for (int d = 0; d < NPT + 2; ++d)
                    pr[d] = *reinterpret_cast<const f32x4*>(patch + ((ty + i) * PW + tx0 + d) * PLD + c4 * 4);
#pragma unroll
                for (int j = 0; j < NPT; ++j)
#pragma unroll
                    for (int d = 0; d < 3; ++d) o[j] += wk[i * 3 + d] * pr[j + d];
            }
#pragma unroll
            for (int j = 0; j < NPT; ++j) {
                const int r = ty * TW + tx0 + j;
                unsigned h0, l0, h1, l1;
                split2(o[j][0], o[j][1], h0, l0);
                split2(o[j][2], o[j][3], h1, l1);
                *reinterpret_cast<u32x2*>(&As[0][r][c4 * 4]) = u32x2{h0, h1};
                if (NPL == 2) *reinterpret_cast<u32x2*>(&As[NPL - 1][r][c4 * 4]) = u32x2{l0, l1};
            }
        }
        SEP_STAMP(2)
        if (it < 0) continue;
        __syncthreads();  // (2) A planes of chunk `it` visible
        SEP_STAMP(3)
#pragma unroll
        for (int ks = 0; ks < BK / 16; ++ks) {
            bf16x8 ah[TM], al[TM], bh[TN], bl[TN];
            if (DUAL && wn >= WN / 2) {
                // the 1x1 projection's A operand = the block's INPUT at the tile's own pixels: the centre of the fp32 patch, split
                // into bf16 hi / lo here (8 channels per lane) instead of going through a second pair of A planes
#pragma unroll
                for (int i = 0; i < TM; ++i) {
                    const int r = wm * (BM / WM) + i * 32 + fr;
                    const float* src = patch + (((r >> 4) + 1) * PW + (r & 15) + 1) * PLD + ks * 16 + fh * 8;
                    const f32x4 v0 = *reinterpret_cast<const f32x4*>(src), v1 = *reinterpret_cast<const f32x4*>(src + 4);
                    unsigned h0, h1, h2, h3, l0, l1, l2, l3;
                    split2(v0[0], v0[1], h0, l0);
                    split2(v0[2], v0[3], h1, l1);
                    split2(v1[0], v1[1], h2, l2);
                    split2(v1[2], v1[3], h3, l3);
                    ah[i] = __builtin_bit_cast(bf16x8, (u32x4{h0, h1, h2, h3}));
                    al[i] = __builtin_bit_cast(bf16x8, (u32x4{l0, l1, l2, l3}));
                }
            } else {
#pragma unroll
                for (int i = 0; i < TM; ++i) {
                    const int r = wm * (BM / WM) + i * 32 + fr;
                    ah[i] = *reinterpret_cast<const bf16x8*>(&As[0][r][ks * 16 + fh * 8]);
                    if (NPL == 2) al[i] = *reinterpret_cast<const bf16x8*>(&As[NPL - 1][r][ks * 16 + fh * 8]);
                }
            }
            auto Bc = WRES ? reinterpret_cast<uint16_t(*)[BN][LDK]>(smem + PATCH_BYTES + A_BYTES + (it % nchunks) * B_CHUNK) : Bs;
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const int r = wn * (BN / WN) + j * 32 + fr;
                bh[j] = *reinterpret_cast<const bf16x8*>(&Bc[0][r][ks * 16 + fh * 8]);
                if (NPL == 2) bl[j] = *reinterpret_cast<const bf16x8*>(&Bc[NPL - 1][r][ks * 16 + fh * 8]);
            }
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    if (PASSES == 3) {
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[i], bh[j], acc[i][j], 0, 0, 0);
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bl[j], acc[i][j], 0, 0, 0);
                    }
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bh[j], acc[i][j], 0, 0, 0);
                }
        }
        SEP_STAMP(4)
        __syncthreads();  // (3) fragment reads done before the next chunk overwrites patch / A / B
        SEP_STAMP(5)
        if ((it + 1) % nchunks != 0) continue;   // more chunks of this tile to come

        // ---- epilogue (see gemm_conv.hip): accumulators -> fp32 LDS tile -> 16-byte stores along the channel axis
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int r = wm * (BM / WM) + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * fh;
                    stage[r][wn * (BN / WN) + j * 32 + fr] = acc[i][j][e];
                }
        __syncthreads();
        constexpr int C4 = BN / 4;
        constexpr int ROWS_PER_PASS = 256 / C4;
        const int ncol = (tid % C4) * 4, er = tid / C4;      // column of the staging tile
        const bool out2 = DUAL && ncol >= BN / 2;             // DUAL: the right half of the tile is the 1x1 projection
        const int n = out2 ? ncol - BN / 2 : ncol;            // channel of the output it belongs to
        if (n < (out2 ? p.N2 : p.N)) {
            const f32x4 s1 = *reinterpret_cast<const f32x4*>((out2 ? p.scale_b : p.scale1) + n);
            const f32x4 t1 = *reinterpret_cast<const f32x4*>((out2 ? p.shift_b : p.shift1) + n);
            f32x4 s2 = {1.f, 1.f, 1.f, 1.f}, t2 = {0.f, 0.f, 0.f, 0.f};
            if (p.scale2 && !out2) {
                s2 = *reinterpret_cast<const f32x4*>(p.scale2 + n);
                t2 = *reinterpret_cast<const f32x4*>(p.shift2 + n);
            }
            float* __restrict__ outp = out2 ? p.y2 : p.y;
            const int ldo = out2 ? p.ldy2 : p.ldy;
            // one clamp form for every activation code: v = min(max(max(v, lo), slope*v), hi) -- (lo, slope, hi) = none: (-inf, 1, inf); relu6: (0, 1, 6);
            // relu: (0, 1, inf); leaky relu (graph G): (-inf, 0.2, inf); a clamped negative comes out as +0, as tf.nn.relu6 gives it
            const int actc = out2 ? 1 : p.act;   // the projection of a DUAL launch is conv + BN + relu6 (conv_block_not_sep)
            const float hi = actc == 1 ? 6.f : __builtin_inff();
            const float hi2 = actc == 2 ? __builtin_inff() : 6.f;   // second stage (extra BN): relu6, or relu with act code relu
            const float slope = actc == 4 ? 0.2f : 1.f, lo = (actc == 1 || actc == 2) ? 0.f : -__builtin_inff();
            const bool two = p.scale2 != nullptr && !out2;
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
            constexpr int NROWS = BM / ROWS_PER_PASS;
            // tile row origin as a 64-bit pointer, the pixel relative to it as a 32-bit offset (the host checks 9 rows fit in 2^31 floats)
            // (x0 is folded into the 32-bit part on purpose: tile-invariant offsets would be hoisted out of the tile loop and pinned
            // in registers for the whole kernel)
            const long pix0 = img + (long)y0 * p.W;
            float* __restrict__ ytile = outp + pix0 * ldo + n;
            const float* __restrict__ rtile = p.res ? p.res + pix0 * p.ldres + n : nullptr;
            auto tpix = [&](int r) { return (r >> 4) * p.W + (r & 15) + x0; };
            // output stage: fp32 NHWC, or (single-output instances) the split32 layout through the pair exchange of emd::dw_store
            auto put = [&](int r, f32x4 v) {
                if (DUAL || !p.out_split) {
                    if (p.nt) store_nt16(ytile + tpix(r) * ldo, v);
                    else *reinterpret_cast<f32x4*>(ytile + tpix(r) * ldo) = v;
                    return;
                }
                unsigned h0, l0, h1, l1;
                split2(v[0], v[1], h0, l0);
                split2(v[2], v[3], h1, l1);
                const int q = n >> 2;
                const bool odd = q & 1;
                const unsigned r0 = emd::swap_pair(odd ? h0 : l0), r1 = emd::swap_pair(odd ? h1 : l1);
                unsigned char* g = reinterpret_cast<unsigned char*>(outp) + (pix0 + tpix(r)) * (long)ldo * 4 + (n >> 5) * 128;
                if (!odd) *reinterpret_cast<u32x4*>(g + (q & 7) * 8) = u32x4{h0, h1, r0, r1};
                else *reinterpret_cast<u32x4*>(g + 64 + ((q - 1) & 7) * 8) = u32x4{r0, r1, l0, l1};
            };
            if (EARLY_RES && p.res) {
#pragma unroll
                for (int k = 0; k < NROWS; ++k) {
                    const int r = er + k * ROWS_PER_PASS;
                    put(r, finish(*reinterpret_cast<const f32x4*>(&stage[r][ncol])) + rve[k]);
                }
            } else if (p.res && !DUAL) {
                // residual values are requested four rows at a time, before the first of them is used (the registers of the
                // next chunk's prefetch are live here: no room for all NROWS at once)
#pragma unroll
                for (int k0 = 0; k0 < NROWS; k0 += 4) {
                    f32x4 rv[4];
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const int r = er + (k0 + k) * ROWS_PER_PASS;
                        rv[k] = *reinterpret_cast<const f32x4*>(rtile + tpix(r) * p.ldres);
                    }
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const int r = er + (k0 + k) * ROWS_PER_PASS;
                        put(r, finish(*reinterpret_cast<const f32x4*>(&stage[r][ncol])) + rv[k]);
                    }
                }
            } else {
#pragma unroll 4
                for (int r = er; r < BM; r += ROWS_PER_PASS)
                    put(r, finish(*reinterpret_cast<const f32x4*>(&stage[r][ncol])));
            }
        }
        __syncthreads();  // the staging tile is read out before the next tile's patch overwrites it
        SEP_STAMP(6)
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
        x0 += TW;
    }
    if (p.stamps && tid == 0) {
        long long* o = p.stamps + ((long)(blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * 8;
#pragma unroll
        for (int i = 0; i < 8; ++i) o[i] = ph[i];
    }
#undef SEP_STAMP
}

// The generated-input layer with nothing staged but one scalar per pixel (emd_sep3x3_fused_gen9_f32; relu6 generation, zero padding,
// BN = 64, resident W tiles, split-bf16; NCH = Cin / 32 chunks).  The Cin-channel input act(d * a[c] + t[c]) is a function of d alone,
// so LDS holds the tile's (8+2) x (16+2) d values (row pitch 20 floats: a thread's six columns are one 16-byte and one 8-byte read) and
// the depthwise thread generates its 3 x 6 input vectors in registers, with the chunk's nine weight vectors and (a, t) resident in
// registers as well.  d itself is formed here from the 1-channel image p.x with the taps p.gen_w9 (cin1_kernel's statement): thread
// idx < 180 owns d pixel idx of the tile, requests its nine image values (clamped indices, unconditional) a whole tile ahead and writes
// d into the other half of a double-buffered tile before barrier (3), so a tile needs no barrier for d.  Per tile: both chunks'
// depthwise stages -> their own A planes, barrier (2), all MFMAs (chunk, k-step and pass order of sep_fused_kernel), barrier (3),
// epilogue through the staging tile (which shares the A planes' storage) as there.
template <int NCH, bool RES>
__global__ __launch_bounds__(256, 2) void sep_gen9_kernel(const SepParams p) {
    constexpr int TH = 8, TW = 16, BM = TH * TW, BN = 64, BK = 32, LDK = BK + 8;
    constexpr int DH = TH + 2, DW = TW + 2, DLD = 20, ND = DH * DW;
    constexpr int LDS_STAGE = BN + 4;
    constexpr int B_CHUNK = 2 * BN * LDK * 2, A_CHUNK = 2 * BM * LDK * 2;
    constexpr int D_BYTES = DH * DLD * 4, STAGE_BYTES = BM * LDS_STAGE * 4;
    constexpr int D_OFF = NCH * B_CHUNK, A_OFF = D_OFF + 2 * D_BYTES;
    constexpr int TILE_BYTES = A_OFF + (NCH * A_CHUNK > STAGE_BYTES ? NCH * A_CHUNK : STAGE_BYTES);
    static_assert(A_OFF % 16 == 0 && (DLD * 4) % 16 == 0, "16-byte reads of the d tile and the A planes");

    __shared__ __attribute__((aligned(16))) unsigned char smem[TILE_BYTES];
    float* dt = reinterpret_cast<float*>(smem + D_OFF);
    float(*stage)[LDS_STAGE] = reinterpret_cast<float(*)[LDS_STAGE]>(smem + A_OFF);

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wv = tid >> 6;
    int bx = blockIdx.x, by = blockIdx.y, bz = blockIdx.z;
    xcd_remap(p.xcd, bx, by, bz);
    const int xbase = bx * p.tpw * TW, y0 = by * TH;
    const long img = (long)bz * p.H * p.W;

    // ---- W tiles, once
    {
        const int w_col = (tid & 3) * 8, w_row = tid >> 2;
        const uint16_t* __restrict__ whi = p.Whi + (long)w_row * p.Cpad + w_col;
        const uint16_t* __restrict__ wlo = p.Wlo + (long)w_row * p.Cpad + w_col;
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            auto Bc = reinterpret_cast<uint16_t(*)[BN][LDK]>(smem + c * B_CHUNK);
            *reinterpret_cast<u32x4*>(&Bc[0][w_row][w_col]) = *reinterpret_cast<const u32x4*>(whi + c * BK);
            *reinterpret_cast<u32x4*>(&Bc[1][w_row][w_col]) = *reinterpret_cast<const u32x4*>(wlo + c * BK);
        }
    }
    // ---- depthwise role: 4 consecutive pixels of tile row ty, 4 channels of every chunk
    const int c4 = tid & 7, pg = tid >> 3;
    const int ty = pg >> 2, tx0 = (pg & 3) * 4;
    f32x4 wk[NCH][9], ga[NCH], gt[NCH];
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
#pragma unroll
        for (int k = 0; k < 9; ++k) wk[c][k] = *reinterpret_cast<const f32x4*>(p.dw + (long)k * p.Cin + c * BK + c4 * 4);
        ga[c] = *reinterpret_cast<const f32x4*>(p.gen_a + c * BK + c4 * 4);
        gt[c] = *reinterpret_cast<const f32x4*>(p.gen_t + c * BK + c4 * 4);
    }
    // ---- d role: d pixel (dpy, dpx) of the tile = image pixel (y0 - 1 + dpy, x0 - 1 + dpx); the threads past the tile compute its last
    // pixel again and do not write it
    const int di = tid < ND ? tid : ND - 1;
    const int dpy = di / DW, dpx = di - dpy * DW;
    bool rok[3];
    const float* irow[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int ry = y0 - 2 + dpy + i;
        rok[i] = ry >= 0 && ry < p.H;
        irow[i] = p.x + img + (long)(ry < 0 ? 0 : (ry >= p.H ? p.H - 1 : ry)) * p.W;
    }
    float w9[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) w9[k] = p.gen_w9[k];
    float iv[9];
    auto load_img = [&](int xt) {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int rx = xt - 2 + dpx + j;
            const int cx = rx < 0 ? 0 : (rx >= p.W ? p.W - 1 : rx);
#pragma unroll
            for (int i = 0; i < 3; ++i) iv[i * 3 + j] = irow[i][cx];
        }
    };
    auto form_d = [&](int xt, int buf) {   // cin1_kernel: taps in i, j order, the ones off the image skipped
        float d = 0.f;
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const int rx = xt - 2 + dpx + j;
                d = (rok[i] && rx >= 0 && rx < p.W) ? fmaf(w9[i * 3 + j], iv[i * 3 + j], d) : d;
            }
        if (tid < ND) dt[buf * (DH * DLD) + dpy * DLD + dpx] = d;
    };

    f32x16 acc[2];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[j][e] = 0.f;
    const int fr = lane & 31, fh = lane >> 5;
    constexpr int E_C4 = BN / 4, E_RPP = 256 / E_C4, E_NROWS = BM / E_RPP;
    const int ncol = (tid % E_C4) * 4, er = tid / E_C4;

    load_img(xbase);
    form_d(xbase, 0);
    // the resident vectors are pinned as arrived here: with a load of the prologue still pending at the loop's head the compiler puts a
    // wait for EVERY outstanding memory operation there, which each later tile spends waiting for the stores of the tile before
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
#pragma unroll
        for (int k = 0; k < 9; ++k) asm volatile("" : "+v"(wk[c][k]));
        asm volatile("" : "+v"(ga[c]), "+v"(gt[c]));
    }
    __syncthreads();   // W tiles and the first d tile visible

    for (int t = 0; t < p.tpw; ++t) {
        const int x0 = xbase + t * TW;
        // the thread's 3 x 6 d values
        float dv[3][6];
        {
            const float* dsrc = dt + (t & 1) * (DH * DLD) + ty * DLD + tx0;
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const f32x4 q = *reinterpret_cast<const f32x4*>(dsrc + i * DLD);
                const f32x2 r = *reinterpret_cast<const f32x2*>(dsrc + i * DLD + 4);
                dv[i][0] = q[0]; dv[i][1] = q[1]; dv[i][2] = q[2]; dv[i][3] = q[3]; dv[i][4] = r[0]; dv[i][5] = r[1];
            }
        }
        const bool more = t + 1 < p.tpw;   // workgroup-uniform
        if (more) load_img(x0 + TW);
        // generate + depthwise 3x3 -> bf16 hi/lo A planes, both chunks.  BORDER: the tile touches the image's edge; a padding pixel
        // of the generated input is 0, not relu6(t[c])
        auto stage1 = [&](auto border) {
            constexpr bool BORDER = decltype(border)::value;
            // of a thread's 3 x 6 pixels only whole rows and the first / last column can lie off the image
            bool rowok[3];
#pragma unroll
            for (int i = 0; i < 3; ++i) rowok[i] = y0 - 1 + ty + i >= 0 && y0 - 1 + ty + i < p.H;
            const bool c0ok = x0 - 1 + tx0 >= 0, c5ok = x0 + tx0 + 4 < p.W;
#pragma unroll
            for (int c = 0; c < NCH; ++c) {
                f32x4 o[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) o[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    f32x4 pr[6];
#pragma unroll
                    for (int d = 0; d < 6; ++d) {
                        const float dd = dv[i][d];
                        const f32x4 u = __builtin_elementwise_fma(f32x4{dd, dd, dd, dd}, ga[c], gt[c]);   // fmaf per channel, two to an instruction
#pragma unroll
                        for (int ch = 0; ch < 4; ++ch) pr[d][ch] = __builtin_amdgcn_fmed3f(u[ch], 0.f, 6.f);
                        if (BORDER) {
                            const bool ok = rowok[i] && (d == 0 ? c0ok : (d == 5 ? c5ok : true));
                            if (!ok) pr[d] = f32x4{0.f, 0.f, 0.f, 0.f};
                        }
                    }
#pragma unroll
                    for (int j = 0; j < 4; ++j)
#pragma unroll
                        for (int d = 0; d < 3; ++d) o[j] += wk[c][i * 3 + d] * pr[j + d];
                }
                auto Ac = reinterpret_cast<uint16_t(*)[BM][LDK]>(smem + A_OFF + c * A_CHUNK);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int r = ty * TW + tx0 + j;
                    unsigned h0, l0, h1, l1;
                    split2(o[j][0], o[j][1], h0, l0);
                    split2(o[j][2], o[j][3], h1, l1);
                    *reinterpret_cast<u32x2*>(&Ac[0][r][c4 * 4]) = u32x2{h0, h1};
                    *reinterpret_cast<u32x2*>(&Ac[1][r][c4 * 4]) = u32x2{l0, l1};
                }
            }
        };
        if (y0 == 0 || y0 + TH == p.H || x0 == 0 || x0 + TW == p.W) stage1(std::true_type{});
        else stage1(std::false_type{});
        // The epilogue's operands are requested here: they land under the MFMA phase and are not live in the stage above.  The loads are
        // unconditional (threads past the last channel quad read quad 0): a load that may still be pending on some path at the loop's head
        // costs a wait for ALL outstanding memory operations there, the stores of the tile before included.
        const int ncl = ncol < p.N ? ncol : 0;
        f32x4 rve[RES ? E_NROWS : 1];
        if constexpr (RES) {
            const float* __restrict__ rt = p.res + (img + (long)y0 * p.W) * p.ldres + ncl;
#pragma unroll
            for (int k = 0; k < E_NROWS; ++k) {
                const int r = er + k * E_RPP;
                rve[k] = *reinterpret_cast<const f32x4*>(rt + ((r >> 4) * p.W + (r & 15) + x0) * p.ldres);
            }
        }
        // (the affine vectors are re-read per tile: as loop-invariant registers they would not fit beside the weights)
        const bool two = p.scale2 != nullptr;
        f32x4 s1 = *reinterpret_cast<const f32x4*>(p.scale1 + ncl);
        f32x4 t1 = *reinterpret_cast<const f32x4*>(p.shift1 + ncl);
        f32x4 s2 = *reinterpret_cast<const f32x4*>((two ? p.scale2 : p.scale1) + ncl);
        f32x4 t2 = *reinterpret_cast<const f32x4*>((two ? p.shift2 : p.shift1) + ncl);
        __syncthreads();  // (2) A planes visible
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            auto Ac = reinterpret_cast<const uint16_t(*)[BM][LDK]>(smem + A_OFF + c * A_CHUNK);
            auto Bc = reinterpret_cast<const uint16_t(*)[BN][LDK]>(smem + c * B_CHUNK);
#pragma unroll
            for (int ks = 0; ks < BK / 16; ++ks) {
                const int r = wv * 32 + fr;
                const bf16x8 ah = *reinterpret_cast<const bf16x8*>(&Ac[0][r][ks * 16 + fh * 8]);
                const bf16x8 al = *reinterpret_cast<const bf16x8*>(&Ac[1][r][ks * 16 + fh * 8]);
                bf16x8 bh[2], bl[2];
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    bh[j] = *reinterpret_cast<const bf16x8*>(&Bc[0][j * 32 + fr][ks * 16 + fh * 8]);
                    bl[j] = *reinterpret_cast<const bf16x8*>(&Bc[1][j * 32 + fr][ks * 16 + fh * 8]);
                }
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh[j], acc[j], 0, 0, 0);
                    acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl[j], acc[j], 0, 0, 0);
                    acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh[j], acc[j], 0, 0, 0);
                }
            }
        }
        if (more) form_d(x0 + TW, (t + 1) & 1);   // (that half was last read a tile ago)
        __syncthreads();  // (3) fragment reads done: the staging tile overwrites the A planes

        // ---- epilogue (sep_fused_kernel's, 64 columns, fp32 output)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int r = wv * 32 + (e & 3) + 8 * (e >> 2) + 4 * fh;
                stage[r][j * 32 + fr] = acc[j][e];
                acc[j][e] = 0.f;
            }
        __syncthreads();
        // (the operands requested before barrier (2) are taken as arrived HERE, on every path, before the stores are issued)
        asm volatile("" : "+v"(s1), "+v"(t1), "+v"(s2), "+v"(t2));
        if constexpr (RES) {
#pragma unroll
            for (int k = 0; k < E_NROWS; ++k) asm volatile("" : "+v"(rve[k]));
        }
        if (ncol < p.N) {
            const float hi = p.act == 1 ? 6.f : __builtin_inff();
            const float hi2 = p.act == 2 ? __builtin_inff() : 6.f;
            const float slope = p.act == 4 ? 0.2f : 1.f, lo = (p.act == 1 || p.act == 2) ? 0.f : -__builtin_inff();
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
            float* __restrict__ ytile = p.y + (img + (long)y0 * p.W) * p.ldy + ncl;
#pragma unroll
            for (int k = 0; k < E_NROWS; ++k) {
                const int r = er + k * E_RPP;
                f32x4 v = finish(*reinterpret_cast<const f32x4*>(&stage[r][ncl]));
                if constexpr (RES) v = v + rve[k];
                float* dst = ytile + ((r >> 4) * p.W + (r & 15) + x0) * p.ldy;
                if (p.nt) store_nt16(dst, v);
                else *reinterpret_cast<f32x4*>(dst) = v;
            }
        }
        __syncthreads();  // the staging tile is read out before the next tile's A planes overwrite it
    }
}

template <int BN>
int launch_bn(const SepParams& q, const SepPlan& plan, hipStream_t st) {
    if (q.gen_a) {
        if (plan.passes == 3)
            hipLaunchKernelGGL((sep_fused_kernel<BN, 3, true>), plan.grid, dim3(256), 0, st, q);
        else
            hipLaunchKernelGGL((sep_fused_kernel<BN, 1, true>), plan.grid, dim3(256), 0, st, q);
    } else if (plan.passes == 3)
        hipLaunchKernelGGL((sep_fused_kernel<BN, 3, false>), plan.grid, dim3(256), 0, st, q);
    else
        hipLaunchKernelGGL((sep_fused_kernel<BN, 1, false>), plan.grid, dim3(256), 0, st, q);
    return emd::check_launch("sep_fused_kernel");
}

}  // namespace

// The plan's route -> the instance (sep_entry.hip made the plan and filled q from it).  The order of the launch sites is the order of the
// kernels in the code object.
int emd::sep_fused_launch(const SepParams& q, const SepPlan& plan, hipStream_t st) {
    const dim3 grid = plan.grid;
    switch (plan.route) {
    case kSepFusedWres:   // BN = 64, Cin <= 64, split-bf16: the pointwise weights stay in LDS for the workgroup's whole life
        if (q.gen_a) hipLaunchKernelGGL((sep_fused_kernel<64, 3, true, 8, false, true>), grid, dim3(256), 0, st, q);
        else hipLaunchKernelGGL((sep_fused_kernel<64, 3, false, 8, false, true>), grid, dim3(256), 0, st, q);
        return emd::check_launch("sep_fused_kernel<resident W>");
    case kSepGen9:   // the generated-input layer fed by the 1-channel image itself
        if (q.Cin == 64) {
            if (q.res) hipLaunchKernelGGL((sep_gen9_kernel<2, true>), grid, dim3(256), 0, st, q);
            else hipLaunchKernelGGL((sep_gen9_kernel<2, false>), grid, dim3(256), 0, st, q);
        } else if (q.res) {
            hipLaunchKernelGGL((sep_gen9_kernel<1, true>), grid, dim3(256), 0, st, q);
        } else {
            hipLaunchKernelGGL((sep_gen9_kernel<1, false>), grid, dim3(256), 0, st, q);
        }
        return emd::check_launch("sep_gen9_kernel");
    case kSepFusedDual:   // 64 | 64 columns on 8 x 16 pixel tiles, or 128 | 128 columns on 4 x 16 pixel tiles
        if (plan.th == 4)
            hipLaunchKernelGGL((sep_fused_kernel<256, 3, false, 4, true>), grid, dim3(256), 0, st, q);
        else
            hipLaunchKernelGGL((sep_fused_kernel<128, 3, false, 8, true>), grid, dim3(256), 0, st, q);
        return emd::check_launch("sep_fused_kernel<dual>");
    case kSepFusedWide:   // one N tile of 256 columns on 4 x 16 pixel tiles, no generated input
        if (plan.passes == 3) hipLaunchKernelGGL((sep_fused_kernel<256, 3, false, 4, false>), grid, dim3(256), 0, st, q);
        else hipLaunchKernelGGL((sep_fused_kernel<256, 1, false, 4, false>), grid, dim3(256), 0, st, q);
        return emd::check_launch("sep_fused_kernel<wide>");
    default:
        return q.N <= 64 ? launch_bn<64>(q, plan, st) : launch_bn<128>(q, plan, st);
    }
}
