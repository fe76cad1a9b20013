// Implicit-GEMM convolutions on the matrix cores from split32 activations (the layout: gemm_split.hip), on the LDS-DMA pipeline of the
// pointwise GEMM there: the dense 3x3 conv as a 9-tap GEMM (gemm_split_conv_kernel, emd_conv3x3_split32_f32) and
// slim.conv2d_transpose(k = 3, s = 2) as GEMM (deconv4_split_kernel, deconv4_half_kernel, the emd_deconv3x3s2_* entry points and
// their routing to the patch-resident kernels conv3_pipe.hip / deconv_pipe.hip).
#include <cstdlib>

#include "conv_plan.hpp"

namespace {

using namespace emd;

// Implicit-GEMM convolutions from split32 activations: dense 3x3 (stride 1/2, dilation), the four output phases of the
// 3x3 stride-2 transposed convolution, strided 1x1 -- the row map and tap list of gemm_conv.hip on the pipelined LDS-DMA
// structure of gemm_split_kernel (gemm_split.hip).  K runs over (tap, 32-channel step); the DMA source of an A row is the tap's source pixel, or a line of
// zeros for TF-SAME padding and rows beyond M (an 8 KB zero buffer, so that "+ K step" needs no per-row select).  The
// row -> destination pixel table lives in LDS behind the staging tile.  Output: fp32 NHWC, or split32 (out_split) when the
// consumer is another of these GEMMs -- a chain of convolutions then never materialises an fp32 activation.
__device__ __attribute__((aligned(128))) unsigned char g_zero_buf[8192];

// BN = 128: 2 x 2 MFMA tiles per wave, 3 stages.  BN = 64 (the 64-channel 512^2 layers): 2 x 1 tiles per wave, a K step is half
// as long, so 4 stages (the whole 160 KB) keep the DMA three K steps ahead and one of its groups may stay in flight across the barrier.
template <int BN, bool FOUR = false>
__global__ __launch_bounds__(512, 2) void gemm_split_conv_kernel(const SplitConvParams cp) {
    const SplitGemmParams& p = cp.g;
    constexpr int BM = 256, NS = BN == 128 ? 3 : 4, WQ = BN / 64, TN = BN / 64;
    constexpr int A_STAGE = BM * 128, W_STAGE = BN * 128, STAGE = A_STAGE + W_STAGE;
    constexpr int EPI_LD = BN + 4;
    constexpr int EPI_BYTES = BM * EPI_LD * 4;
    constexpr int SMEM_BYTES = NS * STAGE > EPI_BYTES + BM * 8 ? NS * STAGE : EPI_BYTES + BM * 8;
    __shared__ __attribute__((aligned(1024))) unsigned char smem[SMEM_BYTES];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wv = tid >> 6;
    const int wm = wv >> 1, wn = wv & 1;
    const int nblk = p.n_mtiles * p.n_ntiles;
    int bid = blockIdx.x;
    {
        const int q = nblk >> 3, r = nblk & 7, xcd = bid & 7, loc = bid >> 3;
        bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + loc;
    }
    const int mt = bid / p.n_ntiles, nt = bid % p.n_ntiles;
    const long m0 = (long)mt * BM;
    const int n0 = nt * BN;

    // this lane's four DMA rows: grid position (b, i, j) of row m, kept as (pixel index of (b,0,0) in the source, i, j)
    const int drow = lane >> 3, dchunk = lane & 7;
    int pi[4], pj[4], pb[4], pc[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int row = wv * 32 + q * 8 + drow;
        pc[q] = (dchunk ^ ((row >> 1) & 7)) * 16;
        const long m = m0 + row;
        if (m < p.M) {
            if (cp.flat) {
                pi[q] = 0; pj[q] = 0; pb[q] = (int)m;
            } else {
                const int j = (int)(m % cp.Wg);
                const long t = m / cp.Wg;
                pi[q] = (int)(t % cp.Hg); pj[q] = j; pb[q] = (int)(t / cp.Hg) * cp.Ha * cp.Wa;
            }
        } else {
            pi[q] = -(1 << 20); pj[q] = 0; pb[q] = 0;    // beyond M: every tap reads zeros
        }
    }
    const int fr = lane & 31, fh = lane >> 5;
    const int sw = (fr >> 1) & 7;
    const int a_off = (wm * 64 + fr) * 128;
    const int w_off = A_STAGE + (wn * (BN / 2) + fr) * 128;
#pragma unroll 1
    for (int ph = 0; ph < (FOUR ? 4 : 1); ++ph) {
    const uint16_t* __restrict__ Whi = FOUR ? cp.Whi4[ph] : p.Whi;
    const uint16_t* __restrict__ Wlo = FOUR ? cp.Wlo4[ph] : p.Wlo;
    const int ntaps = FOUR ? cp.ntaps4[ph] : cp.ntaps;
    const unsigned long long dyp = FOUR ? cp.dyp4[ph] : cp.dyp, dxp = FOUR ? cp.dxp4[ph] : cp.dxp;
    const int py = FOUR ? (ph >> 1) : cp.py, px = FOUR ? (ph & 1) : cp.px;
    const int Ktot = FOUR ? ntaps * cp.Cpad : p.Ktot;
    const unsigned char* asrc[4];
    auto set_tap = [&](int tap) {
        const int dy = (int)((dyp >> (7 * tap)) & 127) - 64, dx = (int)((dxp >> (7 * tap)) & 127) - 64;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            long pix;
            bool ok;
            if (cp.flat) {
                pix = pb[q];
                ok = pi[q] >= 0;
            } else {
                const int iy = pi[q] * cp.sa + dy, ix = pj[q] * cp.sa + dx;
                ok = iy >= 0 && iy < cp.Ha && ix >= 0 && ix < cp.Wa;
                pix = (long)pb[q] + (long)iy * cp.Wa + ix;
            }
            asrc[q] = (ok ? p.A + pix * p.lda_bytes : g_zero_buf) + pc[q];
        }
    };
    const unsigned char* wsrc[WQ];
#pragma unroll
    for (int q = 0; q < WQ; ++q) {
        const int row = wv * (WQ * 8) + q * 8 + drow;
        const int c = dchunk ^ ((row >> 1) & 7);
        const uint16_t* plane = (c & 4) ? Wlo : Whi;
        wsrc[q] = reinterpret_cast<const unsigned char*>(plane + (long)(n0 + row) * Ktot + (c & 3) * 8);
    }
    auto issue = [&](int stage, int tap, int kc) {
        unsigned char* sb = smem + stage * STAGE;
#pragma unroll
        for (int q = 0; q < 4; ++q)
            __builtin_amdgcn_global_load_lds((gptr_t)(asrc[q] + (long)kc * 128), (lptr_t)(sb + (wv * 32 + q * 8) * 128), 16, 0, 0);
        const long wk = ((long)tap * cp.Cpad + (long)kc * 32) * 2;
#pragma unroll
        for (int q = 0; q < WQ; ++q)
            __builtin_amdgcn_global_load_lds((gptr_t)(wsrc[q] + wk), (lptr_t)(sb + A_STAGE + (wv * (WQ * 8) + q * 8) * 128), 16, 0, 0);
    };

    f32x16 acc[2][TN];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    struct Frags { bf16x8 ah[2], al[2], bh[TN], bl[TN]; };
    auto load_frags = [&](Frags& f, const unsigned char* sb, int ks) {
        const int ch = ((ks * 2 + fh) ^ sw) << 4;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            f.ah[i] = *reinterpret_cast<const bf16x8*>(sb + a_off + i * 4096 + ch);
            f.al[i] = *reinterpret_cast<const bf16x8*>(sb + a_off + i * 4096 + (ch ^ 64));
        }
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            f.bh[j] = *reinterpret_cast<const bf16x8*>(sb + w_off + j * 4096 + ch);
            f.bl[j] = *reinterpret_cast<const bf16x8*>(sb + w_off + j * 4096 + (ch ^ 64));
        }
    };
    auto mfma12 = [&](const Frags& f) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f.al[i], f.bh[j], acc[i][j], 0, 0, 0);
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f.ah[i], f.bl[j], acc[i][j], 0, 0, 0);
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f.ah[i], f.bh[j], acc[i][j], 0, 0, 0);
            }
    };

    // (dtap, dkc): the K step the next DMA fetches; it stops advancing at the last one (the two surplus issues at the end
    // re-read it into a stage nobody computes on)
    const int total = ntaps * cp.nkc;
    int dtap = 0, dkc = 0, dstep = 0;
    auto advance = [&]() {
        if (dstep + 1 < total) {
            ++dstep;
            if (++dkc == cp.nkc) {
                dkc = 0;
                ++dtap;
                set_tap(dtap);
            }
        }
    };
    set_tap(0);
#pragma unroll
    for (int s = 0; s < NS - 1; ++s) {
        issue(s, dtap, dkc);
        advance();
    }
    // K steps 0 and 1 landed; NS-3 younger DMA groups (4 + WQ pieces each) may stay in flight across every barrier
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"((NS - 3) * (4 + WQ)) : "memory");
    __builtin_amdgcn_s_barrier();
    Frags f0, f1;
    load_frags(f0, smem, 0);
    int s0 = 0, s1 = 1, s2 = NS - 1;   // stage of K step st / st+1 / the one being refilled (held step st-1)
    for (int st = 0; st < total; ++st) {
        if (st > 0) {
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"((NS - 3) * (4 + WQ)) : "memory");
            __builtin_amdgcn_s_barrier();
        }
        issue(s2, dtap, dkc);
        load_frags(f1, smem + s0 * STAGE, 1);
        mfma12(f0);
        load_frags(f0, smem + s1 * STAGE, 0);
        mfma12(f1);
        if constexpr (TN == 2) {
#pragma unroll
            for (int g = 0; g < 6; ++g) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x010, 1, 0);
            }
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
            }
            __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
#pragma unroll
            for (int g = 0; g < 8; ++g) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
            }
            __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
        } else {   // 6 MFMAs per half step: 5 DMA pieces, then the 6 reads of f1; second half: the 6 reads of the next f0
#pragma unroll
            for (int g = 0; g < 3; ++g) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x010, 2, 0);
            }
#pragma unroll
            for (int g = 0; g < 2; ++g) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x100, 3, 0);
            }
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
#pragma unroll
            for (int g = 0; g < 3; ++g) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
            }
            __builtin_amdgcn_sched_group_barrier(0x008, 3, 0);
        }
        s2 = s0;                                   // the stage just computed on is refilled next
        s0 = s1;
        s1 = s1 + 1 == NS ? 0 : s1 + 1;
        __builtin_amdgcn_sched_barrier(0);
        advance();
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    // ---- epilogue: accumulators -> fp32 LDS tile; row -> destination pixel table behind it
    float(*stage)[EPI_LD] = reinterpret_cast<float(*)[EPI_LD]>(smem);
    long long* rowP = reinterpret_cast<long long*>(smem + EPI_BYTES);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int r = wm * 64 + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * fh;
                stage[r][wn * (BN / 2) + j * 32 + fr] = acc[i][j][e];
            }
    if (tid < BM) {
        const long m = m0 + tid;
        long long dst = -1;
        if (m < p.M) {
            if (cp.flat) {
                dst = m;
            } else {
                const int j = (int)(m % cp.Wg);
                const long t = m / cp.Wg;
                const int i = (int)(t % cp.Hg);
                const long b = t / cp.Hg;
                dst = (b * cp.Hc + (i * cp.sc + py)) * (long)cp.Wc + (j * cp.sc + px);
            }
        }
        rowP[tid] = dst;
    }
    __syncthreads();
    constexpr int C4 = BN / 4;
    constexpr int ROWS_PER_PASS = 512 / C4;
    const int ec = (tid % C4) * 4, er = tid / C4;
    const int n = n0 + ec;
    const int Np = cp.out_split ? (p.N + 31) / 32 * 32 : p.N;   // split32 output: the padding channels are written (zeros)
    if (n < Np) {
        const bool real = n < p.N;                               // N % 4 == 0: a chunk is all inside or all outside
        float4 s1 = make_float4(0.f, 0.f, 0.f, 0.f), t1 = s1, s2 = make_float4(1.f, 1.f, 1.f, 1.f), t2 = s1;
        if (real) {
            s1 = *reinterpret_cast<const float4*>(p.scale1 + n);
            t1 = *reinterpret_cast<const float4*>(p.shift1 + n);
            if (p.scale2) {
                s2 = *reinterpret_cast<const float4*>(p.scale2 + n);
                t2 = *reinterpret_cast<const float4*>(p.shift2 + n);
            }
        }
        const float* __restrict__ resp = real ? p.res : nullptr;
        const float hi = p.act == 1 ? 6.f : __builtin_inff();
        const float hi2 = p.act == 2 ? __builtin_inff() : 6.f;   // second stage (extra BN): relu6, or relu with act code relu
        const float slope = p.act == 4 ? 0.2f : 1.f, lo = (p.act == 1 || p.act == 2) ? 0.f : -__builtin_inff();   // v = min(max(max(v, lo), slope*v), hi): every act code
#pragma unroll 4
        for (int r = er; r < BM; r += ROWS_PER_PASS) {
            const long long pix = rowP[r];
            if (pix < 0) continue;
            float4 v = *reinterpret_cast<const float4*>(&stage[r][ec]);
            float4 rv = make_float4(0.f, 0.f, 0.f, 0.f);
            if (resp) rv = *reinterpret_cast<const float4*>(resp + pix * p.ldres + n);
            v.x = fmaf(v.x, s1.x, t1.x); v.y = fmaf(v.y, s1.y, t1.y); v.z = fmaf(v.z, s1.z, t1.z); v.w = fmaf(v.w, s1.w, t1.w);
            v.x = fminf(fmaxf(fmaxf(v.x, lo), slope * v.x), hi); v.y = fminf(fmaxf(fmaxf(v.y, lo), slope * v.y), hi);
            v.z = fminf(fmaxf(fmaxf(v.z, lo), slope * v.z), hi); v.w = fminf(fmaxf(fmaxf(v.w, lo), slope * v.w), hi);
            if (p.scale2) {
                v.x = fminf(fmaxf(fmaf(v.x, s2.x, t2.x), 0.f), hi2); v.y = fminf(fmaxf(fmaf(v.y, s2.y, t2.y), 0.f), hi2);
                v.z = fminf(fmaxf(fmaf(v.z, s2.z, t2.z), 0.f), hi2); v.w = fminf(fmaxf(fmaf(v.w, s2.w, t2.w), 0.f), hi2);
            }
            v.x += rv.x; v.y += rv.y; v.z += rv.z; v.w += rv.w;
            if (!real) v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (cp.out_split) {
                // 16-byte stores through an exchange between the two lanes of a channel-quad pair (see emd::dw_store): both
                // lanes of a pair share the row and the n < Np test (Np is a multiple of 32)
                unsigned h0, l0, h1, l1;
                split2(v.x, v.y, h0, l0);
                split2(v.z, v.w, h1, l1);
                const int q = n >> 2;
                const bool odd = q & 1;
                const unsigned r0 = emd::swap_pair(odd ? h0 : l0), r1 = emd::swap_pair(odd ? h1 : l1);
                unsigned char* g = reinterpret_cast<unsigned char*>(p.C) + pix * (long)p.ldc * 4 + (n >> 5) * 128;
                u32x4* dst = reinterpret_cast<u32x4*>(!odd ? g + (q & 7) * 8 : g + 64 + ((q - 1) & 7) * 8);
                const u32x4 val = !odd ? u32x4{h0, h1, r0, r1} : u32x4{r0, r1, l0, l1};
                if (p.nt) store_nt16(dst, val);
                else *dst = val;
            } else if (p.nt) {
                store_nt16(p.C + pix * p.ldc + n, f32x4{v.x, v.y, v.z, v.w});
            } else {
                *reinterpret_cast<float4*>(p.C + pix * p.ldc + n) = v;
            }
        }
    }
    if (FOUR) __syncthreads();   // the staging tile and the row table are read out before the next phase's DMA lands on them
    }   // phase loop
}

// slim.conv2d_transpose(k = 3, s = 2) (machine_learning/denoiser.py:138-150) as ONE launch, round 3 form: the four output phases of a
// workgroup's 256 input pixels back to back as in gemm_split_conv_kernel<BN, true> (same K loops, same products in the same order:
// bit-identical), but the epilogue leaves straight from the accumulators (quad transpose, 16-byte non-temporal stores) and touches no
// LDS -- so the DMA of the NEXT phase's first K steps is issued before the stores of this one, and the stores (the layer writes four
// times what it reads: 4.3 GB for deconv1to0) drain under the next K loop instead of between two of them.  fp32 output, no residual.
template <int BN>
__global__ __launch_bounds__(512, 2) void deconv4_split_kernel(const SplitConvParams cp) {
    const SplitGemmParams& p = cp.g;
    constexpr int BM = 256, NS = BN == 128 ? 3 : 4, WQ = BN / 64, TN = BN / 64;
    constexpr int A_STAGE = BM * 128, W_STAGE = BN * 128, STAGE = A_STAGE + W_STAGE;
    constexpr int E = 8 * TN;   // stores per wave and phase
    __shared__ __attribute__((aligned(1024))) unsigned char smem[NS * STAGE];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wv = tid >> 6;
    const int wm = wv >> 1, wn = wv & 1;
    const int nblk = p.n_mtiles * p.n_ntiles;
    int bid = blockIdx.x;
    {
        const int q = nblk >> 3, r = nblk & 7, xcd = bid & 7, loc = bid >> 3;
        bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + loc;
    }
    const int mt = bid / p.n_ntiles, nt = bid % p.n_ntiles;
    const long m0 = (long)mt * BM;
    const int n0 = nt * BN;

    const int drow = lane >> 3, dchunk = lane & 7;
    int pi[4], pj[4], pb[4], pc[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int row = wv * 32 + q * 8 + drow;
        pc[q] = (dchunk ^ ((row >> 1) & 7)) * 16;
        const long m = m0 + row;
        if (m < p.M) {
            const int j = (int)(m % cp.Wg);
            const long t = m / cp.Wg;
            pi[q] = (int)(t % cp.Hg); pj[q] = j; pb[q] = (int)(t / cp.Hg) * cp.Ha * cp.Wa;
        } else {
            pi[q] = -(1 << 20); pj[q] = 0; pb[q] = 0;    // beyond M: every tap reads zeros
        }
    }
    const int fr = lane & 31, fh = lane >> 5;
    const int sw = (fr >> 1) & 7;
    const int a_off = (wm * 64 + fr) * 128;
    const int w_off = A_STAGE + (wn * (BN / 2) + fr) * 128;

    // ---- epilogue roles.  Before the transpose a lane holds channel n0 + wn BN/2 + 32 j + fr of rows (e & 3) + 8 (e >> 2) + 4 fh;
    // after it, row 8 q + 4 fh + li and channels 4 cq .. 4 cq + 3 of the 32-column group
    const int li = fr & 3, cq = fr >> 2;
    long dst0[2][4];     // output pixel of phase (0, 0) for this lane's rows, -1 beyond M
    bool full = true;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const long m = m0 + wm * 64 + i * 32 + 8 * q + 4 * fh + li;
            long d = -1;
            if (m < p.M) {
                const int j = (int)(m % cp.Wg);
                const long t = m / cp.Wg;
                d = ((t / cp.Hg) * cp.Hc + (t % cp.Hg) * 2) * (long)cp.Wc + 2 * j;
            }
            dst0[i][q] = d;
            full = full && d >= 0;
        }
    float es1[TN], et1[TN];
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int n = n0 + wn * (BN / 2) + j * 32 + fr;
        es1[j] = n < p.N ? p.scale1[n] : 0.f;
        et1[j] = n < p.N ? p.shift1[n] : 0.f;
        asm volatile("" ::"v"(es1[j]), "v"(et1[j]));   // waited for here, not behind the DMA groups in the loop
        full = full && (n0 + wn * (BN / 2) + j * 32 + 31 < p.N);
    }
    full = __builtin_amdgcn_readfirstlane(__builtin_amdgcn_ballot_w64(!full) == 0);   // per wave: no masked store, the store count is exact
    const float hi = p.act == 1 ? 6.f : __builtin_inff();
    const float slope = p.act == 4 ? 0.2f : 1.f, lo = (p.act == 1 || p.act == 2) ? 0.f : -__builtin_inff();

    // ---- per-phase state
    const uint16_t* __restrict__ Whi = cp.Whi4[0];
    const uint16_t* __restrict__ Wlo = cp.Wlo4[0];
    int ntaps = cp.ntaps4[0];
    unsigned long long dyp = cp.dyp4[0], dxp = cp.dxp4[0];
    const unsigned char* asrc[4];
    const unsigned char* wsrc[WQ];
    auto set_tap = [&](int tap) {
        const int dy = (int)((dyp >> (7 * tap)) & 127) - 64, dx = (int)((dxp >> (7 * tap)) & 127) - 64;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int iy = pi[q] * cp.sa + dy, ix = pj[q] * cp.sa + dx;
            const bool ok = iy >= 0 && iy < cp.Ha && ix >= 0 && ix < cp.Wa;
            const long pix = (long)pb[q] + (long)iy * cp.Wa + ix;
            asrc[q] = (ok ? p.A + pix * p.lda_bytes : g_zero_buf) + pc[q];
        }
    };
    auto set_phase = [&](int ph) {
        Whi = cp.Whi4[ph]; Wlo = cp.Wlo4[ph]; ntaps = cp.ntaps4[ph]; dyp = cp.dyp4[ph]; dxp = cp.dxp4[ph];
        const int Ktot = ntaps * cp.Cpad;
#pragma unroll
        for (int q = 0; q < WQ; ++q) {
            const int row = wv * (WQ * 8) + q * 8 + drow;
            const int c = dchunk ^ ((row >> 1) & 7);
            const uint16_t* plane = (c & 4) ? Wlo : Whi;
            wsrc[q] = reinterpret_cast<const unsigned char*>(plane + (long)(n0 + row) * Ktot + (c & 3) * 8);
        }
    };
    auto issue = [&](int stage, int tap, int kc) {
        unsigned char* sb = smem + stage * STAGE;
#pragma unroll
        for (int q = 0; q < 4; ++q)
            __builtin_amdgcn_global_load_lds((gptr_t)(asrc[q] + (long)kc * 128), (lptr_t)(sb + (wv * 32 + q * 8) * 128), 16, 0, 0);
        const long wk = ((long)tap * cp.Cpad + (long)kc * 32) * 2;
#pragma unroll
        for (int q = 0; q < WQ; ++q)
            __builtin_amdgcn_global_load_lds((gptr_t)(wsrc[q] + wk), (lptr_t)(sb + A_STAGE + (wv * (WQ * 8) + q * 8) * 128), 16, 0, 0);
    };

    f32x16 acc[2][TN];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    struct Frags { bf16x8 ah[2], al[2], bh[TN], bl[TN]; };
    auto load_frags = [&](Frags& f, const unsigned char* sb, int ks) {
        const int ch = ((ks * 2 + fh) ^ sw) << 4;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            f.ah[i] = *reinterpret_cast<const bf16x8*>(sb + a_off + i * 4096 + ch);
            f.al[i] = *reinterpret_cast<const bf16x8*>(sb + a_off + i * 4096 + (ch ^ 64));
        }
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            f.bh[j] = *reinterpret_cast<const bf16x8*>(sb + w_off + j * 4096 + ch);
            f.bl[j] = *reinterpret_cast<const bf16x8*>(sb + w_off + j * 4096 + (ch ^ 64));
        }
    };
    auto mfma12 = [&](const Frags& f) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f.al[i], f.bh[j], acc[i][j], 0, 0, 0);
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f.ah[i], f.bl[j], acc[i][j], 0, 0, 0);
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f.ah[i], f.bh[j], acc[i][j], 0, 0, 0);
            }
    };

    int total = 0, dtap = 0, dkc = 0, dstep = 0;
    auto advance = [&]() {
        if (dstep + 1 < total) {
            ++dstep;
            if (++dkc == cp.nkc) {
                dkc = 0;
                ++dtap;
                set_tap(dtap);
            }
        }
    };
    auto prologue = [&](int ph) {   // the first NS - 1 K steps of phase ph into stages 0 .. NS - 2
        set_phase(ph);
        total = ntaps * cp.nkc;
        dtap = dkc = dstep = 0;
        set_tap(0);
#pragma unroll
        for (int s = 0; s < NS - 1; ++s) {
            issue(s, dtap, dkc);
            advance();
        }
    };
    prologue(0);
#pragma unroll 1
    for (int ph = 0; ph < 4; ++ph) {
        // K steps 0 and 1 landed; NS-3 younger DMA groups (4 + WQ pieces each) may stay in flight across every barrier -- and, from the
        // second phase on, the previous phase's E stores, which were issued after this phase's first groups
        if (ph > 0 && full) asm volatile("s_waitcnt vmcnt(%0)" ::"n"((NS - 3) * (4 + WQ) + E) : "memory");
        else asm volatile("s_waitcnt vmcnt(%0)" ::"n"((NS - 3) * (4 + WQ)) : "memory");
        __builtin_amdgcn_s_barrier();
        Frags f0, f1;
        load_frags(f0, smem, 0);
        int s0 = 0, s1 = 1, s2 = NS - 1;
        for (int st = 0; st < total; ++st) {
            if (st > 0) {
                asm volatile("s_waitcnt vmcnt(%0)" ::"n"((NS - 3) * (4 + WQ)) : "memory");
                __builtin_amdgcn_s_barrier();
            }
            issue(s2, dtap, dkc);
            load_frags(f1, smem + s0 * STAGE, 1);
            mfma12(f0);
            load_frags(f0, smem + s1 * STAGE, 0);
            mfma12(f1);
            if constexpr (TN == 2) {
#pragma unroll
                for (int g = 0; g < 6; ++g) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(0x010, 1, 0);
                }
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
                }
                __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
#pragma unroll
                for (int g = 0; g < 8; ++g) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
                }
                __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
            } else {
#pragma unroll
                for (int g = 0; g < 3; ++g) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(0x010, 2, 0);
                }
#pragma unroll
                for (int g = 0; g < 2; ++g) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(0x100, 3, 0);
                }
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
#pragma unroll
                for (int g = 0; g < 3; ++g) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
                }
                __builtin_amdgcn_sched_group_barrier(0x008, 3, 0);
            }
            s2 = s0;
            s0 = s1;
            s1 = s1 + 1 == NS ? 0 : s1 + 1;
            __builtin_amdgcn_sched_barrier(0);
            advance();
        }
        // every wave's fragment reads are done and this wave's surplus DMA groups have landed: the stages are free for the next phase
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        const int py = ph >> 1, px = ph & 1;
        if (ph < 3) prologue(ph + 1);
        // ---- epilogue of phase ph, straight from the accumulators
        const long poff = (long)py * cp.Wc + px;
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int n4 = n0 + wn * (BN / 2) + j * 32 + 4 * cq;
            const bool ncol = n4 < p.N;
            const float s1 = es1[j], t1 = et1[j];
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    float r[4];
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const float u = fmaf(acc[i][j][4 * q + k], s1, t1);
                        r[k] = fminf(fmaxf(fmaxf(u, lo), slope * u), hi);
                    }
                    quad_transpose(r, li);
                    if (ncol && dst0[i][q] >= 0) store_nt16(p.C + (dst0[i][q] + poff) * p.ldc + n4, f32x4{r[0], r[1], r[2], r[3]});
                }
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// The same transposed conv on 128-row tiles, 4 waves, two LDS stages (64 KB at BN = 128): TWO workgroups per CU.  vmcnt retires in
// order, so a workgroup's output stores (four times the bytes it reads) hold up its own next K loop whatever the issue order -- here
// the partner workgroup's K loop runs meanwhile.  Same wave tile (64 x 64), same products in the same order along K: bit-identical
// to deconv4_split_kernel.  One K step of DMA in flight (two stages), fragments read after the step's barrier.
template <int BN>
__global__ __launch_bounds__(256, 2) void deconv4_half_kernel(const SplitConvParams cp) {
    const SplitGemmParams& p = cp.g;
    constexpr int BM = 128, NS = 2, WQ = BN / 32, TN = BN / 64;
    constexpr int A_STAGE = BM * 128, W_STAGE = BN * 128, STAGE = A_STAGE + W_STAGE;
    constexpr int E = 8 * TN;   // stores per wave and phase
    __shared__ __attribute__((aligned(1024))) unsigned char smem[NS * STAGE];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wv = tid >> 6;
    const int wm = wv >> 1, wn = wv & 1;
    const int nblk = p.n_mtiles * p.n_ntiles;
    int bid = blockIdx.x;
    {
        const int q = nblk >> 3, r = nblk & 7, xcd = bid & 7, loc = bid >> 3;
        bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + loc;
    }
    const int mt = bid / p.n_ntiles, nt = bid % p.n_ntiles;
    const long m0 = (long)mt * BM;
    const int n0 = nt * BN;

    const int drow = lane >> 3, dchunk = lane & 7;
    int pi[4], pj[4], pb[4], pc[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int row = wv * 32 + q * 8 + drow;
        pc[q] = (dchunk ^ ((row >> 1) & 7)) * 16;
        const long m = m0 + row;
        if (m < p.M) {
            const int j = (int)(m % cp.Wg);
            const long t = m / cp.Wg;
            pi[q] = (int)(t % cp.Hg); pj[q] = j; pb[q] = (int)(t / cp.Hg) * cp.Ha * cp.Wa;
        } else {
            pi[q] = -(1 << 20); pj[q] = 0; pb[q] = 0;    // beyond M: every tap reads zeros
        }
    }
    const int fr = lane & 31, fh = lane >> 5;
    const int sw = (fr >> 1) & 7;
    const int a_off = (wm * 64 + fr) * 128;
    const int w_off = A_STAGE + (wn * (BN / 2) + fr) * 128;

    // ---- epilogue roles.  Before the transpose a lane holds channel n0 + wn BN/2 + 32 j + fr of rows (e & 3) + 8 (e >> 2) + 4 fh;
    // after it, row 8 q + 4 fh + li and channels 4 cq .. 4 cq + 3 of the 32-column group
    const int li = fr & 3, cq = fr >> 2;
    long dst0[2][4];     // output pixel of phase (0, 0) for this lane's rows, -1 beyond M
    bool full = true;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const long m = m0 + wm * 64 + i * 32 + 8 * q + 4 * fh + li;
            long d = -1;
            if (m < p.M) {
                const int j = (int)(m % cp.Wg);
                const long t = m / cp.Wg;
                d = ((t / cp.Hg) * cp.Hc + (t % cp.Hg) * 2) * (long)cp.Wc + 2 * j;
            }
            dst0[i][q] = d;
            full = full && d >= 0;
        }
    float es1[TN], et1[TN];
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int n = n0 + wn * (BN / 2) + j * 32 + fr;
        es1[j] = n < p.N ? p.scale1[n] : 0.f;
        et1[j] = n < p.N ? p.shift1[n] : 0.f;
        asm volatile("" ::"v"(es1[j]), "v"(et1[j]));   // waited for here, not behind the DMA groups in the loop
        full = full && (n0 + wn * (BN / 2) + j * 32 + 31 < p.N);
    }
    full = __builtin_amdgcn_readfirstlane(__builtin_amdgcn_ballot_w64(!full) == 0);   // per wave: no masked store, the store count is exact
    const float hi = p.act == 1 ? 6.f : __builtin_inff();
    const float slope = p.act == 4 ? 0.2f : 1.f, lo = (p.act == 1 || p.act == 2) ? 0.f : -__builtin_inff();

    // ---- per-phase state
    const uint16_t* __restrict__ Whi = cp.Whi4[0];
    const uint16_t* __restrict__ Wlo = cp.Wlo4[0];
    int ntaps = cp.ntaps4[0];
    unsigned long long dyp = cp.dyp4[0], dxp = cp.dxp4[0];
    const unsigned char* asrc[4];
    const unsigned char* wsrc[WQ];
    auto set_tap = [&](int tap) {
        const int dy = (int)((dyp >> (7 * tap)) & 127) - 64, dx = (int)((dxp >> (7 * tap)) & 127) - 64;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int iy = pi[q] * cp.sa + dy, ix = pj[q] * cp.sa + dx;
            const bool ok = iy >= 0 && iy < cp.Ha && ix >= 0 && ix < cp.Wa;
            const long pix = (long)pb[q] + (long)iy * cp.Wa + ix;
            asrc[q] = (ok ? p.A + pix * p.lda_bytes : g_zero_buf) + pc[q];
        }
    };
    auto set_phase = [&](int ph) {
        Whi = cp.Whi4[ph]; Wlo = cp.Wlo4[ph]; ntaps = cp.ntaps4[ph]; dyp = cp.dyp4[ph]; dxp = cp.dxp4[ph];
        const int Ktot = ntaps * cp.Cpad;
#pragma unroll
        for (int q = 0; q < WQ; ++q) {
            const int row = wv * (WQ * 8) + q * 8 + drow;
            const int c = dchunk ^ ((row >> 1) & 7);
            const uint16_t* plane = (c & 4) ? Wlo : Whi;
            wsrc[q] = reinterpret_cast<const unsigned char*>(plane + (long)(n0 + row) * Ktot + (c & 3) * 8);
        }
    };
    auto issue = [&](int stage, int tap, int kc) {
        unsigned char* sb = smem + stage * STAGE;
#pragma unroll
        for (int q = 0; q < 4; ++q)
            __builtin_amdgcn_global_load_lds((gptr_t)(asrc[q] + (long)kc * 128), (lptr_t)(sb + (wv * 32 + q * 8) * 128), 16, 0, 0);
        const long wk = ((long)tap * cp.Cpad + (long)kc * 32) * 2;
#pragma unroll
        for (int q = 0; q < WQ; ++q)
            __builtin_amdgcn_global_load_lds((gptr_t)(wsrc[q] + wk), (lptr_t)(sb + A_STAGE + (wv * (WQ * 8) + q * 8) * 128), 16, 0, 0);
    };

    f32x16 acc[2][TN];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    struct Frags { bf16x8 ah[2], al[2], bh[TN], bl[TN]; };
    auto load_frags = [&](Frags& f, const unsigned char* sb, int ks) {
        const int ch = ((ks * 2 + fh) ^ sw) << 4;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            f.ah[i] = *reinterpret_cast<const bf16x8*>(sb + a_off + i * 4096 + ch);
            f.al[i] = *reinterpret_cast<const bf16x8*>(sb + a_off + i * 4096 + (ch ^ 64));
        }
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            f.bh[j] = *reinterpret_cast<const bf16x8*>(sb + w_off + j * 4096 + ch);
            f.bl[j] = *reinterpret_cast<const bf16x8*>(sb + w_off + j * 4096 + (ch ^ 64));
        }
    };
    auto mfma12 = [&](const Frags& f) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f.al[i], f.bh[j], acc[i][j], 0, 0, 0);
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f.ah[i], f.bl[j], acc[i][j], 0, 0, 0);
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f.ah[i], f.bh[j], acc[i][j], 0, 0, 0);
            }
    };

    int total = 0, dtap = 0, dkc = 0, dstep = 0;
    auto advance = [&]() {
        if (dstep + 1 < total) {
            ++dstep;
            if (++dkc == cp.nkc) {
                dkc = 0;
                ++dtap;
                set_tap(dtap);
            }
        }
    };
    auto prologue = [&](int ph) {   // the first K step of phase ph into stage 0
        set_phase(ph);
        total = ntaps * cp.nkc;
        dtap = dkc = dstep = 0;
        set_tap(0);
        issue(0, 0, 0);
        advance();
    };
    prologue(0);
#pragma unroll 1
    for (int ph = 0; ph < 4; ++ph) {
        for (int st = 0; st < total; ++st) {
            // K step st has landed.  Older than its group: nothing but, at st == 0 of a later phase, nothing either (the previous
            // phase's stores were issued AFTER this phase's first group) -- so the E stores may stay in flight across the first barrier
            if (st == 0 && ph > 0 && full) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(E) : "memory");
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();       // ... for every wave; and every wave is done with the other stage (step st - 1)
            issue((st + 1) & 1, dtap, dkc);     // step st + 1 (beyond the last step: a re-read of it, so that the counts stay uniform)
            advance();
            Frags f0, f1;
            const unsigned char* sb = smem + (st & 1) * STAGE;
            load_frags(f0, sb, 0);
            load_frags(f1, sb, 1);
            mfma12(f0);
            mfma12(f1);
        }
        // every wave's fragment reads are done and this wave's surplus DMA groups have landed: the stages are free for the next phase
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        const int py = ph >> 1, px = ph & 1;
        if (ph < 3) prologue(ph + 1);
        // ---- epilogue of phase ph, straight from the accumulators
        const long poff = (long)py * cp.Wc + px;
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int n4 = n0 + wn * (BN / 2) + j * 32 + 4 * cq;
            const bool ncol = n4 < p.N;
            const float s1 = es1[j], t1 = et1[j];
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    float r[4];
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const float u = fmaf(acc[i][j][4 * q + k], s1, t1);
                        r[k] = fminf(fmaxf(fmaxf(u, lo), slope * u), hi);
                    }
                    quad_transpose(r, li);
                    if (ncol && dst0[i][q] >= 0) store_nt16(p.C + (dst0[i][q] + poff) * p.ldc + n4, f32x4{r[0], r[1], r[2], r[3]});
                }
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

}  // namespace

// plan -> instance (conv_entry.hip made the plan and filled the tile counts and nt from it)
extern "C" int conv_split_launch(const emd::ConvPlan& pl, const SplitConvParams& c, hipStream_t st) {
    const dim3 threads(pl.threads);
    const bool n64 = pl.bn == 64;
    switch (pl.route) {
    case emd::kDeconvHalf:    // 128-row tiles, two workgroups per CU
        if (n64) hipLaunchKernelGGL((deconv4_half_kernel<64>), pl.grid, threads, 0, st, c);
        else hipLaunchKernelGGL((deconv4_half_kernel<128>), pl.grid, threads, 0, st, c);
        return emd::check_launch("deconv4_half_kernel");
    case emd::kDeconvSplit:   // epilogue from the registers, next phase's DMA first
        if (n64) hipLaunchKernelGGL((deconv4_split_kernel<64>), pl.grid, threads, 0, st, c);
        else hipLaunchKernelGGL((deconv4_split_kernel<128>), pl.grid, threads, 0, st, c);
        return emd::check_launch("deconv4_split_kernel");
    case emd::kDeconvFour:
        if (n64) hipLaunchKernelGGL((gemm_split_conv_kernel<64, true>), pl.grid, threads, 0, st, c);
        else hipLaunchKernelGGL((gemm_split_conv_kernel<128, true>), pl.grid, threads, 0, st, c);
        break;
    default:
        if (n64) hipLaunchKernelGGL((gemm_split_conv_kernel<64>), pl.grid, threads, 0, st, c);
        else hipLaunchKernelGGL((gemm_split_conv_kernel<128>), pl.grid, threads, 0, st, c);
    }
    return emd::check_launch("gemm_split_conv_kernel");
}
