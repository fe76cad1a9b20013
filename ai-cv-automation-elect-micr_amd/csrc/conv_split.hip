// Implicit-GEMM convolutions on the matrix cores from split32 activations (the layout: gemm_split.hip), on the LDS-DMA pipeline of the
// pointwise GEMM there: the dense 3x3 conv as a 9-tap GEMM (gemm_split_conv_kernel, emd_conv3x3_split32_f32) and
// slim.conv2d_transpose(k = 3, s = 2) as GEMM (deconv4_split_kernel, deconv4_half_kernel, the emd_deconv3x3s2_* entry points and
// their routing to the patch-resident kernels conv3_pipe.hip / deconv_pipe.hip).
#include <cstdlib>

#include "split_params.hpp"
#include "conv3_params.hpp"

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

// ---------------------------------------------------------------------------------------------- convolutions on split32 input
namespace {

void set_taps(SplitConvParams& c, int n, const int* dy, const int* dx) {
    c.ntaps = n;
    c.dyp = c.dxp = 0;
    for (int t = 0; t < n; ++t) {
        c.dyp |= (unsigned long long)((dy ? dy[t] : 0) + 64) << (7 * t);
        c.dxp |= (unsigned long long)((dx ? dx[t] : 0) + 64) << (7 * t);
    }
}

int conv_checks(const void* xs, int ldx, const uint16_t* whi, const uint16_t* wlo, const float* scale1, const float* shift1,
                const float* scale2, const float* shift2, const float* res, int ldres, void* y, int ldy, int Cin, int Cout,
                int out_split) {
    EMD_REQUIRE(xs && whi && wlo && scale1 && shift1 && y, EMD_E_INVALID, "split32 conv: null pointer");
    EMD_REQUIRE((scale2 == nullptr) == (shift2 == nullptr), EMD_E_INVALID, "split32 conv: scale2/shift2 must come together");
    EMD_REQUIRE(Cin >= 1 && Cin <= 2048 && Cout >= 4 && Cout % 4 == 0, EMD_E_INVALID, "split32 conv: 1 <= Cin <= 2048, Cout a multiple of 4");
    EMD_REQUIRE(ldx % 32 == 0 && ldx >= emd_split32_ld(Cin) && (reinterpret_cast<uintptr_t>(xs) & 127u) == 0, EMD_E_ALIGN,
                "split32 conv: xs 128-byte aligned, ldx a multiple of 32, >= ceil32(Cin)");
    if (out_split)
        EMD_REQUIRE(ldy % 32 == 0 && ldy >= emd_split32_ld(Cout) && (reinterpret_cast<uintptr_t>(y) & 127u) == 0, EMD_E_ALIGN,
                    "split32 conv: split32 output needs y 128-byte aligned, ldy a multiple of 32, >= ceil32(Cout)");
    else
        EMD_REQUIRE(ldy % 4 == 0 && ldy >= Cout && emd::aligned16(y), EMD_E_ALIGN, "split32 conv: ldy a multiple of 4, >= Cout; y 16-byte aligned");
    EMD_REQUIRE(!res || (ldres % 4 == 0 && ldres >= Cout && emd::aligned16(res)), EMD_E_ALIGN, "split32 conv: res alignment");
    EMD_REQUIRE(emd::aligned16(scale1) && emd::aligned16(shift1) && (!scale2 || (emd::aligned16(scale2) && emd::aligned16(shift2))) &&
                    emd::aligned16(whi) && emd::aligned16(wlo),
                EMD_E_ALIGN, "split32 conv: weight planes and scale/shift vectors must be 16-byte aligned");
    return EMD_OK;
}

int launch_conv(SplitConvParams& c, hipStream_t st, bool four = false) {
    SplitGemmParams& p = c.g;
    c.Cpad = (p.Cin + kBK - 1) / kBK * kBK;
    c.nkc = (p.Cin + SBK - 1) / SBK;
    p.Ktot = c.ntaps * c.Cpad;
    const int bn = p.N <= 64 ? 64 : 128;
    p.n_mtiles = (int)((p.M + 255) / 256);
    p.n_ntiles = (p.N + bn - 1) / bn;
    p.stamps = nullptr;
    p.nt = split_nt(0);
    const long nblk = (long)p.n_mtiles * p.n_ntiles;
    if (nblk <= 0 || nblk > 0x7fffffffL) return emd::fail(EMD_E_UNSUPPORTED, "split32 conv: grid too large");
    if (p.M > 0x7fffffffL || (!c.flat && (long)(p.M / ((long)c.Hg * c.Wg)) * c.Ha * c.Wa > 0x7fffffffL))
        return emd::fail(EMD_E_UNSUPPORTED, "split32 conv: more than 2^31 pixels");   // the kernel keeps pixel indices in 32 bits
    if (four && !c.out_split && !p.res && !p.scale2 && emd::g_knobs.deconv_direct == 2) {   // 128-row tiles, two workgroups per CU
        p.n_mtiles = (int)((p.M + 127) / 128);
        const long nb2 = (long)p.n_mtiles * p.n_ntiles;
        if (nb2 > 0x7fffffffL) return emd::fail(EMD_E_UNSUPPORTED, "split32 conv: grid too large");
        if (bn == 64) hipLaunchKernelGGL((deconv4_half_kernel<64>), dim3((unsigned)nb2), dim3(256), 0, st, c);
        else hipLaunchKernelGGL((deconv4_half_kernel<128>), dim3((unsigned)nb2), dim3(256), 0, st, c);
        return emd::check_launch("deconv4_half_kernel");
    }
    if (four && !c.out_split && !p.res && !p.scale2 && emd::g_knobs.deconv_direct) {   // round 3: epilogue from the registers, next phase's DMA first
        if (bn == 64) hipLaunchKernelGGL((deconv4_split_kernel<64>), dim3((unsigned)nblk), dim3(512), 0, st, c);
        else hipLaunchKernelGGL((deconv4_split_kernel<128>), dim3((unsigned)nblk), dim3(512), 0, st, c);
        return emd::check_launch("deconv4_split_kernel");
    }
    if (four) {
        if (bn == 64) hipLaunchKernelGGL((gemm_split_conv_kernel<64, true>), dim3((unsigned)nblk), dim3(512), 0, st, c);
        else hipLaunchKernelGGL((gemm_split_conv_kernel<128, true>), dim3((unsigned)nblk), dim3(512), 0, st, c);
    } else if (bn == 64) hipLaunchKernelGGL((gemm_split_conv_kernel<64>), dim3((unsigned)nblk), dim3(512), 0, st, c);
    else hipLaunchKernelGGL((gemm_split_conv_kernel<128>), dim3((unsigned)nblk), dim3(512), 0, st, c);
    return emd::check_launch("gemm_split_conv_kernel");
}

}  // namespace

extern "C" int emd_conv3x3_split32_f32(const void* xs, int ldx, const uint16_t* whi, const uint16_t* wlo, const float* scale1,
                                       const float* shift1, const float* scale2, const float* shift2, const float* res,
                                       int ldres, void* y, int ldy, int B, int H, int W, int Cin, int Cout, int stride,
                                       int rate, int act, int out_split, emd_stream_t stream) {
    int rc = conv_checks(xs, ldx, whi, wlo, scale1, shift1, scale2, shift2, res, ldres, y, ldy, Cin, Cout, out_split);
    if (rc != EMD_OK) return rc;
    EMD_REQUIRE(B >= 0 && H >= 1 && W >= 1, EMD_E_INVALID, "emd_conv3x3_split32_f32: bad shape");
    EMD_REQUIRE(stride == 1 || stride == 2, EMD_E_UNSUPPORTED, "emd_conv3x3_split32_f32: stride must be 1 or 2");
    EMD_REQUIRE(rate >= 1 && rate <= 31 && (rate == 1 || stride == 1), EMD_E_UNSUPPORTED,
                "emd_conv3x3_split32_f32: rate must be 1..31, and 1 when stride is 2");
    if (B == 0) return EMD_OK;
    if (stride == 1 && rate == 1 && !res && H >= 8 && B <= 65535 && 9L * W * ldy < (1L << 31)) {   // round 3: the patch-resident kernel (conv3_pipe.hip)
        emd::Conv3Params q{};
        q.x = static_cast<const unsigned char*>(xs); q.ldx_bytes = (long)ldx * 4; q.Whi = whi; q.Wlo = wlo; q.y = static_cast<float*>(y);
        q.scale1 = scale1; q.shift1 = shift1; q.scale2 = scale2; q.shift2 = shift2;
        q.H = H; q.W = W; q.Cin = (Cin + 31) / 32 * 32; q.Cpad = (Cin + kBK - 1) / kBK * kBK; q.Ktot = 9 * q.Cpad; q.N = Cout; q.ldy = ldy; q.act = act;
        if (emd::conv3_pipe_covers(q)) return emd::conv3_pipe_launch(q, B, out_split, static_cast<hipStream_t>(stream));
    }
    SplitConvParams c{};
    SplitGemmParams& p = c.g;
    p.A = static_cast<const unsigned char*>(xs); p.Whi = whi; p.Wlo = wlo; p.C = static_cast<float*>(y); p.res = res;
    p.scale1 = scale1; p.shift1 = shift1; p.scale2 = scale2; p.shift2 = shift2;
    p.lda_bytes = (long)ldx * 4; p.N = Cout; p.Cin = Cin; p.ldc = ldy; p.ldres = ldres; p.act = act;
    const int Ho = (H + stride - 1) / stride, Wo = (W + stride - 1) / stride;
    const int eff = 2 * rate + 1;
    int pth = (Ho - 1) * stride + eff - H, ptw = (Wo - 1) * stride + eff - W;  // TF SAME: total padding
    if (pth < 0) pth = 0;
    if (ptw < 0) ptw = 0;
    const int pt = pth / 2, pl = ptw / 2;
    p.M = (long)B * Ho * Wo;
    c.flat = 0; c.out_split = out_split ? 1 : 0;
    c.Hg = Ho; c.Wg = Wo; c.Ha = H; c.Wa = W; c.Hc = Ho; c.Wc = Wo; c.sa = stride; c.sc = 1; c.py = c.px = 0;
    int dy[9], dx[9];
    for (int ky = 0; ky < 3; ++ky)
        for (int kx = 0; kx < 3; ++kx) {
            dy[ky * 3 + kx] = ky * rate - pt;
            dx[ky * 3 + kx] = kx * rate - pl;
        }
    set_taps(c, 9, dy, dx);
    return launch_conv(c, static_cast<hipStream_t>(stream));
}

extern "C" int emd_deconv3x3s2_split32_f32(const void* xs, int ldx, const uint16_t* const whi[4], const uint16_t* const wlo[4],
                                           const float* scale1, const float* shift1, void* y, int ldy, int B, int H, int W,
                                           int Cin, int Cout, int act, int out_split, emd_stream_t stream) {
    EMD_REQUIRE(whi && wlo, EMD_E_INVALID, "emd_deconv3x3s2_split32_f32: null weight table");
    for (int ph = 0; ph < 4; ++ph) {
        int rc = conv_checks(xs, ldx, whi[ph], wlo[ph], scale1, shift1, nullptr, nullptr, nullptr, 0, y, ldy, Cin, Cout, out_split);
        if (rc != EMD_OK) return rc;
    }
    EMD_REQUIRE(B >= 0 && H >= 1 && W >= 1, EMD_E_INVALID, "emd_deconv3x3s2_split32_f32: bad shape");
    if (B == 0) return EMD_OK;
    for (int ph = 0; ph < 4; ++ph) {
        SplitConvParams c{};
        SplitGemmParams& p = c.g;
        int ky[4], kx[4];
        const int nt = emd_deconv_phase_taps(ph, ky, kx);
        p.A = static_cast<const unsigned char*>(xs); p.Whi = whi[ph]; p.Wlo = wlo[ph]; p.C = static_cast<float*>(y); p.res = nullptr;
        p.scale1 = scale1; p.shift1 = shift1; p.scale2 = p.shift2 = nullptr;
        p.lda_bytes = (long)ldx * 4; p.N = Cout; p.Cin = Cin; p.ldc = ldy; p.ldres = 0; p.act = act;
        p.M = (long)B * H * W;
        c.flat = 0; c.out_split = out_split ? 1 : 0;
        c.Hg = H; c.Wg = W; c.Ha = H; c.Wa = W; c.Hc = 2 * H; c.Wc = 2 * W; c.sa = 1; c.sc = 2;
        c.py = ph >> 1; c.px = ph & 1;
        int dy[4], dx[4];
        for (int t = 0; t < nt; ++t) {  // kernel index 2 reads the previous input sample
            dy[t] = ky[t] == 2 ? -1 : 0;
            dx[t] = kx[t] == 2 ? -1 : 0;
        }
        set_taps(c, nt, dy, dx);
        int rc = launch_conv(c, static_cast<hipStream_t>(stream));
        if (rc != EMD_OK) return rc;
    }
    return EMD_OK;
}

// The same transposed convolution as ONE launch (gemm_split_conv_kernel<BN, true>): each workgroup computes the four output
// phases of its 256 input pixels back to back, so the input is fetched from HBM once instead of once per phase launch (the 9 taps'
// DMA re-reads hit L2).  Same products in the same order as the four-launch form: bit-identical results.
// Where graph hosts should take the one-launch form (emd_deconv3x3s2_fused_split32_f32) rather than the register-staged four-phase GEMM:
// always where the patch-resident kernel covers the layer (H % 8 == 0, W % 32 == 0, Cin % 32 == 0: it sums in another order than the GEMM
// forms, so the choice must not depend on the batch size -- image b of a batch == the image alone, bit for bit), otherwise from 192
// row tiles on (the GEMM forms agree with each other bit for bit, there the choice is speed only).
// ONE predicate for "this layer runs on the patch-resident kernel" (deconv_pipe.hip), used by emd_deconv3x3s2_fused_preferred and by the
// entry point alike, and a function of the LAYER only (H, W, Cin, Cout) -- never of the batch size or of the pitches: the kernel sums in
// another order than the GEMM forms, so a route that flipped with B (or with the buffer a tensor happens to live in) would break "image b
// of a batch == the image alone, bit for bit".  What the kernel additionally needs of a call (32-bit in-image offsets: H * W * ldx_bytes <
// 2^32, 36 * W * ldy < 2^31) is checked by the entry point and REPORTED (EMD_E_UNSUPPORTED) instead of silently falling back to a kernel
// with other bits; batches beyond the grid's 65535 images are cut into launches of the same kernel.
static bool deconv_patch_route(int H, int W, int Cin, int Cout) {
    emd::DeconvPipeParams q{};
    q.H = H; q.W = W; q.Cin = (Cin + 31) / 32 * 32; q.N = Cout;   // (ldx_bytes = 0: the offset bound is the entry point's to check)
    return Cin % 32 == 0 && H >= 8 && emd::deconv_pipe_covers(q);
}

extern "C" int emd_deconv3x3s2_fused_preferred(int B, int H, int W, int Cin, int Cout) {
    if (deconv_patch_route(H, W, Cin, Cout)) return 1;
    return (long)B * H * W >= 256L * 192 ? 1 : 0;
}

extern "C" int emd_deconv3x3s2_fused_split32_f32(const void* xs, int ldx, const uint16_t* const whi[4], const uint16_t* const wlo[4],
                                                 const float* scale1, const float* shift1, void* y, int ldy, int B, int H, int W,
                                                 int Cin, int Cout, int act, int out_split, emd_stream_t stream) {
    EMD_REQUIRE(whi && wlo, EMD_E_INVALID, "emd_deconv3x3s2_fused_split32_f32: null weight table");
    for (int ph = 0; ph < 4; ++ph) {
        int rc = conv_checks(xs, ldx, whi[ph], wlo[ph], scale1, shift1, nullptr, nullptr, nullptr, 0, y, ldy, Cin, Cout, out_split);
        if (rc != EMD_OK) return rc;
    }
    EMD_REQUIRE(B >= 0 && H >= 1 && W >= 1, EMD_E_INVALID, "emd_deconv3x3s2_fused_split32_f32: bad shape");
    if (B == 0) return EMD_OK;
    if (Cin % 32 == 0 && deconv_patch_route(H, W, Cin, Cout)) {   // the patch-resident kernel (deconv_pipe.hip), dev knob deconv_direct = 3
        emd::DeconvPipeParams q{};
        q.x = static_cast<const unsigned char*>(xs); q.ldx_bytes = (long)ldx * 4; q.y = static_cast<float*>(y);
        for (int ph = 0; ph < 4; ++ph) { q.Whi[ph] = whi[ph]; q.Wlo[ph] = wlo[ph]; }
        q.scale1 = scale1; q.shift1 = shift1;
        q.H = H; q.W = W; q.Cin = (Cin + 31) / 32 * 32; q.Cpad = (Cin + kBK - 1) / kBK * kBK; q.N = Cout; q.ldy = ldy; q.act = act;
        EMD_REQUIRE(emd::deconv_pipe_covers(q) && 36L * W * ldy < (1L << 31), EMD_E_UNSUPPORTED,
                    "emd_deconv3x3s2_fused_split32_f32: this layer runs on the patch-resident kernel, whose in-image offsets are 32-bit "
                    "(H * W * ldx * 4 < 2^32, 36 * W * ldy < 2^31): pitch too large (a fallback would change the summation order)");
        const long in_img = (long)H * W * q.ldx_bytes, out_img = 4L * H * W * ldy * (long)sizeof(float);
        for (int b0 = 0; b0 < B; b0 += 65535) {   // grid.z <= 65535: the same kernel on slices of the batch
            const int nb = B - b0 < 65535 ? B - b0 : 65535;
            q.x = static_cast<const unsigned char*>(xs) + (long)b0 * in_img;
            q.y = reinterpret_cast<float*>(static_cast<unsigned char*>(y) + (long)b0 * out_img);
            int rc = emd::deconv_pipe_launch(q, nb, out_split, static_cast<hipStream_t>(stream));
            if (rc != EMD_OK) return rc;
        }
        return EMD_OK;
    }
    SplitConvParams c{};
    SplitGemmParams& p = c.g;
    p.A = static_cast<const unsigned char*>(xs); p.Whi = whi[0]; p.Wlo = wlo[0]; p.C = static_cast<float*>(y); p.res = nullptr;
    p.scale1 = scale1; p.shift1 = shift1; p.scale2 = p.shift2 = nullptr;
    p.lda_bytes = (long)ldx * 4; p.N = Cout; p.Cin = Cin; p.ldc = ldy; p.ldres = 0; p.act = act;
    p.M = (long)B * H * W;
    c.flat = 0; c.out_split = out_split ? 1 : 0;
    c.Hg = H; c.Wg = W; c.Ha = H; c.Wa = W; c.Hc = 2 * H; c.Wc = 2 * W; c.sa = 1; c.sc = 2; c.py = c.px = 0;
    for (int ph = 0; ph < 4; ++ph) {
        int ky[4], kx[4], dy[4], dx[4];
        const int nt = emd_deconv_phase_taps(ph, ky, kx);
        for (int t = 0; t < nt; ++t) {  // kernel index 2 reads the previous input sample
            dy[t] = ky[t] == 2 ? -1 : 0;
            dx[t] = kx[t] == 2 ? -1 : 0;
        }
        set_taps(c, nt, dy, dx);
        c.Whi4[ph] = whi[ph]; c.Wlo4[ph] = wlo[ph]; c.ntaps4[ph] = nt; c.dyp4[ph] = c.dyp; c.dxp4[ph] = c.dxp;
    }
    c.ntaps = 4;   // launch_conv derives Ktot from it; the kernel uses the per-phase counts
    return launch_conv(c, static_cast<hipStream_t>(stream), true);
}
