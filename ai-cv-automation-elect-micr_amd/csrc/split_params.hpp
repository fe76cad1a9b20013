// Parameter blocks of the GEMMs on split32 activations: the pointwise GEMM (gemm_split.hip) and the implicit-GEMM convolutions
// (conv_split.hip).  In an anonymous namespace, as the kernels are: a kernel's symbol carries its parameter type's namespace, and the
// trace tools and recorded profiles match on those symbols.
#pragma once

#include "mfma_common.hpp"

namespace {

struct SplitGemmParams {
    const unsigned char* A;   // split32 activations
    const uint16_t* Whi;      // [Npad][Ktot] (emd_pack_weights_bf16, taps = 1: Ktot = Cin padded to 64)
    const uint16_t* Wlo;
    float* C;
    const float* res;
    const float* scale1;
    const float* shift1;
    const float* scale2;
    const float* shift2;
    long M;
    long lda_bytes;           // pixel pitch of A in bytes
    int N, Cin, Ktot;
    int ldc, ldres, act;
    int n_mtiles, n_ntiles;
    double* stats_part;       // optional [n_mtiles][2][N]: per-channel sum / sum of squares of the STORED values of each M tile
    unsigned wlo_delta;       // persistent kernel: byte distance Wlo - Whi (one allocation)
    long long* stamps;        // dev builds only: 5 s_memtime stamps per workgroup (NULL otherwise)
    int out_split;            // pointwise kernel: C is a split32 tensor (pitch ldc 4-byte units), for a following split32 GEMM
    int nt;                   // non-temporal output stores: the output is not re-read by this launch, L2 is kept for the operands
};

struct SplitConvParams {
    SplitGemmParams g;
    int ntaps, Cpad, nkc;        // W tap stride (elements), 32-channel steps per tap
    int flat;                    // 1: source pixel = dest pixel = m
    int Hg, Wg, Ha, Wa, Hc, Wc, sa, sc, py, px;
    unsigned long long dyp, dxp; // per-tap source offsets, 7 bits each, biased by 64
    int out_split;
    // FOUR instances (the 3x3 stride-2 transposed conv as ONE launch): a workgroup runs the four output phases of its 256 input
    // pixels back to back, so the input rows come from HBM once (the later phases' DMA re-reads them from L2) instead of once per
    // phase launch.  Per phase: weight planes, tap count and tap offsets; the output phase (py, px) = (ph >> 1, ph & 1).
    const uint16_t* Whi4[4];
    const uint16_t* Wlo4[4];
    int ntaps4[4];
    unsigned long long dyp4[4], dxp4[4];
};

// Non-temporal output stores are the default (graph D: 26.0 -> 25.5 ms, PMC fetch of the transposed convs 5.97 -> 3.83 GB per launch:
// the outputs no longer push the re-read input rows out of L2).  The dev knob nt_mask masks them: bit 0 = the implicit-GEMM convolutions here,
// bit 2 = the pointwise GEMM (bit 1: sep_fused.hip).
inline int split_nt(int bit) { return (emd::g_knobs.nt_mask >> bit) & 1; }

constexpr int SBN = 128, SBK = 32;

}  // namespace
