// The dense and transposed convolutions (and the pointwise ones on fp32 input), host side: the parameter block of gemm_conv.hip's
// kernels, the plan conv_entry.hip makes for a launch (which kernel, on which tiles, with which grid) and the one launcher each kernel
// file ends with, which maps a plan to a template instance and reads no knob.  The entry points, their checks, the geometry and every
// routing rule are in conv_entry.hip.
#pragma once

#include "split_params.hpp"
#include "conv3_params.hpp"

namespace {   // (anonymous, as the kernels are: see split_params.hpp)

struct GemmParams {
    const float* A;       // source activations (NHWC), pixel stride lda
    const uint16_t* Whi;  // [Npad][taps*Cpad]
    const uint16_t* Wlo;
    float* C;             // destination, pixel stride ldc
    const float* res;     // optional residual (same pixel indexing as C), pixel stride ldres
    const float* scale1;  // [N] epilogue: y = acc*scale1 + shift1
    const float* shift1;
    const float* scale2;  // optional second affine + relu6 (ASPP extra BN)
    const float* shift2;
    long M;               // B*Hg*Wg
    int N, Cin, Cpad, ntaps;
    int lda, ldc, ldres;
    int act;              // EMD_ACT_*: 0 none, 1 relu6, 2 relu -- after the first affine (and after the second)
    // row map: m -> (b,i,j) on Hg x Wg;  source (b, i*sa+dy, j*sa+dx) in Ha x Wa;  dest (b, i*sc+py, j*sc+px) in Hc x Wc
    int flat;             // 1: source pixel = dest pixel = m (plain pointwise)
    int Hg, Wg, Ha, Wa, Hc, Wc, sa, sc, py, px;
    unsigned long long dyp, dxp;  // per-tap source offsets, 7 bits each, biased by 64 (no dynamic kernarg indexing)
    int n_mtiles, n_ntiles;
    double* stats_part;   // optional [n_mtiles][2][N]: per-channel sum / sum of squares of the values each M tile STORES (training: the
                          // batch norm behind the conv takes batch statistics -- no second pass over y)
    int stats_tpi, stats_nph, stats_ph;   // the transposed conv's four phase launches share one table: M tile mt of phase ph is slab
                                          // ((mt / tpi) * nph + ph) * tpi + mt % tpi  (tpi = tiles per image, or all tiles; nph = 0: slab = mt)
};

// UP epilogue: the per-channel shift is replaced by a per-pixel one, the bilinear upsampling of a low-resolution tensor `up` [B,Hu,Wu,N]
// to the output's Hc x Wc pixels, sampled with resize_bilinear_kernel's arithmetic (f4_math.hpp) and never written.  Its arguments ride
// behind GemmParams in the UP instances' own parameter type: the other instances keep their kernel arguments, and their instructions.
struct UpSample {
    const float* up;
    int ldup, Hu, Wu;
    float sy, sx;   // (float)Hu / Hc, (float)Wu / Wc
};
struct GemmUpParams : GemmParams {
    UpSample u;
};

}  // namespace

namespace emd {

// Which kernel takes a launch; emd_debug_conv_plan reports these numbers.
enum ConvRoute {
    kConvNone = 0,
    kGemmConv,       // gemm_conv.hip: gemm_conv_kernel<bn, passes, flat>, fp32 input
    kGemmConvUp,     //   its upsampled-shift instance
    kConvSplit,      // conv_split.hip: gemm_split_conv_kernel<bn>
    kConv3Pipe,      // conv3_pipe.hip
    kDeconvFour,     // conv_split.hip, the transposed conv in one launch: gemm_split_conv_kernel<bn, true>
    kDeconvSplit,    //   deconv4_split_kernel<bn>
    kDeconvHalf,     //   deconv4_half_kernel<bn>
    kDeconvPipe,     // deconv_pipe.hip
};

// Everything a launch is made of besides the caller's pointers and shape.
struct ConvPlan {
    int route;            // ConvRoute; kConvNone: the entry answers EMD_E_UNSUPPORTED with `refuse`
    const char* refuse;
    int bm, bn;           // rows (pixels) and columns (channels) of a tile; the patch-resident kernels: 8 x 32 pixels, 64 columns
    int threads;
    dim3 grid;            // of one launch
    int launches;         // 4: the transposed conv as four phase GEMMs; deconv_pipe: slices of 65535 images
    int n_mtiles, n_ntiles;
    int form;             // gemm_conv_kernel: 1 = the flat row map; patch-resident kernels: 1 = split32 output
    int passes;           // gemm_conv_kernel: MFMA passes = the precision
    int tpw, epi;         // patch-resident kernels: tiles per workgroup, epilogue width the instance is compiled for
    int nt;               // non-temporal output stores (split32 input)
    int ablate;           // deconv_pipe: the dev knob sep_ablate
};

}  // namespace emd

// One per kernel file.  extern "C" because the parameter types live in an anonymous namespace: a C++ function of such a type could not be
// called from another file; every file sees the same definition through this header.
extern "C" int gemm_conv_launch(const emd::ConvPlan& plan, const GemmParams& p, const UpSample* up, hipStream_t st);
extern "C" int conv_split_launch(const emd::ConvPlan& plan, const SplitConvParams& c, hipStream_t st);
namespace emd {
int conv3_pipe_launch(const ConvPlan& plan, const Conv3Params& q, hipStream_t st);
int deconv_pipe_launch(const ConvPlan& plan, const DeconvPipeParams& q, hipStream_t st);
}  // namespace emd
