// Parameter block shared by the fused separable-convolution kernels -- sep_fused.hip: register-staged loader, 8 x 16 (4 x 16) pixel tiles;
// sep_pipe.hip: LDS-DMA ring, 8 or 4 waves on 8 x 32 / 8 x 16 tiles, stride 1 and 2; sep_pipe2.hip: its software-pipelined form and the
// whole-chunk instance -- and the host-side plan (route, geometry) that sep_entry.hip makes for a launch and each kernel file maps to an
// instance.  The entry points, their checks and every routing rule are in sep_entry.hip.
#pragma once

#include "mfma_common.hpp"

namespace emd {

struct SepParams {
    const float* x;       // [B,H,W,Cin] pixel stride ldx
    const float* dw;      // [9][Cin]
    const uint16_t* Whi;  // [Npad][Cpad]
    const uint16_t* Wlo;
    float* y;             // [B,H,W,N] pixel stride ldy
    const float* res;
    const float* scale1;
    const float* shift1;
    const float* scale2;
    const float* shift2;
    int H, W, Cin, Cpad, N;
    int ldx, ldy, ldres, act;
    int stride;           // 1, or 2 (sep_pipe.hip only: TF SAME on even sizes; H, W are the INPUT sizes, the output is H/2 x W/2)
    int reflect;          // 1: the patch border is tf.pad(REFLECT) of the image (graph G), 0: zero (TF SAME)
    int tpw;              // output tiles per workgroup, side by side along W
    // generated input (layers fed by a 1-channel image): x is a one-value-per-pixel tensor d (pitch ldx) and the Cin-channel
    // input the depthwise stage sees is act(d * gen_a[c] + gen_t[c]) -- never written to memory
    const float* gen_a;
    const float* gen_t;
    int gen_act;
    int rg_stride;        // > 0: the residual is generated (below)
    // second output of the DUAL instances (emd_sep3x3_dual_f32): y2 = relu6(x * W2 * scale_b + shift_b), a 1x1 conv of the block's
    // INPUT -- the decoder's residual projection (denoiser.py:359/:371/:383), which reads the same tensor as the separable conv
    // Generated residual (rg_stride > 0; sep_pipe.hip, the stride-2 128-column instance: emd_sep3x3_fused_s2_genres_f32): where res would be
    // read, the epilogue computes what emd_cin1_f32 (no depthwise stage) would have written there -- fma(d, rg_a[c], rg_t[c]), relu6 if
    // rg_act -- from the one-value-per-pixel image rg_x (pitch rg_ld floats) sampled every rg_stride pixels: d = rg_x[b][oy * rg_stride]
    // [ox * rg_stride].  That instance has one output: its three pointers share the second output's storage and its three ints sit in
    // what was alignment padding, so the block keeps its size and offsets -- a longer block changes the code the compiler makes for
    // EVERY instance (argument loads regroup, scratch sizes and VGPR counts move), which this one must not.
    // Folded final conv (fold != 0; sep_pipe.hip, the 4-wave 64-column FOLD instance: emd_sep3x3_fused_fold_f32): y is not stored -- the
    // epilogue forms z_t[pixel] = sum_c fold_w[t][c] * y[pixel][c], t = 0..8, and writes nine planes fold_z [9][B][H][W].  One output too:
    // its two pointers and its flag share the second output's storage in the same way.
    // d formed in the kernel (sep_fused.hip, sep_gen9_kernel: emd_sep3x3_fused_gen9_f32): x is the contiguous 1-channel image and gen_w9
    // the nine taps of its 3x3 depthwise conv; one output, no generated residual: the pointer shares the second output's storage too.
    union { const uint16_t* W2hi; const float* rg_x; const float* gen_w9; };
    union { const uint16_t* W2lo; const float* fold_w; };   // [9][64]: the 3x3 conv's taps, channel innermost
    union { float* y2; float* fold_z; };
    union { const float* scale_b; const float* rg_a; };
    union { const float* shift_b; const float* rg_t; };
    int N2;
    union { int ldy2; int fold; };   // (fold means something only where N2 == 0: folded())
    int out_split;        // y is a split32 tensor (pitch ldy 4-byte units; N % 32 == 0): the consumer is a split32 GEMM
    int rg_ld;
    long long* stamps;    // dev hook: per-workgroup phase cycle sums (NULL otherwise)
    int nt;               // outputs leave with non-temporal stores (they are not re-read by this launch: keep L2 for the patch halos)
    int ablate;           // dev: sep_pipe phase ablation bits (0 in every product launch)
    int xcd;              // workgroup -> tile map that gives each XCD (workgroup id mod 8) one contiguous run of tiles
    int rg_act;
};
inline bool folded(const SepParams& p) { return p.N2 == 0 && p.fold != 0; }   // a two-output launch keeps its pitch in the same word
static_assert(sizeof(SepParams) == 232, "SepParams: the rg_* fields fill padding and share storage; see above before adding a field");

// Which kernel takes a launch.  sep_entry.hip (sep_plan) holds the rules; emd_debug_sep_plan reports these numbers (sep_fused.hip's
// routes come first: sep_plan tells the files apart by the order).
enum SepRoute {
    kSepNone = 0,
    kSepFused,        // sep_fused.hip: 64 / 128 columns, weights per chunk
    kSepFusedWres,    //   64 columns, Cin <= 64: weights resident in LDS
    kSepFusedWide,    //   one output of 129 .. 256 columns on 4 x 16 tiles
    kSepFusedDual,    //   two outputs
    kSepGen9,         //   sep_gen9_kernel
    kSepPipe,         // sep_pipe.hip
    kSepPipe2,        // sep_pipe2.hip, sep_pipe2_kernel
    kSepPipe2Chunk,   //   sep_pipe2_chunk_kernel
};

// Host side: everything a launch is made of besides the caller's pointers and shape.
struct SepPlan {
    int route;            // SepRoute
    int nw;               // waves per workgroup
    int tw, th;           // output pixels of a tile
    int tpw;
    dim3 grid;
    int xcd, nt;          // (nt is set on the sep_fused routes only)
    int mode;             // sep_pipe schedule: 1 = the patch one step ahead, 0 = two
    int epi;              // epilogue width the instance is compiled for (0: sep_fused has one form)
    int passes;           // sep_fused: MFMA passes = the precision
    long long* stamps;    // what the kernel gets as SepParams::stamps / ablate
    int ablate;
};
SepPlan sep_plan(const SepParams& p, int B, int precision);   // a pure function of its arguments and g_knobs

// One per kernel file: q is the caller's block with the plan's tpw, xcd, nt, stamps and ablate filled in; maps plan to an instance.
int sep_fused_launch(const SepParams& q, const SepPlan& plan, hipStream_t st);   // the kSepFused* routes and kSepGen9
int sep_pipe_launch(const SepParams& q, const SepPlan& plan, hipStream_t st);
int sep_pipe2_launch(const SepParams& q, const SepPlan& plan, hipStream_t st);   // kSepPipe2 and kSepPipe2Chunk

}  // namespace emd
