// Fused separable convolution, host side only: the C entry points emd_sep3x3_*, one routine for their argument checks (sep_check), one
// builder for the kernels' parameter block (sep_params) and the plan (sep_plan): which kernel of sep_fused.hip, sep_pipe.hip or
// sep_pipe2.hip takes a launch, on which tiles, with which grid.  Every routing rule and every dev knob of this path is read here and
// nowhere else; the kernel files map a plan to a template instance.  emd_debug_sep_plan shows the plan without a device.
#include <initializer_list>

#include "sep_params.hpp"

using namespace emd;

namespace {

// ------------------------------------------------------------------------------------------------------------------------------
// Argument checks.  Every entry runs the same ladder -- null pointers, the scale2/shift2 pair, the shape, the entry's own rule
// ("unsupported"), B, the 2^31 span, the pixel strides, 16-byte alignment -- and differs in what the descriptor below says.  The first
// failing step decides the code and the text.
struct SepEntry {
    const char* who;        // the name the messages carry
    const char* needs;      // the sentence of the "unsupported" step
    const char* span;       // the sentence of the 2^31 step
    const char* aligned;    // the sentence of the alignment step
    int min_hw;             // smallest H and W
    bool pitch_first;       // the pixel-stride step comes before the span step
};
struct SepPtr {
    const void* p;
    bool optional;          // may be NULL
    bool any_align;         // not asked for 16-byte alignment
};
struct SepPitch {
    int ld, min;            // ld >= min
    bool checked, quad;     // quad: ld % 4 == 0 too
};
enum SepStage { kAfterNull, kAfterSpan, kAfterPitch, kAfterAlign };
struct SepExtra {           // a step only this entry has, with its own code and text
    SepStage after;
    bool ok;
    int code;
    const char* msg;
};

int sep_check(const SepEntry& e, std::initializer_list<SepPtr> ptrs, const float* scale2, const float* shift2, int B, int H, int W,
              bool supported, int span_ld, std::initializer_list<SepPitch> pitches, std::initializer_list<SepExtra> extras = {}) {
    auto say = [&](int code, const char* what) {
        set_error("%s: %s", e.who, what);
        return code;
    };
    auto extra = [&](SepStage s) {
        for (const SepExtra& x : extras)
            if (x.after == s && !x.ok) return emd::fail(x.code, x.msg);
        return (int)EMD_OK;
    };
    bool null = false, pitch_ok = true, aligned = (!scale2 || emd::aligned16(scale2)) && (!shift2 || emd::aligned16(shift2));
    for (const SepPtr& a : ptrs) {
        null |= !a.p && !a.optional;
        aligned &= !a.p || a.any_align || emd::aligned16(a.p);
    }
    for (const SepPitch& s : pitches) pitch_ok &= !s.checked || ((!s.quad || s.ld % 4 == 0) && s.ld >= s.min);
    const char* pitch = "pixel strides must be multiples of 4 and >= the channel count";
    if (null) return say(EMD_E_INVALID, "null pointer");
    if (int rc = extra(kAfterNull)) return rc;
    if ((scale2 == nullptr) != (shift2 == nullptr)) return say(EMD_E_INVALID, "scale2/shift2 pair");
    if (!(B >= 0 && H >= e.min_hw && W >= e.min_hw)) return say(EMD_E_INVALID, "bad shape");
    if (!supported) return say(EMD_E_UNSUPPORTED, e.needs);
    if (B > 65535) return say(EMD_E_UNSUPPORTED, "B > 65535");
    if (e.pitch_first && !pitch_ok) return say(EMD_E_ALIGN, pitch);
    if (!(9L * W * span_ld < (1L << 31))) return say(EMD_E_UNSUPPORTED, e.span);
    if (int rc = extra(kAfterSpan)) return rc;
    if (!pitch_ok) return say(EMD_E_ALIGN, pitch);
    if (int rc = extra(kAfterPitch)) return rc;
    if (!aligned) return say(EMD_E_ALIGN, e.aligned);
    return extra(kAfterAlign);
}

constexpr const char* kSpanOut = "9 image rows of the output must span fewer than 2^31 floats";
constexpr const char* kAligned = "pointers must be 16-byte aligned";

// ------------------------------------------------------------------------------------------------------------------------------
// The parameter block: the fields every entry has; an entry adds its own (generated input, second output, fold, generated residual).
SepParams sep_params(const float* x, int ldx, const float* dw, const uint16_t* whi, const uint16_t* wlo, const float* scale1,
                     const float* shift1, const float* scale2, const float* shift2, const float* res, int ldres, float* y, int ldy, int H,
                     int W, int Cin, int Cout, int act, int stride, int reflect) {
    SepParams p{};
    p.x = x; p.dw = dw; p.Whi = whi; p.Wlo = wlo; p.y = y; p.res = res;
    p.scale1 = scale1; p.shift1 = shift1; p.scale2 = scale2; p.shift2 = shift2;
    p.H = H; p.W = W; p.Cin = Cin; p.Cpad = (Cin + kBK - 1) / kBK * kBK; p.N = Cout;
    p.ldx = ldx; p.ldy = ldy; p.ldres = ldres; p.act = act; p.stride = stride; p.reflect = reflect;
    return p;
}

// A block that carries a layer's shape and form and no tensors: what the predicates and emd_debug_sep_plan give to the rules below,
// which only ask whether a pointer is set.  The bits are emd_debug_sep_plan's.
enum : unsigned { kReflect = 1, kRes = 2, kAffine2 = 4, kOutSplit = 8, kGen = 16, kGen9 = 32, kGenRes = 64, kFold = 128 };
SepParams sep_shape(int H, int W, int Cin, int Cout, int Cout2, int stride, unsigned flags) {
    static const float set[4] = {};
    const float* res = (flags & kRes) ? set : nullptr;
    const float* s2 = (flags & kAffine2) ? set : nullptr;
    SepParams p = sep_params(nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, s2, s2, res, 0, nullptr, 0, H, W, Cin, Cout, 0, stride,
                             (flags & kReflect) ? 1 : 0);
    p.N2 = Cout2;
    p.out_split = (flags & kOutSplit) ? 1 : 0;
    if (flags & (kGen | kGen9)) { p.gen_a = p.gen_t = set; p.gen_act = EMD_ACT_RELU6; }
    if (flags & kGen9) p.gen_w9 = set;
    if (flags & kGenRes) p.rg_stride = 2;
    if (flags & kFold) p.fold = 1;
    return p;
}

// ------------------------------------------------------------------------------------------------------------------------------
// Routing: the shape rules of the entries, then the rules that choose among the kernels.

// emd_sep3x3_fused_f32 and its variants, stride 1.  128 < Cout <= 256: one N tile of 256 columns on 4 x 16 pixel tiles
// (sep_fused_kernel<256, PASSES, false, 4>).  Against depthwise -> HBM -> pointwise at [32,128,128,.]: 128 -> 256 256 vs 335 us,
// 256 -> 256 (+ residual) 537 vs 609 us, 384 -> 256 773 vs 734 us: the rule takes it up to Cin = 256.  dev knob sep_wide: 0 = never,
// 2 = whenever it fits.
bool fused_shape(const SepParams& p) {
    const bool wide = p.N > 128 && p.N <= 256 && (g_knobs.sep_wide == 2 || (g_knobs.sep_wide == 1 && p.Cin <= 256));
    return p.stride == 1 && p.H % 8 == 0 && p.W % 16 == 0 && p.Cin % 32 == 0 && p.Cin >= 32 && p.Cin <= 4096 && p.N % 4 == 0 && p.N >= 4 &&
           (p.N <= 128 || wide);
}

// emd_sep3x3_dual_f32: 64 | 64 columns on 8-row tiles, up to 128 | 128 on 4-row tiles (sep_fused.hip's forms; sep_pipe.hip asks for more)
bool dual_shape(const SepParams& p) {
    const bool wide = p.N > 64 || p.N2 > 64;
    return p.H % (wide ? 4 : 8) == 0 && p.W % 16 == 0 && p.Cin % 32 == 0 && p.Cin >= 32 && p.Cin <= 4096 && p.N % 4 == 0 && p.N2 % 4 == 0 &&
           p.N >= 4 && p.N2 >= 4 && p.N <= 128 && p.N2 <= 128;
}

// emd_sep3x3_fused_gen9_f32: a function of the layer's shape alone
bool gen9_shape(const SepParams& p) {
    return p.H >= 8 && p.W >= 16 && p.H % 8 == 0 && p.W % 16 == 0 && (p.Cin == 32 || p.Cin == 64) && p.N % 4 == 0 && p.N >= 4 && p.N <= 64;
}

// sep_pipe.hip's 4-wave form (8 x 16 tiles, 80 KiB of LDS or less: two workgroups per CU, whose phases -- DMA wait, depthwise stage, MFMAs,
// epilogue -- interleave): instances up to 128 output columns (one output, fp32 or split32) and 64 | 64 (two outputs).  Rule: wherever
// there is an instance.  Measured on graph D's shapes (tools/sep_epi_bench.py with SEB_KNOB=sep_nw, [32, ., ., .], two boxes): the
// two-output launch 512^2 x 128 -> 64 | 64 2078 -> 1892 us, 2084 -> 1921; 64 -> 64 961 -> 859, 943 -> 873; 128 -> 64 1382 -> 1354;
// 64 -> 64 with a residual 1161 / 1288 -> 1212 / 1210; 256^2 x 128 -> 128 480 -> 467, 486 -> 469; with residual and split32 output
// 669 -> 647 / 653; 384 -> 128 1155 -> 1144; the whole D step 23.36 -> 23.24 ms in one process (tools/d_knob_ab.py).  Dev knob
// sep_nw = 8 / 4 forces.
bool use_nw4(const SepParams& p) {
    if (g_knobs.sep_nw == 8 || p.stride == 2) return false;
    return p.N2 > 0 ? (p.N <= 64 && p.N2 <= 64) : (p.N <= 128 && !(p.out_split && p.N <= 64));    // instances: sep_pipe.hip, launch_mode
}

// true when the LDS-DMA pipelined kernel (sep_pipe.hip) covers the launch: split-bf16, W % 32 == 0 (W % 16 == 0 in the 4-wave form)
bool pipe_covers(const SepParams& p, int precision) {
    if (!g_knobs.sep_pipe || precision != 3) return false;
    if (folded(p))    // folded final conv: the 4-wave 64-column instance only -- deconv0_b of graph D and its likes
        return p.stride == 1 && p.H % 8 == 0 && p.W % 16 == 0 && p.Cin % 32 == 0 && p.Cin >= 32 && p.Cin <= 4064 && p.N == 64 && p.N2 == 0 &&
               !p.out_split && !p.gen_a && !p.rg_stride && !p.reflect && g_knobs.sep_nw != 8;
    if (p.gen_a)   // generated input (opt-in: dev knob sep_gen_pipe): the 4-wave 64-column instance only -- cnn0_last of graphs D / X and its likes
        return g_knobs.sep_gen_pipe && p.stride == 1 && p.H % 8 == 0 && p.W % 16 == 0 && (p.Cin == 32 || p.Cin == 64) && p.N <= 64 && p.N2 == 0 &&
               !p.out_split && !p.res && g_knobs.sep_nw != 8;
    if (p.rg_stride && (p.stride != 2 || p.N2 > 0 || p.N > 128 || p.res || p.reflect)) return false;   // generated residual: the stride-2 128-column instance only
    if (p.stride == 2)   // output tiles of 4 x 16 pixels: H % 8 == 0, W % 32 == 0 (input sizes); one fp32 output of up to 256 channels
        return p.H % 8 == 0 && p.W % 32 == 0 && p.Cin % 32 == 0 && p.Cin >= 32 && p.Cin <= 4064 && p.N2 == 0 && !p.out_split && p.N <= 256;
    if (p.H % 8 != 0 || p.W % (use_nw4(p) ? 16 : 32) != 0 || p.Cin % 32 != 0 || p.Cin < 32 || p.Cin > 4064) return false;
    if (p.N2 > 0) return p.N <= 128 && p.N2 <= 128 && !p.out_split && !p.res && !p.scale2;
    if (p.out_split && p.N <= 64) return false;
    return p.N <= 256;
}

// Shapes the software-pipelined kernel (sep_pipe2.hip) has an instance for: stride 1, 8 x 32 tiles (H % 8 == 0, W % 32 == 0), split-bf16,
// one output of up to 256 channels (fp32, or split32 from 128 channels on) or two of up to 128 each (no residual / second affine there).
bool pipe2_covers(const SepParams& p) {
    if (p.stride != 1 || p.gen_a || p.H % 8 != 0 || p.W % 32 != 0 || p.Cin % 32 != 0 || p.Cin < 32 || p.Cin > 4064) return false;
    if (p.N2 > 0) return p.N <= 128 && p.N2 <= 128 && !p.out_split && !p.res && !p.scale2;
    if (p.out_split && p.N <= 64) return false;
    return p.N <= 256;
}

// Its whole-chunk instance (sep_pipe2_chunk_kernel): two fp32 outputs, more than 64 columns in one of them (the 256-column tile), stride 1,
// 8 x 32 tiles.  A rule of the layer's shape alone.
bool pipe2_chunk_covers(const SepParams& p) {
    if (p.stride != 1 || p.gen_a || p.rg_stride || p.H % 8 != 0 || p.W % 32 != 0 || p.Cin % 32 != 0 || p.Cin < 32 || p.Cin > 4064) return false;
    return p.N2 > 0 && p.N <= 128 && p.N2 <= 128 && (p.N > 64 || p.N2 > 64) && !p.out_split && !p.res && !p.scale2;
}

// Which of sep_pipe.hip's launches go to the software-pipelined kernel (same bits).  Dev knob sep_pipe2: 0 (default) none, 1 the two-output
// launches with more than 64 columns per output (deconv1_a + residual1_d, 384 -> 128 | 128: the one shape whose slots are matrix-core
// bound), 2 everything it has an instance for (the parity tests).  Measured (profiles/r04_experiments.txt 3): standalone at parity on
// that shape (2034 / 2070 us against 2059 / 2004 on two boxes), 5-50 % SLOWER on every one-output shape -- where sep_pipe.hip's 4-wave
// two-workgroups-per-CU form wins: both kernels are bound by instruction issue and by phases no other wave fills, and the pipelined one
// issues ~1.9 x the instructions per chunk -- and graph D 22.10 ms with 0, 22.26 with 1, 23.07 with 2 in one process.  A forced 4-wave
// form (dev knob sep_nw = 4) always means sep_pipe.hip's kernel.
bool use_pipe2(const SepParams& p) {
    if (p.gen_a || p.rg_stride || folded(p)) return false;
    if (!g_knobs.sep_pipe2 || g_knobs.sep_ablate || g_knobs.sep_nw == 4 || !pipe2_covers(p)) return false;
    if (g_knobs.sep_pipe2 == 2) return true;
    return p.N2 > 0 && (p.N > 64 || p.N2 > 64);
}

// The whole-chunk instance (same bits): the two-output launches on the 256-column tile (deconv1_a + residual1_d of graph D), by the layer's
// shape alone.  Dev knob sep_pipe2_chunk: 1 takes it, 0 keeps sep_pipe.hip's lockstep kernel, -1 (default) = kChunkRule; the older knob
// sep_pipe2 (run-time parity instances) and the forced forms go first, and the instance writes no stamps.
constexpr int kChunkRule = 1;
bool use_pipe2_chunk(const SepParams& p) {
    const int on = g_knobs.sep_pipe2_chunk < 0 ? kChunkRule : g_knobs.sep_pipe2_chunk;
    if (!on || g_knobs.sep_pipe2 || g_knobs.sep_ablate || g_knobs.sep_nw == 4 || g_knobs.sep_stamps) return false;
    return pipe2_chunk_covers(p);
}

int pipe_route(const SepParams& p) { return use_pipe2(p) ? kSepPipe2 : use_pipe2_chunk(p) ? kSepPipe2Chunk : kSepPipe; }

// The route of a launch; kSepNone where the entry that would make it answers "unsupported".
int sep_route(const SepParams& p, int precision) {
    if (p.gen_a && p.gen_w9)   // emd_sep3x3_fused_gen9_f32: relu6 generation, zero padding, split-bf16
        return p.gen_act == EMD_ACT_RELU6 && !p.reflect && precision == 3 && gen9_shape(p) ? kSepGen9 : kSepNone;
    if (p.N2 > 0) {            // two outputs: sep_pipe.hip where it covers the shape, else sep_fused.hip's DUAL instances
        if (!dual_shape(p)) return kSepNone;
        return pipe_covers(p, 3) ? pipe_route(p) : kSepFusedDual;
    }
    if (folded(p))             // csrc/sep_pipe.hip (FOLD) only: there is no other form
        return p.H >= 1 && p.W >= 1 && pipe_covers(p, 3) ? pipe_route(p) : kSepNone;
    if (p.stride == 2) {       // only sep_pipe.hip has the form; its dev knob sep_pipe = 0 switches it off: hosts then take depthwise + pointwise
        if (p.N % 4 != 0 || p.N < 4 || !pipe_covers(p, 3)) return kSepNone;
        if (p.rg_stride && 64 % (p.N / 4) != 0) return kSepNone;   // (Cout / 4 divides 64: emd_cin1_f32's rule)
        return pipe_route(p);
    }
    if (!fused_shape(p)) return kSepNone;
    if (pipe_covers(p, precision)) return pipe_route(p);
    if (p.N > 128) return p.gen_a ? kSepNone : kSepFusedWide;   // 4 x 16 pixel tiles, no generated input
    // dev knob sep_wres: 0 = per-chunk W loads in the 64-column instances
    return p.N <= 64 && g_knobs.sep_wres && p.Cin <= 64 && precision == 3 ? kSepFusedWres : kSepFused;
}

// Several tiles per workgroup, side by side (the staging pipeline or DMA ring runs on across them), where at least min_wgs workgroups remain
int tiles_per_workgroup(int tiles_w, long wgs1, long min_wgs) {
    int tpw = 1;
    for (int t = 8; t >= 2; t >>= 1)
        if (tiles_w % t == 0 && wgs1 / t >= min_wgs) { tpw = t; break; }
    if (g_knobs.sep_tpw > 0 && tiles_w % g_knobs.sep_tpw == 0) tpw = g_knobs.sep_tpw;
    return tpw;
}

// B == 0 is a valid call that launches nothing.  no_route: the two entries whose checks leave a launch without a kernel say why.
int sep_run(const SepParams& p, int B, int precision, emd_stream_t stream,
            const char* no_route = "fused separable conv: no kernel takes the launch") {
    if (B == 0) return EMD_OK;
    const SepPlan plan = sep_plan(p, B, precision);
    SepParams q = p;
    q.tpw = plan.tpw; q.xcd = plan.xcd; q.nt = plan.nt; q.stamps = plan.stamps; q.ablate = plan.ablate;
    hipStream_t st = static_cast<hipStream_t>(stream);
    switch (plan.route) {
    case kSepNone: return emd::fail(EMD_E_UNSUPPORTED, no_route);
    case kSepPipe: return sep_pipe_launch(q, plan, st);
    case kSepPipe2:
    case kSepPipe2Chunk: return sep_pipe2_launch(q, plan, st);
    default: return sep_fused_launch(q, plan, st);
    }
}

}  // namespace

SepPlan emd::sep_plan(const SepParams& p, int B, int precision) {
    SepPlan pl{};
    pl.route = sep_route(p, precision);
    if (pl.route == kSepNone) return pl;
    int Ho = p.H, Wo = p.W;
    long min_wgs;
    // epilogue of the LDS-DMA kernels (see sep_pipe.hip): per-channel dword stores, 2.7 % over graph D's twelve shapes (tools/sep_epi_bench.py;
    // the two-output launches 5 %) -- except with a residual on more than 128 columns (cnn2_last: 445 against 430 us for the transposed
    // 16-byte form); the dev knob epi_width (1 / 4) overrides where the instance exists
    const bool epi4 = (g_knobs.epi_width ? g_knobs.epi_width : ((p.res && p.N > 128) ? 4 : 1)) == 4;
    if (pl.route <= kSepGen9) {   // sep_fused.hip: 4 waves on 8 x 16 pixels (4 x 16 on the 256-column tile), >= 8 workgroups per CU
        pl.nw = 4; pl.tw = 16;
        pl.th = pl.route == kSepFusedWide || (pl.route == kSepFusedDual && (p.N > 64 || p.N2 > 64)) ? 4 : 8;
        min_wgs = 2048;
        pl.passes = precision;
        pl.nt = (g_knobs.nt_mask >> 1) & 1;   // nt_mask bit 1 = non-temporal output stores (default on)
        pl.stamps = pl.route == kSepGen9 ? nullptr : g_knobs.sep_stamps;
    } else if (pl.route == kSepPipe) {   // 8 waves on 8 x 32 pixels or 4 on 8 x 16; stride 2: 8 on 4 x 16 output pixels; >= 4 workgroups per CU
        const bool s2 = p.stride == 2;
        pl.nw = (p.gen_a || folded(p) || (!s2 && use_nw4(p))) ? 4 : 8;
        pl.tw = s2 ? 16 : 4 * pl.nw; pl.th = s2 ? 4 : 8;
        if (s2) { Ho /= 2; Wo /= 2; }
        min_wgs = 1024 * (8 / pl.nw);
        pl.stamps = g_knobs.sep_stamps;
        pl.ablate = g_knobs.sep_ablate;
        // schedule (see the kernel): rule = the patch two steps ahead; one step ahead for two outputs, with a residual (its loads then
        // queue behind one DMA group instead of two) and in the 4-wave form; the dev knob sep_mode (0 / 1) overrides.  The generated-input
        // and generated-residual instances have the one schedule.
        const int mode = g_knobs.sep_mode >= 0 ? g_knobs.sep_mode : ((pl.nw == 4 || p.res) ? 1 : 0);
        pl.mode = mode == 1 || p.gen_a || p.rg_stride || p.N2 > 0;
        pl.epi = epi4 && !folded(p) && !p.rg_stride ? 4 : 1;   // the folded and generated-residual instances have one form
    } else {   // sep_pipe2.hip: 8 waves on 8 x 32 pixels
        pl.nw = 8; pl.tw = 32; pl.th = 8;
        min_wgs = 1024;
        if (pl.route == kSepPipe2) {   // (the whole-chunk instance writes no stamps)
            pl.stamps = g_knobs.sep_stamps;
            pl.ablate = g_knobs.sep_stamp_wave & 7;
            pl.epi = epi4 && p.N2 == 0 && p.N > 128 ? 4 : 1;   // only the 256-column one-output instances come in both widths
        } else {
            pl.epi = g_knobs.epi_width == 4 ? 4 : 1;
        }
    }
    const int tiles_w = Wo / pl.tw;
    pl.tpw = tiles_per_workgroup(tiles_w, (long)tiles_w * (Ho / pl.th) * B, min_wgs);
    pl.grid = dim3(tiles_w / pl.tpw, Ho / pl.th, B);
    pl.xcd = g_knobs.sep_xcd && ((long)pl.grid.x * pl.grid.y * pl.grid.z) % 8 == 0;
    return pl;
}

// ------------------------------------------------------------------------------------------------------------------------------
// Predicates and dev hooks

extern "C" int emd_sep3x3_fused_supported(int H, int W, int Cin, int Cout, int stride, int rate) {
    return rate == 1 && sep_route(sep_shape(H, W, Cin, Cout, 0, stride, 0), 3) != kSepNone;
}

extern "C" int emd_sep3x3_fused_fold_supported(int H, int W, int Cin, int Cout) {
    return sep_route(sep_shape(H, W, Cin, Cout, 0, 1, kFold), 3) != kSepNone;
}

extern "C" int emd_sep3x3_fused_s2_genres_supported(int H, int W, int Cin, int Cout) {
    return sep_route(sep_shape(H, W, Cin, Cout, 0, 2, kGenRes), 3) != kSepNone;
}

extern "C" int emd_sep3x3_fused_gen9_supported(int H, int W, int Cin, int Cout) { return gen9_shape(sep_shape(H, W, Cin, Cout, 0, 1, 0)); }

extern "C" int emd_sep3x3_dual_supported(int H, int W, int Cin, int Cout, int Cout2) {
    return dual_shape(sep_shape(H, W, Cin, Cout, Cout2, 1, 0));
}

// 1 when the one-launch form is the faster route for the shape (a pure function of the shape; graph D's decoder pairs): always for two
// outputs of up to 64 channels; for wider ones only where the LDS-DMA pipelined kernel takes the launch (W % 32 == 0, H % 8 == 0:
// 384 -> 128 | 128 at 256^2 2.07 ms against 1.32 + 0.99 for the pair; the 4 x 16-tile form of sep_fused.hip is slower than the pair).
extern "C" int emd_sep3x3_dual_preferred(int H, int W, int Cin, int Cout, int Cout2) {
    if (!emd_sep3x3_dual_supported(H, W, Cin, Cout, Cout2)) return 0;
    if (Cout <= 64 && Cout2 <= 64) return 1;
    return H % 8 == 0 && W % 32 == 0;
}

// dev hook (include/emdenoise_dev.h), host only: the shape rule of the whole-chunk instance of sep_pipe2.hip -- no batch argument
extern "C" int emd_debug_sep_pipe2_chunk_covers(int H, int W, int Cin, int Cout, int Cout2) {
    const SepParams p = sep_shape(H, W, Cin, Cout, Cout2, 1, 0);
    return dual_shape(p) && pipe2_chunk_covers(p) ? 1 : 0;
}

// dev hook (include/emdenoise_dev.h), host only: the plan of a launch
extern "C" int emd_debug_sep_plan(int B, int H, int W, int Cin, int Cout, int Cout2, int stride, int precision, unsigned flags, int out[10]) {
    const SepPlan pl = sep_plan(sep_shape(H, W, Cin, Cout, Cout2, stride, flags), B, precision);
    if (pl.route == kSepNone || !out) return pl.route;
    const int v[10] = {pl.route, pl.nw, pl.tpw, (int)pl.grid.x, (int)pl.grid.y, (int)pl.grid.z, pl.mode, pl.epi, pl.xcd, pl.nt};
    for (int i = 0; i < 10; ++i) out[i] = v[i];
    return pl.route;
}

// dev hook (include/emdenoise_dev.h): per-workgroup phase cycle sums for tools/sep_bench.py
extern "C" void emd_debug_sep_stamps(void* buf) { g_knobs.sep_stamps = static_cast<long long*>(buf); }

// ------------------------------------------------------------------------------------------------------------------------------
// Entry points

// emd_sep3x3_fused_f32 and the variants that share its checks and report under its name: _reflect, _out (split32 output), _gen (generated input)
static int sep_fused_entry(const float* x, int ldx, const float* dw, const uint16_t* whi, const uint16_t* wlo,
                           const float* scale1, const float* shift1, const float* scale2, const float* shift2,
                           const float* res, int ldres, float* y, int ldy, int B, int H, int W, int Cin, int Cout, int act,
                           int precision, int reflect, emd_stream_t stream, const float* gen_a = nullptr,
                           const float* gen_t = nullptr, int gen_act = 0, int out_split = 0) {
    static const SepEntry e{"emd_sep3x3_fused_f32",
                            "needs H%8==0, W%16==0, Cin%32==0, Cout%4==0, Cout<=128 or Cout<=256 with Cin<=256 (use emd_dw3x3_f32 + emd_conv1x1_f32)",
                            kSpanOut, kAligned, 1, false};
    const int rc = sep_check(
        e, {{x}, {dw}, {whi}, {wlo, true}, {scale1}, {shift1}, {y}, {res, true}}, scale2, shift2, B, H, W,
        emd_sep3x3_fused_supported(H, W, Cin, Cout, 1, 1), ldy > ldres ? ldy : ldres,
        {{ldx, gen_a ? 1 : Cin, true, !gen_a}, {ldy, Cout, true, true}, {ldres, Cout, res != nullptr, true}},
        {{kAfterNull, precision == 1 || precision == 3, EMD_E_INVALID, "emd_sep3x3_fused_f32: bad precision"},
         {kAfterNull, precision == 1 || wlo, EMD_E_INVALID, "emd_sep3x3_fused_f32: the split-bf16 mode needs the lo plane"},
         {kAfterSpan, !out_split || (Cout % 32 == 0 && ldy % 32 == 0 && (reinterpret_cast<uintptr_t>(y) & 127u) == 0), EMD_E_ALIGN,
          "emd_sep3x3_fused_out_f32: a split32 output needs Cout % 32 == 0, ldy % 32 == 0 and y 128-byte aligned"},
         {kAfterPitch, !gen_a || (gen_t && emd::aligned16(gen_a) && emd::aligned16(gen_t) && gen_act >= 0 && gen_act <= 4 && gen_act != 3),
          EMD_E_INVALID, "emd_sep3x3_fused_gen_f32: gen_a / gen_t must be 16-byte aligned device vectors, gen_act an EMD_ACT_* code"}});
    if (rc) return rc;
    SepParams p = sep_params(x, ldx, dw, whi, wlo, scale1, shift1, scale2, shift2, res, ldres, y, ldy, H, W, Cin, Cout, act, 1, reflect);
    p.gen_a = gen_a; p.gen_t = gen_t; p.gen_act = gen_act; p.out_split = out_split ? 1 : 0;
    return sep_run(p, B, precision, stream, "emd_sep3x3_fused_gen_f32: Cout > 128 has no generated-input form");
}

extern "C" int emd_sep3x3_fused_f32(const float* x, int ldx, const float* dw, const uint16_t* whi,
                                    const uint16_t* wlo, const float* scale1, const float* shift1,
                                    const float* scale2, const float* shift2, const float* res, int ldres,
                                    float* y, int ldy, int B, int H, int W, int Cin, int Cout, int act,
                                    int precision, emd_stream_t stream) {
    return sep_fused_entry(x, ldx, dw, whi, wlo, scale1, shift1, scale2, shift2, res, ldres, y, ldy, B, H, W, Cin, Cout, act,
                           precision, 0, stream);
}

// emd_sep3x3_fused_f32 writing y as a split32 tensor (Cout % 32 == 0; pitch ldy 4-byte units, % 32): the producer of a split32
// convolution's input (graph D: deconv1_b -> deconv1to0) then writes no fp32 activation and needs no converter pass.
extern "C" int emd_sep3x3_fused_out_f32(const float* x, int ldx, const float* dw, const uint16_t* whi,
                                        const uint16_t* wlo, const float* scale1, const float* shift1,
                                        const float* scale2, const float* shift2, const float* res, int ldres,
                                        void* y, int ldy, int B, int H, int W, int Cin, int Cout, int act,
                                        emd_stream_t stream) {
    return sep_fused_entry(x, ldx, dw, whi, wlo, scale1, shift1, scale2, shift2, res, ldres, static_cast<float*>(y), ldy, B, H, W, Cin,
                           Cout, act, 3, 0, stream, nullptr, nullptr, 0, 1);
}

// The same with the depthwise stage reading the tf.pad(REFLECT, 1) border instead of zeros: graph G's
// strided_conv_block(stride 1, pad_size=(1,1)) (misc_py/gan-infilling-100.py:205-243); act is usually EMD_ACT_LEAKY.
extern "C" int emd_sep3x3_fused_reflect_f32(const float* x, int ldx, const float* dw, const uint16_t* whi,
                                            const uint16_t* wlo, const float* scale1, const float* shift1,
                                            const float* scale2, const float* shift2, const float* res, int ldres,
                                            float* y, int ldy, int B, int H, int W, int Cin, int Cout, int act,
                                            int precision, emd_stream_t stream) {
    return sep_fused_entry(x, ldx, dw, whi, wlo, scale1, shift1, scale2, shift2, res, ldres, y, ldy, B, H, W, Cin, Cout, act,
                           precision, 1, stream);
}

// The fused separable conv on a GENERATED input: the layer's Cin-channel input is act(d[pixel] * gen_a[c] + gen_t[c]), d a
// one-value-per-pixel tensor (pitch ldd floats) -- what emd_cin1_f32 / emd_cin1_k7_reflect_f32 would write out for the layer
// that follows the one fed by the 1-channel image (cnn0 -> cnn0_last, machine_learning/denoiser.py:252-255; the generator's first
// two layers, misc_py/gan-infilling-100.py:343-349).  The Cin-channel tensor never exists in memory.
extern "C" int emd_sep3x3_fused_gen_f32(const float* d, int ldd, const float* gen_a, const float* gen_t, int gen_act,
                                        const float* dw, const uint16_t* whi, const uint16_t* wlo, const float* scale1,
                                        const float* shift1, const float* scale2, const float* shift2, const float* res,
                                        int ldres, float* y, int ldy, int B, int H, int W, int Cin, int Cout, int act,
                                        int precision, int reflect, emd_stream_t stream) {
    EMD_REQUIRE(gen_a && gen_t, EMD_E_INVALID, "emd_sep3x3_fused_gen_f32: null gen_a / gen_t");
    return sep_fused_entry(d, ldd, dw, whi, wlo, scale1, shift1, scale2, shift2, res, ldres, y, ldy, B, H, W, Cin, Cout, act,
                           precision, reflect, stream, gen_a, gen_t, gen_act);
}

// The same layer taking the 1-channel image and the nine taps of its depthwise conv instead of d (graph D's cnn0 -> cnn0_last,
// machine_learning/denoiser.py:252-255): d = what emd_cin1_f32(img, w9, (1,0,0,0), 0, act = 0) writes is formed per tile inside the
// kernel (sep_fused.hip, sep_gen9_kernel), so neither d nor the Cin-channel tensor goes through memory.
extern "C" int emd_sep3x3_fused_gen9_f32(const float* img, const float* w9, const float* gen_a, const float* gen_t, int gen_act,
                                         const float* dw, const uint16_t* whi, const uint16_t* wlo, const float* scale1,
                                         const float* shift1, const float* scale2, const float* shift2, const float* res,
                                         int ldres, float* y, int ldy, int B, int H, int W, int Cin, int Cout, int act,
                                         int precision, int reflect, emd_stream_t stream) {
    static const SepEntry e{"emd_sep3x3_fused_gen9_f32",
                            "needs relu6 generation, zero padding, split-bf16, H%8==0, W%16==0, Cin 32 or 64, Cout%4==0, "
                            "Cout<=64 (use emd_cin1_f32 + emd_sep3x3_fused_gen_f32)",
                            kSpanOut, "pointers (but img, w9) must be 16-byte aligned", 1, false};
    SepParams p = sep_params(img, 1, dw, whi, wlo, scale1, shift1, scale2, shift2, res, ldres, y, ldy, H, W, Cin, Cout, act, 1, reflect);
    p.gen_a = gen_a; p.gen_t = gen_t; p.gen_act = gen_act; p.gen_w9 = w9;
    const int rc = sep_check(e, {{img, false, true}, {w9, false, true}, {gen_a}, {gen_t}, {dw}, {whi}, {wlo}, {scale1}, {shift1}, {y}, {res, true}},
                             scale2, shift2, B, H, W, sep_route(p, precision) == kSepGen9,
                             ldy > ldres ? ldy : ldres, {{ldy, Cout, true, true}, {ldres, Cout, res != nullptr, true}});
    if (rc) return rc;
    return sep_run(p, B, 3, stream);
}

// The stride-1 block whose output feeds only a 3x3 convolution to one channel (deconv0_b -> deconv_final, machine_learning/denoiser.py:
// 383-387), with that convolution's CHANNEL sum folded into the epilogue: y = the block's output (affine, activation, second affine,
// + res, the arithmetic of emd_sep3x3_fused_f32) is not stored; z[t][b][h][w] = sum_c wfin[t][c] * y[b][h][w][c], t = 0..8, is -- nine
// planes of B*H*W floats.  emd_cout1_gather9_f32 adds the nine shifted planes.
extern "C" int emd_sep3x3_fused_fold_f32(const float* x, int ldx, const float* dw, const uint16_t* whi, const uint16_t* wlo,
                                         const float* scale1, const float* shift1, const float* scale2, const float* shift2,
                                         const float* res, int ldres, const float* wfin, float* z, int B, int H, int W, int Cin, int Cout,
                                         int act, emd_stream_t stream) {
    static const SepEntry e{"emd_sep3x3_fused_fold_f32",
                            "needs H%8==0, W%16==0, Cin%32==0, Cout==64 (use emd_sep3x3_fused_f32 + emd_conv3x3_cout1_f32)", "9 image rows of the input must span fewer than 2^31 floats",
                            kAligned, 1, false};
    const int rc = sep_check(e, {{x}, {dw}, {whi}, {wlo}, {scale1}, {shift1}, {wfin}, {z}, {res, true}}, scale2, shift2, B, H, W,
                             emd_sep3x3_fused_fold_supported(H, W, Cin, Cout), ldx > ldres ? ldx : ldres,
                             {{ldx, Cin, true, true}, {ldres, Cout, res != nullptr, true}});
    if (rc) return rc;
    SepParams p = sep_params(x, ldx, dw, whi, wlo, scale1, shift1, scale2, shift2, res, ldres, nullptr, 0, H, W, Cin, Cout, act, 1, 0);
    p.fold_w = wfin; p.fold_z = z; p.fold = 1;
    return sep_run(p, B, 3, stream);
}

// The stride-2 separable block (strided_conv_block(stride=2), machine_learning/denoiser.py:258, :273, :288) in one launch: x [B,H,W,Cin]
// (H, W even; TF SAME = no padding before, one pixel after) -> y [B,H/2,W/2,Cout].  Split-bf16.  Same arithmetic as emd_dw3x3_f32(stride 2)
// followed by emd_conv1x1_f32; the depthwise result never exists in memory.  Only sep_pipe.hip has the form (STRIDE = 2): even sizes with
// H % 8 == 0, W % 32 == 0 (output tiles of 4 x 16 pixels), Cout <= 256.  _reflect and _genres share the checks and report under this name.
struct GenRes {   // the generated residual of emd_sep3x3_fused_s2_genres_f32 (SepParams::rg_*)
    const float* img;
    int ld, stride;
    const float* a;
    const float* t;
    int act;
};

static int sep_s2_entry(const float* x, int ldx, const float* dw, const uint16_t* whi, const uint16_t* wlo, const float* scale1,
                        const float* shift1, const float* scale2, const float* shift2, const float* res, int ldres, float* y, int ldy,
                        int B, int H, int W, int Cin, int Cout, int act, int reflect, emd_stream_t stream, const GenRes* gr = nullptr) {
    static const SepEntry e{"emd_sep3x3_fused_s2_f32", "needs H%8==0, W%32==0, Cin%32==0, Cout%4==0, Cout<=256 (use emd_dw3x3_f32 + emd_conv1x1_f32)",
                            kSpanOut, kAligned, 2, true};
    const int rc = sep_check(e, {{x}, {dw}, {whi}, {wlo}, {scale1}, {shift1}, {y}, {res, true}}, scale2, shift2, B, H, W,
                             emd_sep3x3_fused_supported(H, W, Cin, Cout, 2, 1), ldy > ldres ? ldy : ldres,
                             {{ldx, Cin, true, true}, {ldy, Cout, true, true}, {ldres, Cout, res != nullptr, true}});
    if (rc) return rc;
    SepParams p = sep_params(x, ldx, dw, whi, wlo, scale1, shift1, scale2, shift2, res, ldres, y, ldy, H, W, Cin, Cout, act, 2, reflect);
    if (gr) {
        p.rg_x = gr->img; p.rg_ld = gr->ld; p.rg_stride = gr->stride; p.rg_a = gr->a; p.rg_t = gr->t; p.rg_act = gr->act;
    }
    return sep_run(p, B, 3, stream, "emd_sep3x3_fused_s2_f32: the pipelined kernel is switched off (dev knob sep_pipe)");
}

extern "C" int emd_sep3x3_fused_s2_f32(const float* x, int ldx, const float* dw, const uint16_t* whi, const uint16_t* wlo,
                                       const float* scale1, const float* shift1, const float* scale2, const float* shift2,
                                       const float* res, int ldres, float* y, int ldy, int B, int H, int W, int Cin, int Cout, int act,
                                       emd_stream_t stream) {
    return sep_s2_entry(x, ldx, dw, whi, wlo, scale1, shift1, scale2, shift2, res, ldres, y, ldy, B, H, W, Cin, Cout, act, 0, stream);
}

// The same with the depthwise stage on the tf.pad(REFLECT, 1) image and VALID padding: graph G's strided_conv_block(stride 2,
// pad_size = (1, 1)) (misc_py/gan-infilling-100.py:205-243, the down-sampling layers :345-352): output pixel (i, j) reads input rows
// 2 i - 1 .. 2 i + 1 (row -1 = row 1); on even sizes nothing is read beyond the last row / column.
extern "C" int emd_sep3x3_fused_s2_reflect_f32(const float* x, int ldx, const float* dw, const uint16_t* whi, const uint16_t* wlo,
                                               const float* scale1, const float* shift1, const float* scale2, const float* shift2,
                                               const float* res, int ldres, float* y, int ldy, int B, int H, int W, int Cin, int Cout,
                                               int act, emd_stream_t stream) {
    return sep_s2_entry(x, ldx, dw, whi, wlo, scale1, shift1, scale2, shift2, res, ldres, y, ldy, B, H, W, Cin, Cout, act, 1, stream);
}

// The same block with the residual GENERATED in the epilogue: res[b][oy][ox][c] = f(img[b][oy * img_stride][ox * img_stride] * res_a[c] +
// res_t[c]), f = relu6 if res_act else the identity -- what emd_cin1_f32(img, NULL, res_a, res_t, ..., stride = img_stride, res_act) writes
// for a residual projection of the 1-channel image (residual0 of graph D, machine_learning/denoiser.py:252: a 1x1 conv of one channel is
// rank 1), same fma, same clamp; that tensor is then neither written nor read.  Cout <= 128.
extern "C" int emd_sep3x3_fused_s2_genres_f32(const float* x, int ldx, const float* dw, const uint16_t* whi, const uint16_t* wlo,
                                              const float* scale1, const float* shift1, const float* scale2, const float* shift2,
                                              const float* img, int ldimg, int img_stride, const float* res_a, const float* res_t,
                                              int res_act, float* y, int ldy, int B, int H, int W, int Cin, int Cout, int act,
                                              emd_stream_t stream) {
    EMD_REQUIRE(img && res_a && res_t, EMD_E_INVALID, "emd_sep3x3_fused_s2_genres_f32: null pointer");
    EMD_REQUIRE(ldimg >= 1 && img_stride >= 1, EMD_E_INVALID, "emd_sep3x3_fused_s2_genres_f32: image pitch and sampling stride must be >= 1");
    // what emd_cin1_f32 takes (stride 1 or 2; Cout / 4 a divisor of 64: the predicate), so that the promised equivalence has a left-hand
    // side; the pixel pitch is the one thing beyond it (d as channel 0 of a wider scratch tensor, as emd_sep3x3_fused_gen_f32 takes it)
    EMD_REQUIRE(img_stride <= 2 && ldimg <= 64, EMD_E_UNSUPPORTED, "emd_sep3x3_fused_s2_genres_f32: sampling stride 1 or 2, image pitch <= 64");
    EMD_REQUIRE(emd_sep3x3_fused_s2_genres_supported(H, W, Cin, Cout), EMD_E_UNSUPPORTED,
                "emd_sep3x3_fused_s2_genres_f32: needs H%8==0, W%32==0, Cin%32==0, Cout%4==0, Cout<=128 (use emd_cin1_f32 + emd_sep3x3_fused_s2_f32)");
    const GenRes gr{img, ldimg, img_stride, res_a, res_t, res_act ? 1 : 0};
    return sep_s2_entry(x, ldx, dw, whi, wlo, scale1, shift1, scale2, shift2, nullptr, 0, y, ldy, B, H, W, Cin, Cout, act, 0, stream, &gr);
}

// The decoder pair "separable conv + 1x1 residual projection of the same input" in ONE launch (machine_learning/denoiser.py:356-359,
// :368-371, :380-383: deconv*_a = strided_conv_block(concat) and residual*_d = conv_block_not_sep(concat, kernel_size=1)):
//   y  = relu6(BN2(BN1(pointwise(depthwise3x3(x)))))        the fused separable conv of emd_sep3x3_fused_f32 (scale1 / shift1)
//   y2 = relu6(BN(x * W2 + bias))                           a 1x1 conv of x itself (scale_b / shift_b: bias and BN folded)
// Both read the 384- or 128-channel input, the largest tensors of the decoder; fused, it comes from HBM once.  The input patch of
// a tile is staged in LDS for the depthwise stage anyway; its centre pixels are the projection's A operand.
extern "C" int emd_sep3x3_dual_f32(const float* x, int ldx, const float* dw, const uint16_t* whi, const uint16_t* wlo,
                                   const float* scale1, const float* shift1, float* y, int ldy, const uint16_t* w2hi,
                                   const uint16_t* w2lo, const float* scale_b, const float* shift_b, float* y2, int ldy2, int B, int H,
                                   int W, int Cin, int Cout, int Cout2, int act, emd_stream_t stream) {
    static const SepEntry e{"emd_sep3x3_dual_f32",
                            "needs H%8==0 (H%4==0 above 64 output channels), W%16==0, Cin%32==0, Cout%4==0, Cout<=128 (both outputs)",
                            "9 image rows of an output must span fewer than 2^31 floats", kAligned, 1, false};
    const int rc = sep_check(e, {{x}, {dw}, {whi}, {wlo}, {scale1}, {shift1}, {y}, {w2hi}, {w2lo}, {scale_b}, {shift_b}, {y2}}, nullptr, nullptr, B,
                             H, W, emd_sep3x3_dual_supported(H, W, Cin, Cout, Cout2), ldy > ldy2 ? ldy : ldy2,
                             {{ldx, Cin, true, true}, {ldy, Cout, true, true}, {ldy2, Cout2, true, true}},
                             {{kAfterAlign, y != y2, EMD_E_INVALID, "emd_sep3x3_dual_f32: the two outputs alias"}});
    if (rc) return rc;
    SepParams p = sep_params(x, ldx, dw, whi, wlo, scale1, shift1, nullptr, nullptr, nullptr, 0, y, ldy, H, W, Cin, Cout, act, 1, 0);
    p.W2hi = w2hi; p.W2lo = w2lo; p.y2 = y2; p.scale_b = scale_b; p.shift_b = shift_b; p.N2 = Cout2; p.ldy2 = ldy2;
    return sep_run(p, B, 3, stream);
}
