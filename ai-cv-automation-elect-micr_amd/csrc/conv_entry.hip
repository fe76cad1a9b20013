// Dense, pointwise and transposed convolutions, host side only: the C entry points on fp32 input (emd_conv1x1_f32, emd_conv3x3_f32,
// emd_deconv3x3s2_f32, their *_stats[_fold]_f32 forms, ...) and the 3x3 and transposed convs on split32 input (emd_conv3x3_split32_f32,
// emd_deconv3x3s2[_fused]_split32_f32), in four parts: one ladder of argument checks per input format, the geometry (TF-SAME conv, a
// phase of the transposed conv, packed taps) that fills both parameter families, the plan (conv_plan: which kernel of gemm_conv.hip,
// conv_split.hip, conv3_pipe.hip or deconv_pipe.hip takes a launch, on which tiles, with which grid), and the entries.  Every routing
// rule and every dev knob of these entries is read here and nowhere else; the kernel files map a plan to a template instance.
// emd_debug_conv_plan shows the plan without a device.  (The pointwise GEMM on split32 input keeps its entries in gemm_split.hip.)
#include <utility>

#include "conv_plan.hpp"
#include "bn_chain_dev.hpp"

using namespace emd;

namespace {

int say(int code, const char* who, const char* what) {
    set_error("%s: %s", who, what);
    return code;
}
bool aligned128(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 127u) == 0; }
int ceil_to(int n, int t) { return (n + t - 1) / t * t; }

// ------------------------------------------------------------------------------------------------------------------------------
// Argument checks, fp32 input.  One ladder, whose messages all start with "conv:" whatever the entry; then the entry's own steps under
// its own name, as its descriptor says.  The first failing step decides the code and the text.
int f32_ladder(const float* x, const void* whi, const void* wlo, const float* scale1, const float* shift1, const float* scale2,
               const float* shift2, const float* res, float* y, int Cin, int N, int ldx, int ldy, int ldres, int passes) {
    EMD_REQUIRE(x && whi && scale1 && shift1 && y, EMD_E_INVALID, "conv: null pointer");
    EMD_REQUIRE(passes == 1 || passes == 3, EMD_E_INVALID, "conv: precision must be EMD_PREC_BF16 or EMD_PREC_BF16X3");
    EMD_REQUIRE(passes == 1 || wlo, EMD_E_INVALID, "conv: the split-bf16 mode needs the lo weight plane");
    EMD_REQUIRE((scale2 == nullptr) == (shift2 == nullptr), EMD_E_INVALID, "conv: scale2/shift2 must come together");
    EMD_REQUIRE(Cin >= 4 && N >= 1, EMD_E_INVALID, "conv: bad channel counts");
    EMD_REQUIRE(Cin % 4 == 0 && ldx % 4 == 0 && ldx >= Cin, EMD_E_ALIGN, "conv: Cin and ldx must be multiples of 4, ldx >= Cin");
    EMD_REQUIRE(ldy >= N && (!res || ldres >= N), EMD_E_INVALID, "conv: ldy/ldres smaller than Cout");
    EMD_REQUIRE(N % 4 == 0 && ldy % 4 == 0 && aligned16(y) && (!res || (ldres % 4 == 0 && aligned16(res))),
                EMD_E_ALIGN, "conv: Cout, ldy, ldres must be multiples of 4 and y, res 16-byte aligned");
    EMD_REQUIRE(aligned16(scale1) && aligned16(shift1) && (!scale2 || (aligned16(scale2) && aligned16(shift2))),
                EMD_E_ALIGN, "conv: scale/shift vectors must be 16-byte aligned");
    EMD_REQUIRE(aligned16(x) && aligned16(whi) && (!wlo || aligned16(wlo)), EMD_E_ALIGN,
                "conv: x and the weight planes must be 16-byte aligned");
    return EMD_OK;
}

struct F32Entry {
    const char* who;     // the name the entry's own steps carry
    int k;               // kernel size: 1 or 3
    bool table;          // whi / wlo are tables of four planes: the phases of the transposed conv
    bool stats;          // batch statistics of the output: 1 <= B <= 65535, no empty batch
    bool strided;        // takes a stride, 1 or 2
    const char* rate;    // the sentence of its rate rule, or null
    bool transposed;     // the data gradient of the stride-2 1x1 conv: the row map of that conv with source and destination exchanged
};
struct F32Args {         // what every fp32-input entry passes, in the order of emd_conv3x3_f32
    const float* x; int ldx;
    const void* whi; const void* wlo;   // planes, or tables of four
    const float *scale1, *shift1, *scale2, *shift2, *res; int ldres;
    float* y; int ldy, B, H, W, Cin, N, stride, rate, act, passes;
};
const uint16_t* plane(const void* w, bool table, int ph) {
    return table ? (w ? static_cast<const uint16_t* const*>(w)[ph] : nullptr) : static_cast<const uint16_t*>(w);
}

int f32_checks(const F32Entry& e, const F32Args& a) {
    if (e.table && !a.whi) return say(EMD_E_INVALID, e.who, "null weight table");
    for (int ph = 0; ph < (e.table ? 4 : 1); ++ph)
        if (int rc = f32_ladder(a.x, plane(a.whi, e.table, ph), plane(a.wlo, e.table, ph), a.scale1, a.shift1, a.scale2, a.shift2, a.res, a.y,
                                a.Cin, a.N, a.ldx, a.ldy, a.ldres, a.passes))
            return rc;
    if (!(a.B >= (e.stats ? 1 : 0) && (!e.stats || a.B <= 65535) && a.H >= 1 && a.W >= 1)) return say(EMD_E_INVALID, e.who, "bad shape");
    if (e.strided && a.stride != 1 && a.stride != 2) return say(EMD_E_UNSUPPORTED, e.who, "stride must be 1 or 2");
    if (e.rate && !(a.rate >= 1 && a.rate <= 31 && (a.rate == 1 || a.stride == 1))) return say(EMD_E_UNSUPPORTED, e.who, e.rate);
    return EMD_OK;
}

// Argument checks, split32 input: the 3x3 and the transposed convs report as "split32 conv".
int split_checks(const void* xs, int ldx, const uint16_t* whi, const uint16_t* wlo, const float* scale1, const float* shift1, const float* scale2,
                 const float* shift2, const float* res, int ldres, const void* y, int ldy, int Cin, int Cout, int out_split) {
    EMD_REQUIRE(xs && whi && wlo && scale1 && shift1 && y, EMD_E_INVALID, "split32 conv: null pointer");
    EMD_REQUIRE((scale2 == nullptr) == (shift2 == nullptr), EMD_E_INVALID, "split32 conv: scale2/shift2 must come together");
    EMD_REQUIRE(Cin >= 1 && Cin <= 2048 && Cout >= 4 && Cout % 4 == 0, EMD_E_INVALID, "split32 conv: 1 <= Cin <= 2048, Cout a multiple of 4");
    EMD_REQUIRE(ldx % 32 == 0 && ldx >= emd_split32_ld(Cin) && aligned128(xs), EMD_E_ALIGN,
                "split32 conv: xs 128-byte aligned, ldx a multiple of 32, >= ceil32(Cin)");
    if (out_split)
        EMD_REQUIRE(ldy % 32 == 0 && ldy >= emd_split32_ld(Cout) && aligned128(y), EMD_E_ALIGN,
                    "split32 conv: split32 output needs y 128-byte aligned, ldy a multiple of 32, >= ceil32(Cout)");
    else
        EMD_REQUIRE(ldy % 4 == 0 && ldy >= Cout && aligned16(y), EMD_E_ALIGN, "split32 conv: ldy a multiple of 4, >= Cout; y 16-byte aligned");
    EMD_REQUIRE(!res || (ldres % 4 == 0 && ldres >= Cout && aligned16(res)), EMD_E_ALIGN, "split32 conv: res alignment");
    EMD_REQUIRE(aligned16(scale1) && aligned16(shift1) && (!scale2 || (aligned16(scale2) && aligned16(shift2))) && aligned16(whi) && aligned16(wlo),
                EMD_E_ALIGN, "split32 conv: weight planes and scale/shift vectors must be 16-byte aligned");
    return EMD_OK;
}

// The transposed convs on split32 input: the table, the ladder once per phase, the shape.
int split_deconv_checks(const char* who, const void* xs, int ldx, const uint16_t* const whi[4], const uint16_t* const wlo[4], const float* scale1,
                        const float* shift1, const void* y, int ldy, int B, int H, int W, int Cin, int Cout, int out_split) {
    if (!(whi && wlo)) return say(EMD_E_INVALID, who, "null weight table");
    for (int ph = 0; ph < 4; ++ph)
        if (int rc = split_checks(xs, ldx, whi[ph], wlo[ph], scale1, shift1, nullptr, nullptr, nullptr, 0, y, ldy, Cin, Cout, out_split))
            return rc;
    if (!(B >= 0 && H >= 1 && W >= 1)) return say(EMD_E_INVALID, who, "bad shape");
    return EMD_OK;
}

// ------------------------------------------------------------------------------------------------------------------------------
// Geometry: the row map of an implicit GEMM.  Row m = (b, i, j) on Hg x Wg reads, for tap t, source pixel (b, i * sa + dy_t, j * sa + dx_t)
// of Ha x Wa (zero outside) and writes pixel (b, i * sc + py, j * sc + px) of Hc x Wc; the tap offsets are packed 7 bits each, biased by 64.
struct ConvGeom {
    long M;
    int flat, Hg, Wg, Ha, Wa, Hc, Wc, sa, sc, py, px, ntaps;
    unsigned long long dyp, dxp;
};

void set_taps(ConvGeom& g, int n, const int* dy, const int* dx) {
    g.ntaps = n;
    g.dyp = g.dxp = 0;
    for (int t = 0; t < n; ++t) {
        g.dyp |= (unsigned long long)(dy[t] + 64) << (7 * t);
        g.dxp |= (unsigned long long)(dx[t] + 64) << (7 * t);
    }
}

// k x k conv with TF SAME padding, stride 1 or 2, dilation `rate`: tap (ky, kx) reads source pixel (i * s + ky * rate - pad_top,
// j * s + kx * rate - pad_left).  k = 1: no padding, samples x[0::s]; at stride 1 source pixel = destination pixel = m (flat).
ConvGeom same_conv(int B, int H, int W, int k, int stride, int rate) {
    ConvGeom g{};
    const int Ho = (H + stride - 1) / stride, Wo = (W + stride - 1) / stride, eff = (k - 1) * rate + 1;
    const int pth = (Ho - 1) * stride + eff - H, ptw = (Wo - 1) * stride + eff - W;   // total padding
    const int pt = pth < 0 ? 0 : pth / 2, pl = ptw < 0 ? 0 : ptw / 2;
    g.M = (long)B * Ho * Wo;
    g.flat = k == 1 && stride == 1;
    g.Hg = Ho; g.Wg = Wo; g.Ha = H; g.Wa = W; g.Hc = Ho; g.Wc = Wo; g.sa = stride; g.sc = 1;
    int dy[9], dx[9];
    for (int ky = 0; ky < k; ++ky)
        for (int kx = 0; kx < k; ++kx) {
            dy[ky * k + kx] = ky * rate - pt;
            dx[ky * k + kx] = kx * rate - pl;
        }
    set_taps(g, k * k, dy, dx);
    return g;
}

// Phase ph = 2 py + px of the 3x3 stride-2 transposed conv: y[2i+k] += x[i]*w[k] cropped to [0,2N) (gradient of the SAME stride-2 conv,
// denoiser.py:141-148) -- even output index 2i: taps k=0 (from x[i]) and k=2 (from x[i-1]); odd 2i+1: tap k=1 (from x[i]).  The four
// (row-parity, column-parity) phases are four GEMMs over the INPUT grid with 4/2/2/1 taps, each with its own packed weight block.
ConvGeom deconv_phase(int B, int H, int W, int ph) {
    ConvGeom g{};
    int ky[4], kx[4], dy[4], dx[4];
    const int n = emd_deconv_phase_taps(ph, ky, kx);
    for (int t = 0; t < n; ++t) {   // kernel index 2 reads the previous input sample
        dy[t] = ky[t] == 2 ? -1 : 0;
        dx[t] = kx[t] == 2 ? -1 : 0;
    }
    g.M = (long)B * H * W;
    g.Hg = H; g.Wg = W; g.Ha = H; g.Wa = W; g.Hc = 2 * H; g.Wc = 2 * W; g.sa = 1; g.sc = 2; g.py = ph >> 1; g.px = ph & 1;
    set_taps(g, n, dy, dx);
    return g;
}

template <class P>   // GemmParams or SplitConvParams (whose M is in its GEMM block)
void put_geom(P& p, const ConvGeom& g) {
    p.flat = g.flat; p.ntaps = g.ntaps; p.dyp = g.dyp; p.dxp = g.dxp;
    p.Hg = g.Hg; p.Wg = g.Wg; p.Ha = g.Ha; p.Wa = g.Wa; p.Hc = g.Hc; p.Wc = g.Wc; p.sa = g.sa; p.sc = g.sc; p.py = g.py; p.px = g.px;
}

// ------------------------------------------------------------------------------------------------------------------------------
// The plan.  What a launch is asked for: the entry, the layer, the form.  The flag bits and the operations are emd_debug_conv_plan's.
enum : unsigned { kRes = 1, kAffine2 = 2, kOutSplit = 4, kStats = 8, kUp = 16 };
enum ConvOp { kOpConv1, kOpConv3, kOpDeconv, kOpConv1Bwd, kOpSplitConv3, kOpSplitDeconv, kOpSplitDeconvFused };
struct ConvAsk {
    int op, B, H, W, Cin, N, stride, rate, passes;
    unsigned flags;
    long ldx, ldy;        // pixel pitches in the entry's units
};

long tiles(long n, int t) { return (n + t - 1) / t; }

ConvPlan refuse(const char* why) {
    ConvPlan pl{};
    pl.refuse = why;
    return pl;
}
// fp32 input, gemm_conv_kernel: 128-row tiles of 128 columns, or of 64 where N <= 64 and where a grid cannot even give every CU one
// 128x128 tile (a single 32x32 training tower: 8 x 6 tiles): twice the workgroups, each latency-bound pass over K shorter.
ConvPlan plan_gemm(const ConvAsk& a, long M) {
    ConvPlan pl{};
    pl.route = (a.flags & kUp) ? kGemmConvUp : kGemmConv;
    pl.bm = 128;
    pl.bn = (a.N <= 64 || tiles(M, 128) * tiles(a.N, 128) < 192) ? 64 : 128;
    pl.threads = 256;
    pl.passes = a.passes;
    pl.form = (a.op == kOpConv1 && a.stride == 1) ? 1 : 0;   // flat
    pl.launches = a.op == kOpDeconv ? 4 : 1;
    pl.n_mtiles = (int)tiles(M, 128);
    pl.n_ntiles = (int)tiles(a.N, pl.bn);
    const long nblk = (long)pl.n_mtiles * pl.n_ntiles;
    if (nblk <= 0 || nblk > 0x7fffffffL) return refuse("gemm_conv: grid too large");
    pl.grid = dim3((unsigned)nblk);
    return pl;
}

// Tiles per workgroup of the patch-resident kernels (8 x 32 pixels, 64 columns), side by side along W: the largest of 8, 4, 2 that divides
// the tiles of a row and leaves 1024 workgroups; the dev knob sep_tpw (shared with the separable kernels) overrides where it divides.
// Their epilogue width is a rule of each kernel (dev knob epi_width overrides).
void patch_grid(ConvPlan& pl, const ConvAsk& a, int B) {
    const int tiles_w = a.W / 32;
    pl.bm = 256; pl.bn = 64; pl.threads = 512;
    pl.n_ntiles = (int)tiles(a.N, 64);
    const long wgs1 = (long)tiles_w * (a.H / 8) * B * pl.n_ntiles;
    pl.tpw = 1;
    for (int t = 8; t >= 2; t >>= 1)
        if (tiles_w % t == 0 && wgs1 / t >= 1024) { pl.tpw = t; break; }
    if (g_knobs.sep_tpw > 0 && tiles_w % g_knobs.sep_tpw == 0) pl.tpw = g_knobs.sep_tpw;
    pl.grid = dim3(tiles_w / pl.tpw * pl.n_ntiles, a.H / 8, B);
    pl.form = (a.flags & kOutSplit) ? 1 : 0;
}

// ONE predicate for "this transposed conv runs on the patch-resident kernel" (deconv_pipe.hip), used by emd_deconv3x3s2_fused_preferred and
// by the entry point alike, and a function of the LAYER only (H, W, Cin, Cout) -- never of the batch size or of the pitches: the kernel sums
// in another order than the GEMM forms, so a route that flipped with B (or with the buffer a tensor happens to live in) would break "image b
// of a batch == the image alone, bit for bit".  What the kernel additionally needs of a call (32-bit in-image offsets) is checked by the
// plan and REPORTED (EMD_E_UNSUPPORTED) instead of silently falling back to a kernel with other bits; batches beyond the grid's 65535
// images are cut into launches of the same kernel.
bool deconv_patch_route(int H, int W, int Cin, int Cout) {
    return g_knobs.deconv_direct == 3 && Cin % 32 == 0 && Cin >= 32 && Cin <= 4064 && H >= 8 && H % 8 == 0 && W % 32 == 0 && Cout % 4 == 0 && Cout <= 1024;
}

// The 3x3 and transposed convs on split32 input.  gemm_split_conv_kernel: 256-row tiles of 64 (N <= 64) or 128 columns; pixel indices in 32 bits.
ConvPlan plan_split_conv(const ConvAsk& a, long M) {
    const bool out_split = a.flags & kOutSplit, fused = a.op == kOpSplitDeconvFused;
    ConvPlan pl{};
    pl.launches = a.op == kOpSplitDeconv ? 4 : 1;
    pl.nt = split_nt(0);   // non-temporal output stores (split_params.hpp: dev knob nt_mask, bit 0)
    // conv3_pipe.hip, the patch-resident kernel: stride 1, rate 1, no residual, whole 8 x 32 tiles, up to 256 columns (measured,
    // tools/conv3_bench.py: faster up to 192 columns, 3-4 % at 256; knob conv3_pipe = 2: up to 1024, 0: never; column tiles of 64: the
    // packed weight planes are padded to a multiple of 128 rows, so a last partial tile stays inside them).  A rule of the layer, not of B.
    if (a.op == kOpSplitConv3 && a.stride == 1 && a.rate == 1 && !(a.flags & kRes) && a.H >= 8 && a.B <= 65535 && 9L * a.W * a.ldy < (1L << 31) &&
        g_knobs.conv3_pipe && a.H % 8 == 0 && a.W % 32 == 0 && a.N <= (g_knobs.conv3_pipe >= 2 ? 1024 : 256)) {
        pl.route = kConv3Pipe;
        patch_grid(pl, a, a.B);
        pl.epi = (g_knobs.epi_width ? g_knobs.epi_width == 4 : pl.n_ntiles >= 4) ? 4 : 1;   // four or more column tiles do better with the transposed 16-byte form
        return pl;
    }
    if (fused && deconv_patch_route(a.H, a.W, a.Cin, a.N)) {
        if (!((long)a.H * a.W * a.ldx * 4 < (1L << 32) && 36L * a.W * a.ldy < (1L << 31)))
            return refuse("emd_deconv3x3s2_fused_split32_f32: this layer runs on the patch-resident kernel, whose in-image offsets are 32-bit "
                          "(H * W * ldx * 4 < 2^32, 36 * W * ldy < 2^31): pitch too large (a fallback would change the summation order)");
        pl.route = kDeconvPipe;
        pl.launches = (int)tiles(a.B, 65535);   // grid.z <= 65535: the same kernel on slices of the batch
        patch_grid(pl, a, a.B < 65535 ? a.B : 65535);
        pl.epi = (g_knobs.epi_width && g_knobs.epi_width != 1) ? 4 : 1;
        pl.ablate = g_knobs.sep_ablate;
        return pl;
    }
    pl.bm = 256;
    pl.bn = a.N <= 64 ? 64 : 128;
    pl.threads = 512;
    pl.n_mtiles = (int)tiles(M, 256);
    pl.n_ntiles = (int)tiles(a.N, pl.bn);
    long nblk = (long)pl.n_mtiles * pl.n_ntiles;
    if (nblk <= 0 || nblk > 0x7fffffffL) return refuse("split32 conv: grid too large");
    if (M > 0x7fffffffL || (long)a.B * a.H * a.W > 0x7fffffffL) return refuse("split32 conv: more than 2^31 pixels");
    // the one-launch transposed conv: knob deconv_direct = 0 the LDS-staged epilogue, 2 = 128-row tiles, two workgroups per CU, else
    // (round 3) the epilogue from the registers with the next phase's DMA first; a split32 output has the LDS-staged form only
    pl.route = !fused ? kConvSplit : (out_split || !g_knobs.deconv_direct) ? kDeconvFour : g_knobs.deconv_direct == 2 ? kDeconvHalf : kDeconvSplit;
    if (pl.route == kDeconvHalf) {
        pl.bm = 128; pl.threads = 256;
        pl.n_mtiles = (int)tiles(M, 128);
        nblk = (long)pl.n_mtiles * pl.n_ntiles;
        if (nblk > 0x7fffffffL) return refuse("split32 conv: grid too large");
    }
    pl.grid = dim3((unsigned)nblk);
    return pl;
}

// A pure function of its argument and the knobs.
ConvPlan conv_plan(const ConvAsk& a) {
    const int s = a.op == kOpConv1Bwd ? 2 : ((a.op == kOpConv1 || a.op == kOpConv3 || a.op == kOpSplitConv3) && a.stride > 1) ? a.stride : 1;
    const long M = (long)a.B * tiles(a.H, s) * tiles(a.W, s);   // rows of the GEMM forms
    return a.op <= kOpConv1Bwd ? plan_gemm(a, M) : plan_split_conv(a, M);
}

// ------------------------------------------------------------------------------------------------------------------------------
// Running a plan.

// fp32 input: one launch, or the four phases of the transposed conv; with `so`, the batch statistics of the output from the epilogues.
struct StatsOut {
    int images;           // per-image statistics ([B][N]) instead of [N]
    float* mean;
    float* var;
    void* workspace;
    const BnFoldArgs* fold;
};

int f32_run(const F32Entry& e, const F32Args& a, emd_stream_t stream, const UpSample* up = nullptr, const StatsOut* so = nullptr) {
    if (a.B == 0) return EMD_OK;
    const ConvAsk ask{e.transposed ? kOpConv1Bwd : e.table ? kOpDeconv : e.k == 1 ? kOpConv1 : kOpConv3, a.B, a.H, a.W, a.Cin, a.N, a.stride, a.rate,
                      a.passes, up ? kUp : 0u, a.ldx, a.ldy};
    const ConvPlan pl = conv_plan(ask);
    if (!pl.route) return fail(EMD_E_UNSUPPORTED, pl.refuse);
    hipStream_t st = static_cast<hipStream_t>(stream);
    GemmParams p{};
    p.A = a.x; p.C = a.y; p.res = a.res;
    p.scale1 = a.scale1; p.shift1 = up ? nullptr : a.shift1; p.scale2 = a.scale2; p.shift2 = a.shift2;
    p.N = a.N; p.Cin = a.Cin; p.Cpad = ceil_to(a.Cin, kBK);
    p.lda = a.ldx; p.ldc = a.ldy; p.ldres = a.ldres; p.act = a.act;
    p.n_mtiles = pl.n_mtiles; p.n_ntiles = pl.n_ntiles;
    long npix_img = 0;
    for (int ph = 0; ph < pl.launches; ++ph) {
        ConvGeom g = e.table ? deconv_phase(a.B, a.H, a.W, ph) : same_conv(a.B, a.H, a.W, e.k, a.stride, a.rate);
        if (e.transposed) { std::swap(g.Ha, g.Hc); std::swap(g.Wa, g.Wc); std::swap(g.sa, g.sc); }
        put_geom(p, g);
        p.M = g.M;
        p.Whi = plane(a.whi, e.table, ph); p.Wlo = plane(a.wlo, e.table, ph);
        npix_img = (long)g.Hg * g.Wg;
        if (so) {   // (always 128-row tiles: the number of partials per image must not depend on the column tile the plan picks)
            p.stats_part = static_cast<double*>(so->workspace);
            p.stats_nph = e.table ? 4 : 0; p.stats_ph = ph; p.stats_tpi = so->images ? (int)(npix_img / 128) : pl.n_mtiles;
        }
        if (int rc = gemm_conv_launch(pl, p, up, st)) return rc;
    }
    if (!so) return EMD_OK;
    const int tpi = so->images ? (int)(npix_img / 128) : pl.n_mtiles;
    return launch_bn_stats_final(p.stats_part, pl.launches * tpi, a.N, pl.launches * (so->images ? npix_img : p.M), so->mean, so->var, st, nullptr,
                                 nullptr, 0.f, nullptr, nullptr, so->images ? a.B : 1, so->fold);
}

// The convolutions of a TRAINING forward pass (misc_py/denoiser-multi-gpu.py:200-540 with phase = True: every conv is followed by a batch
// norm on batch statistics): y = conv(x) with no affine and no activation, plus the per-channel mean and biased variance of y gathered in
// the GEMM's epilogue (one partial per 128-row tile, reduced in a fixed order by bn_stats_final): what emd_bn_stats_f32 /
// emd_bn_stats_images_f32 would return for y, without their pass over it.  images = 0: statistics over all output pixels (mean / var
// [Cout]); images = 1: per image ([B][Cout]; needs 128 | pixels of the GEMM's grid per image so that no tile straddles two images:
// EMD_E_UNSUPPORTED otherwise -- call the conv and the statistics separately).  With a fold block, the training-mode fold of the norm
// behind the conv rides in the statistics' final kernel (emd_bn_train_fold[_images]_f32's step; one launch less).  The transposed conv
// converts the fold block before the common checks and names itself in the two statistics steps; the others convert it after.
int f32_stats(const F32Entry& e, const F32Args& a, int images, float* mean, float* var, void* workspace, const emd_bn_train_fold_t* fold,
              emd_stream_t stream) {
    BnFoldArgs fa;
    if (e.table && !a.whi) return say(EMD_E_INVALID, e.who, "null weight table");
    if (e.table && fold)
        if (int rc = bn_fold_args(fold, &fa)) return rc;
    if (int rc = f32_checks(e, a)) return rc;
    if (!e.table && fold)
        if (int rc = bn_fold_args(fold, &fa)) return rc;
    const char* who = e.table ? e.who : "emd_conv*_stats_f32";
    if (!(mean && var && workspace && (reinterpret_cast<uintptr_t>(workspace) & 7) == 0))
        return say(EMD_E_INVALID, who, "mean, var and an 8-byte aligned workspace are required");
    const long npix_img = e.table ? (long)a.H * a.W : (long)tiles(a.H, a.stride) * tiles(a.W, a.stride);
    if (images && npix_img % 128 != 0) {
        set_error("%s: per-image statistics need %s %% 128 == 0 (a 128-row tile must not straddle two images)", who, e.table ? "H * W" : "Ho * Wo");
        return EMD_E_UNSUPPORTED;
    }
    const StatsOut so{images, mean, var, workspace, fold ? &fa : nullptr};
    return f32_run(e, a, stream, nullptr, &so);
}

const F32Entry kConv1{"emd_conv1x1_f32", 1, false, false, true}, kConv1Up{"emd_conv1x1_up_f32", 1},
    kConv3{"emd_conv3x3_f32", 3, false, false, true, "rate must be 1..31, and 1 when stride is 2"}, kDeconv{"emd_deconv3x3s2_f32", 3, true},
    kConv1Bwd{"emd_conv1x1_s2_bwd_data_f32", 1, false, false, false, nullptr, true}, kConv1Stats{"emd_conv1x1_stats_f32", 1, false, true, true},
    kConv3Stats{"emd_conv3x3_stats_f32", 3, false, true, false, "rate must be 1..31 (stride 1)"},
    kDeconvStats{"emd_deconv3x3s2_stats_f32", 3, true, true};

// split32 input: the GEMM block inside SplitConvParams, and the whole block
SplitGemmParams split_params(const void* xs, int ldx, const uint16_t* whi, const uint16_t* wlo, const float* scale1, const float* shift1,
                             const float* scale2, const float* shift2, const float* res, int ldres, void* y, int ldy, long M, int Cin, int Cout,
                             int act, const ConvPlan& pl) {
    SplitGemmParams p{};
    p.A = static_cast<const unsigned char*>(xs); p.Whi = whi; p.Wlo = wlo; p.C = static_cast<float*>(y); p.res = res;
    p.scale1 = scale1; p.shift1 = shift1; p.scale2 = scale2; p.shift2 = shift2;
    p.M = M; p.lda_bytes = (long)ldx * 4; p.N = Cout; p.Cin = Cin; p.Ktot = ceil_to(Cin, kBK);
    p.ldc = ldy; p.ldres = ldres; p.act = act;
    p.n_mtiles = pl.n_mtiles; p.n_ntiles = pl.n_ntiles; p.nt = pl.nt;
    return p;
}

SplitConvParams split_conv_params(const SplitGemmParams& gemm, const ConvGeom& g, int out_split) {
    SplitConvParams c{};
    c.g = gemm;
    put_geom(c, g);
    c.Cpad = c.g.Ktot; c.nkc = (c.g.Cin + SBK - 1) / SBK;
    c.g.Ktot = c.ntaps * c.Cpad;
    c.out_split = out_split ? 1 : 0;
    return c;
}

}  // namespace

// ------------------------------------------------------------------------------------------------------------------------------
// Predicates and dev hooks

// Where graph hosts should take the one-launch transposed conv (emd_deconv3x3s2_fused_split32_f32) rather than the register-staged
// four-phase GEMM: always where the patch-resident kernel covers the layer (deconv_patch_route), otherwise from 192 row tiles on (the GEMM
// forms agree with each other bit for bit, there the choice is speed only).
extern "C" int emd_deconv3x3s2_fused_preferred(int B, int H, int W, int Cin, int Cout) {
    if (deconv_patch_route(H, W, Cin, Cout)) return 1;
    return (long)B * H * W >= 256L * 192 ? 1 : 0;
}

// dev hook (include/emdenoise_dev.h), host only: the plan of a launch
extern "C" int emd_debug_conv_plan(int op, int B, int H, int W, int Cin, int Cout, int stride, int rate, int precision, unsigned flags, int ldx,
                                   int ldy, int out[12]) {
    if (op < kOpConv1 || op > kOpSplitDeconvFused) return 0;
    const bool split = op >= kOpSplitConv3;
    const ConvAsk ask{op, B, H, W, Cin, Cout, stride, rate, precision, flags, ldx ? ldx : split ? emd_split32_ld(Cin) : Cin,
                      ldy ? ldy : (flags & kOutSplit) ? emd_split32_ld(Cout) : Cout};
    const ConvPlan pl = conv_plan(ask);
    if (!pl.route || !out) return pl.route;
    const int v[12] = {pl.route, pl.bm, pl.bn, pl.threads, (int)pl.grid.x, (int)pl.grid.y, (int)pl.grid.z, pl.launches, pl.tpw, pl.epi, pl.nt, pl.form};
    for (int i = 0; i < 12; ++i) out[i] = v[i];
    return pl.route;
}

// ------------------------------------------------------------------------------------------------------------------------------
// Host packing: W [taps][Cin][Cout] (TF conv) or [taps][Cout][Cin] (conv2d_transpose) -> two bf16 planes (hi, lo), [Npad][taps*Cpad],
// K-contiguous per output channel, zero padded.
static uint16_t f32_to_bf16_rne(float f) {
    uint32_t u;
    __builtin_memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);  // NaN stays NaN
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
static float bf16_to_f32(uint16_t h) {
    uint32_t u = (uint32_t)h << 16;
    float f;
    __builtin_memcpy(&f, &u, 4);
    return f;
}

extern "C" size_t emd_packed_weight_elems(int taps, int Cin, int Cout) {
    if (taps < 1 || Cin < 1 || Cout < 1) return 0;
    const size_t cpad = (size_t)(Cin + kBK - 1) / kBK * kBK;
    const size_t npad = (size_t)(Cout + kNPadTo - 1) / kNPadTo * kNPadTo;
    return npad * taps * cpad;
}

extern "C" int emd_pack_weights_bf16(const float* w_host, int taps, int Cin, int Cout, int cout_major,
                                     uint16_t* hi_host, uint16_t* lo_host) {
    EMD_REQUIRE(w_host && hi_host && lo_host, EMD_E_INVALID, "emd_pack_weights_bf16: null pointer");
    EMD_REQUIRE(taps >= 1 && taps <= 9 && Cin >= 1 && Cout >= 1, EMD_E_INVALID, "emd_pack_weights_bf16: bad shape");
    const size_t cpad = (size_t)(Cin + kBK - 1) / kBK * kBK;
    const size_t npad = (size_t)(Cout + kNPadTo - 1) / kNPadTo * kNPadTo;
    const size_t ktot = (size_t)taps * cpad;
    for (size_t i = 0; i < npad * ktot; ++i) hi_host[i] = lo_host[i] = 0;
    for (int t = 0; t < taps; ++t)
        for (int c = 0; c < Cin; ++c)
            for (int n = 0; n < Cout; ++n) {
                const float w = cout_major ? w_host[((size_t)t * Cout + n) * Cin + c]
                                           : w_host[((size_t)t * Cin + c) * Cout + n];
                const uint16_t h = f32_to_bf16_rne(w);
                const uint16_t l = f32_to_bf16_rne(w - bf16_to_f32(h));
                const size_t o = (size_t)n * ktot + (size_t)t * cpad + c;
                hi_host[o] = h;
                lo_host[o] = l;
            }
    return EMD_OK;
}

// phase = 2*py + px; returns the number of taps and their 3x3 kernel coordinates, in the order the packed weights of that phase must be
// laid out (see deconv_phase)
extern "C" int emd_deconv_phase_taps(int phase, int* ky, int* kx) {
    if (phase < 0 || phase > 3 || !ky || !kx) return 0;
    const int py = phase >> 1, px = phase & 1;
    int kys[2], kxs[2], ny, nx;
    if (py) { kys[0] = 1; ny = 1; } else { kys[0] = 0; kys[1] = 2; ny = 2; }
    if (px) { kxs[0] = 1; nx = 1; } else { kxs[0] = 0; kxs[1] = 2; nx = 2; }
    int n = 0;
    for (int a = 0; a < ny; ++a)
        for (int b = 0; b < nx; ++b) { ky[n] = kys[a]; kx[n] = kxs[b]; ++n; }
    return n;
}

// ------------------------------------------------------------------------------------------------------------------------------
// Entry points, fp32 input (gemm_conv.hip).  replaces slim.conv2d / the pointwise half of slim.separable_convolution2d + bias + BN + relu6
// and the residual "+=" behind them: see gemm_conv.hip.

extern "C" int emd_conv1x1_f32(const float* x, int ldx, const uint16_t* whi, const uint16_t* wlo, const float* scale1, const float* shift1,
                               const float* scale2, const float* shift2, const float* res, int ldres, float* y, int ldy, int B, int H, int W,
                               int Cin, int Cout, int stride, int act, int precision, emd_stream_t stream) {
    const F32Args a{x, ldx, whi, wlo, scale1, shift1, scale2, shift2, res, ldres, y, ldy, B, H, W, Cin, Cout, stride, 1, act, precision};
    if (int rc = f32_checks(kConv1, a)) return rc;
    return f32_run(kConv1, a, stream);
}

// emd_conv1x1_f32 (stride 1) whose shift is a per-pixel value: y = act(fmaf(x . W, scale1, U)), U = emd_resize_bilinear_f32 of
// up [B,Hu,Wu,Cout] to [H, W], sampled in the epilogue (the resize kernel's arithmetic on the same taps: U carries its bits) and never
// written.  For a 1x1 conv over concat(resize(a), x): the interpolation weights sum to 1, so resize commutes with the conv and the affine
// -- up = scale1 * (a . W_a) + shift1 at a's resolution (graph D's residual2_d, machine_learning/denoiser.py:350-356).  No second
// affine and no residual in this mode.  (The ladder sees `up` in shift1's place: a misaligned `up` reports the scale/shift sentence.)
extern "C" int emd_conv1x1_up_f32(const float* x, int ldx, const uint16_t* whi, const uint16_t* wlo, const float* scale1, const float* up,
                                  int ldup, int Hu, int Wu, const float* scale2, const float* shift2, const float* res, int ldres, float* y,
                                  int ldy, int B, int H, int W, int Cin, int Cout, int act, int precision, emd_stream_t stream) {
    EMD_REQUIRE(!scale2 && !shift2 && !res, EMD_E_UNSUPPORTED, "emd_conv1x1_up_f32: no second affine and no residual with an upsampled shift");
    const F32Args a{x, ldx, whi, wlo, scale1, up, nullptr, nullptr, nullptr, 0, y, ldy, B, H, W, Cin, Cout, 1, 1, act, precision};
    if (int rc = f32_checks(kConv1Up, a)) return rc;
    EMD_REQUIRE(Hu >= 1 && Wu >= 1, EMD_E_INVALID, "emd_conv1x1_up_f32: bad shape");
    EMD_REQUIRE(ldup % 4 == 0 && ldup >= Cout, EMD_E_ALIGN, "emd_conv1x1_up_f32: ldup must be a multiple of 4, >= Cout");
    EMD_REQUIRE(H <= (1 << 20) && W <= (1 << 20) && B < (1 << 23), EMD_E_UNSUPPORTED, "emd_conv1x1_up_f32: H, W <= 2^20, B < 2^23");
    const UpSample u{up, ldup, Hu, Wu, (float)Hu / (float)H, (float)Wu / (float)W};
    return f32_run(kConv1Up, a, stream, &u);
}

// tf.layers.conv2d / slim.conv2d with kernel_size 3, TF SAME padding, stride 1 or 2, dilation `rate` (stride 1 only) as a 9-tap
// implicit GEMM.  Weights: emd_pack_weights_bf16(taps = 9, [ky][kx][Cin][Cout]).
extern "C" int emd_conv3x3_f32(const float* x, int ldx, const uint16_t* whi, const uint16_t* wlo, const float* scale1, const float* shift1,
                               const float* scale2, const float* shift2, const float* res, int ldres, float* y, int ldy, int B, int H, int W,
                               int Cin, int Cout, int stride, int rate, int act, int precision, emd_stream_t stream) {
    const F32Args a{x, ldx, whi, wlo, scale1, shift1, scale2, shift2, res, ldres, y, ldy, B, H, W, Cin, Cout, stride, rate, act, precision};
    if (int rc = f32_checks(kConv3, a)) return rc;
    return f32_run(kConv3, a, stream);
}

// slim.conv2d_transpose(k=3, stride=2, 'same') + bias + BN + relu6 (denoiser.py:141-148): the four phases of deconv_phase, one launch each
extern "C" int emd_deconv3x3s2_f32(const float* x, int ldx, const uint16_t* const whi[4], const uint16_t* const wlo[4], const float* scale1,
                                   const float* shift1, float* y, int ldy, int B, int H, int W, int Cin, int Cout, int act, int precision,
                                   emd_stream_t stream) {
    const F32Args a{x, ldx, whi, wlo, scale1, shift1, nullptr, nullptr, nullptr, 0, y, ldy, B, H, W, Cin, Cout, 1, 1, act, precision};
    if (int rc = f32_checks(kDeconv, a)) return rc;
    return f32_run(kDeconv, a, stream);
}

// Data gradient of the stride-2 1x1 convolution: dx[b, 2i, 2j, :] (+)= dy[b, i, j, :] * W^T, the other pixels of dx
// are not touched (the caller zero-fills dx, or passes res == dx to add into a gradient that already exists).
// whi/wlo: W packed transposed (emd_pack_weights_dev with Cin/Cout swapped and cout_major = 1).
extern "C" int emd_conv1x1_s2_bwd_data_f32(const float* dy, int ldd, const uint16_t* whi, const uint16_t* wlo, const float* scale1,
                                           const float* shift1, const float* res, int ldres, float* dx, int ldx, int B, int H, int W, int Cout,
                                           int Cin, int precision, emd_stream_t stream) {
    const F32Args a{dy, ldd, whi, wlo, scale1, shift1, nullptr, nullptr, res, ldres, dx, ldx, B, H, W, Cout, Cin, 2, 1, 0, precision};
    if (int rc = f32_checks(kConv1Bwd, a)) return rc;
    return f32_run(kConv1Bwd, a, stream);
}

// workspace of the *_stats[_fold]_f32 entries: + 3 rows: the transposed conv asks with M = 4 * B * H * W and its four phases write
// 4 * ceil(B * H * W / 128) rows of partials, up to three more than ceil(M / 128) when B * H * W is no multiple of 128 (without them the
// last phase wrote past the workspace)
extern "C" size_t emd_conv_stats_workspace_bytes(long M, int Cout) {
    if (M <= 0 || Cout <= 0) return 0;
    return (size_t)((M + 127) / 128 + 3) * 2 * Cout * sizeof(double);
}

extern "C" int emd_conv1x1_stats_f32(const float* x, int ldx, const uint16_t* whi, const uint16_t* wlo, const float* ones, const float* zeros,
                                     float* y, int ldy, int B, int H, int W, int Cin, int Cout, int stride, int precision, int images,
                                     float* mean, float* var, void* workspace, emd_stream_t stream) {
    const F32Args a{x, ldx, whi, wlo, ones, zeros, nullptr, nullptr, nullptr, 0, y, ldy, B, H, W, Cin, Cout, stride, 1, 0, precision};
    return f32_stats(kConv1Stats, a, images, mean, var, workspace, nullptr, stream);
}

extern "C" int emd_conv1x1_stats_fold_f32(const float* x, int ldx, const uint16_t* whi, const uint16_t* wlo, const float* ones,
                                          const float* zeros, float* y, int ldy, int B, int H, int W, int Cin, int Cout, int stride,
                                          int precision, int images, float* mean, float* var, void* workspace,
                                          const emd_bn_train_fold_t* fold, emd_stream_t stream) {
    EMD_REQUIRE(fold, EMD_E_INVALID, "emd_conv1x1_stats_fold_f32: null fold block");
    const F32Args a{x, ldx, whi, wlo, ones, zeros, nullptr, nullptr, nullptr, 0, y, ldy, B, H, W, Cin, Cout, stride, 1, 0, precision};
    return f32_stats(kConv1Stats, a, images, mean, var, workspace, fold, stream);
}

extern "C" int emd_conv3x3_stats_f32(const float* x, int ldx, const uint16_t* whi, const uint16_t* wlo, const float* ones, const float* zeros,
                                     float* y, int ldy, int B, int H, int W, int Cin, int Cout, int rate, int precision, int images,
                                     float* mean, float* var, void* workspace, emd_stream_t stream) {
    const F32Args a{x, ldx, whi, wlo, ones, zeros, nullptr, nullptr, nullptr, 0, y, ldy, B, H, W, Cin, Cout, 1, rate, 0, precision};
    return f32_stats(kConv3Stats, a, images, mean, var, workspace, nullptr, stream);
}

extern "C" int emd_conv3x3_stats_fold_f32(const float* x, int ldx, const uint16_t* whi, const uint16_t* wlo, const float* ones,
                                          const float* zeros, float* y, int ldy, int B, int H, int W, int Cin, int Cout, int rate,
                                          int precision, int images, float* mean, float* var, void* workspace,
                                          const emd_bn_train_fold_t* fold, emd_stream_t stream) {
    EMD_REQUIRE(fold, EMD_E_INVALID, "emd_conv3x3_stats_fold_f32: null fold block");
    const F32Args a{x, ldx, whi, wlo, ones, zeros, nullptr, nullptr, nullptr, 0, y, ldy, B, H, W, Cin, Cout, 1, rate, 0, precision};
    return f32_stats(kConv3Stats, a, images, mean, var, workspace, fold, stream);
}

// The transposed conv of a training forward pass: mean / var over all B * 2H * 2W output pixels, or per image (needs H * W % 128 == 0).
// workspace: emd_conv_stats_workspace_bytes(4 * B * H * W, Cout) bytes.
extern "C" int emd_deconv3x3s2_stats_f32(const float* x, int ldx, const uint16_t* const whi[4], const uint16_t* const wlo[4], const float* ones,
                                         const float* zeros, float* y, int ldy, int B, int H, int W, int Cin, int Cout, int precision,
                                         int images, float* mean, float* var, void* workspace, emd_stream_t stream) {
    const F32Args a{x, ldx, whi, wlo, ones, zeros, nullptr, nullptr, nullptr, 0, y, ldy, B, H, W, Cin, Cout, 1, 1, 0, precision};
    return f32_stats(kDeconvStats, a, images, mean, var, workspace, nullptr, stream);
}

extern "C" int emd_deconv3x3s2_stats_fold_f32(const float* x, int ldx, const uint16_t* const whi[4], const uint16_t* const wlo[4],
                                              const float* ones, const float* zeros, float* y, int ldy, int B, int H, int W, int Cin, int Cout,
                                              int precision, int images, float* mean, float* var, void* workspace,
                                              const emd_bn_train_fold_t* fold, emd_stream_t stream) {
    EMD_REQUIRE(fold, EMD_E_INVALID, "emd_deconv3x3s2_stats_fold_f32: null fold block");
    const F32Args a{x, ldx, whi, wlo, ones, zeros, nullptr, nullptr, nullptr, 0, y, ldy, B, H, W, Cin, Cout, 1, 1, 0, precision};
    return f32_stats(kDeconvStats, a, images, mean, var, workspace, fold, stream);
}

// ------------------------------------------------------------------------------------------------------------------------------
// Entry points, split32 input: the 3x3 and transposed convs (conv_split.hip, conv3_pipe.hip, deconv_pipe.hip)

extern "C" int emd_conv3x3_split32_f32(const void* xs, int ldx, const uint16_t* whi, const uint16_t* wlo, const float* scale1,
                                       const float* shift1, const float* scale2, const float* shift2, const float* res, int ldres, void* y,
                                       int ldy, int B, int H, int W, int Cin, int Cout, int stride, int rate, int act, int out_split,
                                       emd_stream_t stream) {
    if (int rc = split_checks(xs, ldx, whi, wlo, scale1, shift1, scale2, shift2, res, ldres, y, ldy, Cin, Cout, out_split)) return rc;
    EMD_REQUIRE(B >= 0 && H >= 1 && W >= 1, EMD_E_INVALID, "emd_conv3x3_split32_f32: bad shape");
    EMD_REQUIRE(stride == 1 || stride == 2, EMD_E_UNSUPPORTED, "emd_conv3x3_split32_f32: stride must be 1 or 2");
    EMD_REQUIRE(rate >= 1 && rate <= 31 && (rate == 1 || stride == 1), EMD_E_UNSUPPORTED,
                "emd_conv3x3_split32_f32: rate must be 1..31, and 1 when stride is 2");
    if (B == 0) return EMD_OK;
    const ConvPlan pl = conv_plan({kOpSplitConv3, B, H, W, Cin, Cout, stride, rate, 3, (res ? kRes : 0u) | (out_split ? kOutSplit : 0u), ldx, ldy});
    if (!pl.route) return fail(EMD_E_UNSUPPORTED, pl.refuse);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (pl.route == kConv3Pipe) {
        Conv3Params q{};
        q.x = static_cast<const unsigned char*>(xs); q.ldx_bytes = (long)ldx * 4; q.Whi = whi; q.Wlo = wlo; q.y = static_cast<float*>(y);
        q.scale1 = scale1; q.shift1 = shift1; q.scale2 = scale2; q.shift2 = shift2;
        q.H = H; q.W = W; q.Cin = ceil_to(Cin, 32); q.Cpad = ceil_to(Cin, kBK); q.Ktot = 9 * q.Cpad; q.N = Cout; q.ldy = ldy; q.act = act;
        q.tpw = pl.tpw; q.n_ntiles = pl.n_ntiles;
        return conv3_pipe_launch(pl, q, st);
    }
    const ConvGeom g = same_conv(B, H, W, 3, stride, rate);
    const SplitConvParams c = split_conv_params(
        split_params(xs, ldx, whi, wlo, scale1, shift1, scale2, shift2, res, ldres, y, ldy, g.M, Cin, Cout, act, pl), g, out_split);
    return conv_split_launch(pl, c, st);
}

extern "C" int emd_deconv3x3s2_split32_f32(const void* xs, int ldx, const uint16_t* const whi[4], const uint16_t* const wlo[4],
                                           const float* scale1, const float* shift1, void* y, int ldy, int B, int H, int W, int Cin, int Cout,
                                           int act, int out_split, emd_stream_t stream) {
    if (int rc = split_deconv_checks("emd_deconv3x3s2_split32_f32", xs, ldx, whi, wlo, scale1, shift1, y, ldy, B, H, W, Cin, Cout, out_split)) return rc;
    if (B == 0) return EMD_OK;
    const ConvPlan pl = conv_plan({kOpSplitDeconv, B, H, W, Cin, Cout, 1, 1, 3, out_split ? kOutSplit : 0u, ldx, ldy});
    if (!pl.route) return fail(EMD_E_UNSUPPORTED, pl.refuse);
    for (int ph = 0; ph < 4; ++ph) {
        const ConvGeom g = deconv_phase(B, H, W, ph);
        const SplitConvParams c = split_conv_params(
            split_params(xs, ldx, whi[ph], wlo[ph], scale1, shift1, nullptr, nullptr, nullptr, 0, y, ldy, g.M, Cin, Cout, act, pl), g, out_split);
        if (int rc = conv_split_launch(pl, c, static_cast<hipStream_t>(stream))) return rc;
    }
    return EMD_OK;
}

// The same transposed convolution as ONE launch.  gemm_split_conv_kernel<BN, true> and its deconv4_* forms: each workgroup computes the
// four output phases of its 256 input pixels back to back, so the input is fetched from HBM once instead of once per phase launch (the 9
// taps' DMA re-reads hit L2); same products in the same order as the four-launch form: bit-identical results.  deconv_pipe.hip where it
// covers the layer (see deconv_patch_route).
extern "C" int emd_deconv3x3s2_fused_split32_f32(const void* xs, int ldx, const uint16_t* const whi[4], const uint16_t* const wlo[4],
                                                 const float* scale1, const float* shift1, void* y, int ldy, int B, int H, int W, int Cin,
                                                 int Cout, int act, int out_split, emd_stream_t stream) {
    if (int rc = split_deconv_checks("emd_deconv3x3s2_fused_split32_f32", xs, ldx, whi, wlo, scale1, shift1, y, ldy, B, H, W, Cin, Cout, out_split))
        return rc;
    if (B == 0) return EMD_OK;
    ConvAsk ask{kOpSplitDeconvFused, B, H, W, Cin, Cout, 1, 1, 3, out_split ? kOutSplit : 0u, ldx, ldy};
    ConvPlan pl = conv_plan(ask);
    if (!pl.route) return fail(EMD_E_UNSUPPORTED, pl.refuse);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (pl.route == kDeconvPipe) {
        DeconvPipeParams q{};
        q.ldx_bytes = (long)ldx * 4;
        for (int ph = 0; ph < 4; ++ph) { q.Whi[ph] = whi[ph]; q.Wlo[ph] = wlo[ph]; }
        q.scale1 = scale1; q.shift1 = shift1;
        q.H = H; q.W = W; q.Cin = Cin; q.Cpad = ceil_to(Cin, kBK); q.N = Cout; q.ldy = ldy; q.act = act;
        const long in_img = (long)H * W * q.ldx_bytes, out_img = 4L * H * W * ldy * (long)sizeof(float);
        for (int b0 = 0; b0 < B; b0 += 65535) {   // a slice of the batch has its own plan (tiles per workgroup)
            if (b0) { ask.B = B - b0; pl = conv_plan(ask); }
            q.x = static_cast<const unsigned char*>(xs) + (long)b0 * in_img;
            q.y = reinterpret_cast<float*>(static_cast<unsigned char*>(y) + (long)b0 * out_img);
            q.tpw = pl.tpw; q.n_ntiles = pl.n_ntiles; q.ablate = pl.ablate;
            if (int rc = deconv_pipe_launch(pl, q, st)) return rc;
        }
        return EMD_OK;
    }
    ConvGeom g = deconv_phase(B, H, W, 3);
    g.ntaps = 4;   // the tap stride of the weights; the kernel uses the per-phase counts
    g.py = g.px = 0;
    SplitConvParams c = split_conv_params(
        split_params(xs, ldx, whi[0], wlo[0], scale1, shift1, nullptr, nullptr, nullptr, 0, y, ldy, g.M, Cin, Cout, act, pl), g, out_split);
    for (int ph = 0; ph < 4; ++ph) {
        g = deconv_phase(B, H, W, ph);
        c.Whi4[ph] = whi[ph]; c.Wlo4[ph] = wlo[ph]; c.ntaps4[ph] = g.ntaps; c.dyp4[ph] = g.dyp; c.dxp4[ph] = g.dxp;
    }
    return conv_split_launch(pl, c, st);
}
