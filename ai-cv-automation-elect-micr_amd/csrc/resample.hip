// cv2.resize on the device for one-channel float32: INTER_NEAREST, INTER_LINEAR, INTER_CUBIC and INTER_AREA, restated
// from the rules in include/emdenoise.h -- the reference's load_image(addr, resizeSize), its random crops resized to the network's
// side and EWREC.resize_stack.
//
//   emd_resize_f32   one launch: a workgroup owns 16 x 64 outputs of one image; a lane owns one output column and four output rows.
//                    Their tap descriptions (resize_taps.hpp) are formed once, in registers: the column's by its lane, a wave's
//                    four rows' by four of its lanes and broadcast into scalar registers; the source rows and columns the tile's taps
//                    cover pass through LDS in coalesced segments of up to 20 rows x 264 columns, and every lane adds
//                    beta * (sum of alpha * x) from LDS into double accumulators, rows ascending.  Both directions are segmented, so
//                    any ratio fits (32768 -> 1).  With boxes, image b's source is its rectangle, clamped into the image, and the sizes
//                    and the area rule are taken per image.
//   emd_resize_taps  HOST: the same descriptions as a table.
//
// No atomics, no workspace, a fixed summation order: bitwise reproducible, and an image's result does not depend on the batch.
#include "emd_common.hpp"
#include "resize_taps.hpp"

#pragma clang fp contract(off)   // every operation rounds on its own, as in the host restatement

namespace {

constexpr int kMaxExtent = 32768;   // H, W
constexpr int kMaxOut = 8192;       // h, w
constexpr int kRT = 16;             // output rows of a tile (a wave: 4)
constexpr int kRW = 4;              // rows of a lane: resize_kernel spells the four out
constexpr int kRC = 64;             // output columns of a tile = lanes of a wave
// An LDS segment: 20 source rows x 264 columns (21 KiB, seven workgroups per CU).  A tile's 16 output rows with CUBIC's three extra
// taps cover 19 source rows up to ratio 1, and 64 output columns 259 source columns up to ratio 4: one segment each way.
constexpr int kSegR = 20;
constexpr int kSegC = 264;

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// Lane `src`'s copy of a value, in every lane (src is a constant: the value lands in scalar registers).
__device__ __forceinline__ int from_lane(int v, int src) { return __builtin_amdgcn_readlane(v, src); }
__device__ __forceinline__ double from_lane(double v, int src) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), src), __builtin_amdgcn_readlane(__double2loint(v), src));
}
__device__ __forceinline__ emd::ResizeTap from_lane(const emd::ResizeTap& t, int src) {
    emd::ResizeTap r;
    r.first = from_lane(t.first, src), r.count = from_lane(t.count, src);
    r.w0 = from_lane(t.w0, src), r.w1 = from_lane(t.w1, src), r.w2 = from_lane(t.w2, src), r.wl = from_lane(t.wl, src);
    return r;
}

// The taps k of `t` whose source index lies in [lo, hi), a segment of the axis of n samples: [ka, kb).  The clamped index ascends
// with k, so they are one range; for every k in it, resize_tap_index(t, k, n) - lo is in 0 .. hi - lo - 1 whatever `t` holds.
__device__ __forceinline__ void taps_in(const emd::ResizeTap& t, int lo, int hi, int n, int& ka, int& kb) {
    ka = lo <= 0 ? 0 : max(0, lo - t.first);
    kb = hi >= n ? t.count : min(t.count, hi - t.first);
}

// One output row's share of a segment: acc += beta_i * (sum over this lane's column taps [ja, jb) of alpha_j * x), for the row taps i
// whose source row lies in the segment's rows [sr, sr + hr); the segment's first column is sc.
__device__ __forceinline__ void add_row(const float* seg, const emd::ResizeTap& tr, const emd::ResizeTap& tc, int sr, int hr, int sc, int ja,
                                        int jb, int bh, int bw, double& acc) {
    int ia, ib;
    taps_in(tr, sr, sr + hr, bh, ia, ib);
    for (int i = ia; i < ib; ++i) {
        const float* srow = seg + (emd::resize_tap_index(tr, i, bh) - sr) * kSegC;
        double s = 0.0;
        for (int j = ja; j < jb; ++j) s += emd::resize_tap_weight(tc, j) * (double)srow[emd::resize_tap_index(tc, j, bw) - sc];
        acc += emd::resize_tap_weight(tr, i) * s;
    }
}

// A lane's column taps in the fixed forms (at most four), as they stand in one column segment: bit k of `mask` says tap k reads
// column at[k] of the segment with weight w[k].
struct FixedCols {
    int at0, at1, at2, at3;
    unsigned mask;
    double w0, w1, w2, w3;
};

// add_row for the fixed forms.  The same products in the same order as add_row.
__device__ __forceinline__ void add_row_fixed(const float* seg, const emd::ResizeTap& tr, const FixedCols& fc, int sr, int hr, int bh,
                                              double& acc) {
    int ia, ib;
    taps_in(tr, sr, sr + hr, bh, ia, ib);
    for (int i = ia; i < ib; ++i) {
        const float* srow = seg + (emd::resize_tap_index(tr, i, bh) - sr) * kSegC;
        double s = 0.0;
        if (fc.mask & 1u) s += fc.w0 * (double)srow[fc.at0];
        if (fc.mask & 2u) s += fc.w1 * (double)srow[fc.at1];
        if (fc.mask & 4u) s += fc.w2 * (double)srow[fc.at2];
        if (fc.mask & 8u) s += fc.w3 * (double)srow[fc.at3];
        acc += emd::resize_tap_weight(tr, i) * s;
    }
}

// grid (tiles, B), 256 threads.  x: image b at x + b * xstride, rows row_stride apart, H x W; boxes NULL or [B][4] = (x0, y0, bw, bh).
// FIXED: every image is in a fixed form (at most four taps a sample: the host knows), and add_row_fixed is the inner loop; otherwise
// add_row, which serves every form.  Kept on a measurement (tools/resample_bench.py).
template <bool FIXED>
__global__ __launch_bounds__(256) void resize_kernel(const float* __restrict__ x, long xstride, int row_stride, int H, int W,
                                                     const int* __restrict__ boxes, float* __restrict__ y, int h, int w, int interpolation,
                                                     int tiles_x) {
    __shared__ float seg[kSegR * kSegC];
    __shared__ int range[2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r0 = (blockIdx.x / tiles_x) * kRT, c0 = (blockIdx.x % tiles_x) * kRC;
    // the source rectangle, clamped into the image whatever the box holds: no address leaves the image
    int bx = 0, by = 0, bw = W, bh = H;
    if (boxes) {
        const int* bp = boxes + 4 * (long)blockIdx.y;
        bx = clampi(bp[0], 0, W - 1);
        by = clampi(bp[1], 0, H - 1);
        bw = clampi(bp[2], 1, W - bx);
        bh = clampi(bp[3], 1, H - by);
    }
    const float* xb = x + (long)blockIdx.y * xstride + (long)by * row_stride + bx;
    emd::ResizeAxis ax, ay;
    emd::resize_axes(interpolation, bw, w, bh, h, ax, ay);
    // this thread's outputs: column c0 + lane, rows r0 + wave * kRW + 0 .. 3
    const int oc = c0 + lane, or0 = r0 + wave * kRW;
    emd::ResizeTap tc = emd::resize_tap(ax, min(oc, w - 1));
    // a wave's four rows are the same in all its lanes: lane q forms row q's description, and every lane takes the four from there
    const emd::ResizeTap tq = emd::resize_tap(ay, min(or0 + (lane & 3), h - 1));
    emd::ResizeTap ta = from_lane(tq, 0), tb = from_lane(tq, 1), tg = from_lane(tq, 2), td = from_lane(tq, 3);
    // the source rows and columns the tile's taps cover: the first tap of its first sample to the last tap of its last sample (both
    // ascend with the output index), from the threads that own those samples
    const int rl = min(r0 + kRT, h) - 1, cl = min(c0 + kRC, w) - 1;
    const int cb = __shfl(emd::resize_tap_index(tc, 0, bw), 0), ce = __shfl(emd::resize_tap_index(tc, tc.count - 1, bw), cl - c0) + 1;
    if (lane == 0) {
        if (wave == 0) range[0] = emd::resize_tap_index(ta, 0, bh);
        if (wave == (rl - r0) / kRW) {
            const int q = (rl - r0) % kRW;
            const int la = emd::resize_tap_index(ta, ta.count - 1, bh), lb = emd::resize_tap_index(tb, tb.count - 1, bh);
            const int lg = emd::resize_tap_index(tg, tg.count - 1, bh), ld = emd::resize_tap_index(td, td.count - 1, bh);
            range[1] = (q == 0 ? la : (q == 1 ? lb : (q == 2 ? lg : ld))) + 1;
        }
    }
    __syncthreads();
    const int rb = range[0], re = range[1];
    if (oc >= w) tc.count = 0;
    if (or0 >= h) ta.count = 0;
    if (or0 + 1 >= h) tb.count = 0;
    if (or0 + 2 >= h) tg.count = 0;
    if (or0 + 3 >= h) td.count = 0;
    double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0, acc3 = 0.0;
    FixedCols fc;
    fc.w0 = emd::resize_tap_weight(tc, 0), fc.w1 = emd::resize_tap_weight(tc, 1);
    fc.w2 = emd::resize_tap_weight(tc, 2), fc.w3 = emd::resize_tap_weight(tc, 3);
    for (int sc = cb; sc < ce; sc += kSegC) {
        const int wc = min(kSegC, ce - sc);
        int ja, jb;
        taps_in(tc, sc, sc + wc, bw, ja, jb);   // this lane's column taps inside the segment
        fc.at0 = emd::resize_tap_index(tc, 0, bw) - sc, fc.at1 = emd::resize_tap_index(tc, 1, bw) - sc;
        fc.at2 = emd::resize_tap_index(tc, 2, bw) - sc, fc.at3 = emd::resize_tap_index(tc, 3, bw) - sc;
        fc.mask = (ja <= 0 && 0 < jb ? 1u : 0u) | (ja <= 1 && 1 < jb ? 2u : 0u) | (ja <= 2 && 2 < jb ? 4u : 0u) | (ja <= 3 && 3 < jb ? 8u : 0u);
        for (int sr = rb; sr < re; sr += kSegR) {
            const int hr = min(kSegR, re - sr);
            __syncthreads();   // the previous segment may still be read
            for (int r = wave; r < hr; r += 4) {
                const float* row = xb + (long)(sr + r) * row_stride + sc;
                for (int c = lane; c < wc; c += 64) seg[r * kSegC + c] = row[c];
            }
            __syncthreads();
            if (!FIXED) {
                add_row(seg, ta, tc, sr, hr, sc, ja, jb, bh, bw, acc0);
                add_row(seg, tb, tc, sr, hr, sc, ja, jb, bh, bw, acc1);
                add_row(seg, tg, tc, sr, hr, sc, ja, jb, bh, bw, acc2);
                add_row(seg, td, tc, sr, hr, sc, ja, jb, bh, bw, acc3);
            } else {
                add_row_fixed(seg, ta, fc, sr, hr, bh, acc0);
                add_row_fixed(seg, tb, fc, sr, hr, bh, acc1);
                add_row_fixed(seg, tg, fc, sr, hr, bh, acc2);
                add_row_fixed(seg, td, fc, sr, hr, bh, acc3);
            }
        }
    }
    if (oc < w) {
        float* yo = y + ((long)blockIdx.y * h + or0) * w + oc;
        const bool block = ax.form == emd::kFormAreaBlock;
        const double count = (double)ay.block * (double)ax.block;
        if (or0 < h) yo[0] = (float)(block ? acc0 / count : acc0);
        if (or0 + 1 < h) yo[w] = (float)(block ? acc1 / count : acc1);
        if (or0 + 2 < h) yo[2L * w] = (float)(block ? acc2 / count : acc2);
        if (or0 + 3 < h) yo[3L * w] = (float)(block ? acc3 / count : acc3);
    }
}

bool interpolation_ok(int i) { return i >= emd::kResizeNearest && i <= emd::kResizeArea; }

}  // namespace

extern "C" int emd_resize_taps(int interpolation, int n_in, int n_out, int other_in, int other_out, int* first, int* count, double* weights,
                               int* block) {
    EMD_REQUIRE(interpolation_ok(interpolation), EMD_E_INVALID, "emd_resize_taps: interpolation must be 0 (nearest), 1 (linear), 2 (cubic) or 3 (area)");
    if (n_in < 1 || n_in > kMaxExtent || n_out < 1 || n_out > kMaxOut || other_in < 1 || other_in > kMaxExtent || other_out < 1 ||
        other_out > kMaxOut) {
        emd::set_error("emd_resize_taps: 1 <= n_in <= 32768 and 1 <= n_out <= 8192 on both axes (got %d -> %d and %d -> %d)", n_in, n_out,
                       other_in, other_out);
        return EMD_E_INVALID;
    }
    EMD_REQUIRE(first && count && weights && block, EMD_E_INVALID, "emd_resize_taps: null pointer");
    emd::ResizeAxis a, other;
    emd::resize_axes(interpolation, n_in, n_out, other_in, other_out, a, other);
    *block = a.block;
    for (int d = 0; d < n_out; ++d) {
        const emd::ResizeTap t = emd::resize_tap(a, d);
        first[d] = t.first;
        count[d] = t.count;
        weights[4 * d] = t.w0, weights[4 * d + 1] = t.w1, weights[4 * d + 2] = t.w2, weights[4 * d + 3] = t.wl;
    }
    return EMD_OK;
}

extern "C" int emd_resize_f32(const float* x, long image_stride, int row_stride, int B, int H, int W, const int* boxes_dev, float* y, int h,
                              int w, int interpolation, emd_stream_t stream) {
    EMD_REQUIRE(B >= 0 && B <= 65535, EMD_E_INVALID, "emd_resize_f32: the batch must be 0..65535");
    EMD_REQUIRE(H >= 1 && H <= kMaxExtent && W >= 1 && W <= kMaxExtent && h >= 1 && h <= kMaxOut && w >= 1 && w <= kMaxOut, EMD_E_INVALID,
                "emd_resize_f32: 1 <= H, W <= 32768 and 1 <= h, w <= 8192");
    EMD_REQUIRE(interpolation_ok(interpolation), EMD_E_INVALID, "emd_resize_f32: interpolation must be 0 (nearest), 1 (linear), 2 (cubic) or 3 (area)");
    EMD_REQUIRE(row_stride >= W && image_stride >= 0, EMD_E_INVALID, "emd_resize_f32: row_stride must be >= W, image_stride >= 0");
    if (B == 0) return EMD_OK;
    EMD_REQUIRE(x && y, EMD_E_INVALID, "emd_resize_f32: null pointer");
    const size_t nx = ((size_t)(B - 1) * (size_t)image_stride + (size_t)(H - 1) * row_stride + W) * sizeof(float);
    const size_t ny = (size_t)B * h * w * sizeof(float);
    EMD_REQUIRE(!emd::overlap(x, nx, y, ny), EMD_E_INVALID, "emd_resize_f32: y may not overlap x");
    EMD_REQUIRE(!boxes_dev || (!emd::overlap(boxes_dev, (size_t)B * 4 * sizeof(int), y, ny)), EMD_E_INVALID,
                "emd_resize_f32: y may not overlap the boxes");
    const int tiles_x = (w + kRC - 1) / kRC;
    const dim3 grid((unsigned)(tiles_x * ((h + kRT - 1) / kRT)), (unsigned)B);
    // the fixed forms: everything but true area, whose decision is per image with boxes (then the loop that serves every form runs)
    bool fixed = interpolation != emd::kResizeArea;
    if (!fixed && !boxes_dev) {
        emd::ResizeAxis ax, ay;
        emd::resize_axes(interpolation, W, w, H, h, ax, ay);
        fixed = ax.form == emd::kFormAreaLinear;
    }
    hipLaunchKernelGGL(fixed && !emd::g_knobs.resize_generic ? resize_kernel<true> : resize_kernel<false>, grid, dim3(256), 0,
                       static_cast<hipStream_t>(stream), x, image_stride, row_stride, H, W, boxes_dev, y, h, w, interpolation, tiles_x);
    return emd::check_launch("resize_kernel");
}
