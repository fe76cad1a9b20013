// The one copy of the tap arithmetic of emdenoise.resample: cv2.resize for one-channel float32, restated from the
// rules in include/emdenoise.h.  __host__ __device__: resize_kernel (resample.hip) forms every description in registers from these
// functions, and emd_resize_taps, the tests' window, calls the same ones on the host.  Everything is IEEE double, every operation
// rounds on its own (no fused multiply-add), except where a rounding to float32 is written out: those are cv2's own and decide
// which pixels are read.  Only +, -, *, /, floor, ceil and conversions: host and device give the same bits.
#pragma once

#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>

namespace emd {

enum ResizeInterp { kResizeNearest = 0, kResizeLinear = 1, kResizeCubic = 2, kResizeArea = 3 };   // cv2's codes
enum ResizeForm {
    kFormNearest = 0,
    kFormLinear = 1,
    kFormCubic = 2,
    kFormAreaRun = 3,      // true area: fractional coverage, one run with a first, an interior and a last weight
    kFormAreaBlock = 4,    // true area at whole ratios on both axes: the mean of the block
    kFormAreaLinear = 5,   // an axis enlarges: cv2's emulated area, the LINEAR form with area coordinates on both axes
};

// One axis of one image: what every sample of the axis shares.
struct ResizeAxis {
    int form, n_in, n_out;
    int block;           // kFormAreaBlock: pixels of a block along this axis
    double inv, scale;   // inv = (double)n_out / n_in, scale = 1.0 / inv (cv2's order; not n_in / n_out)
};

// One output sample along one axis.  Tap k (0 <= k < count) reads source index min(max(first + k, 0), n_in - 1) -- CUBIC reaches -1 and
// n_in, LINEAR n_in: the border replicates -- with weight
//     k == 0 ? w0 : k == count - 1 ? wl : k == 1 ? w1 : w2
// which covers the fixed forms (1, 2 and 4 taps) and a run of any length whose interior taps share one weight (w1 == w2).
struct ResizeTap {
    int first, count;
    double w0, w1, w2, wl;
};

__host__ __device__ __forceinline__ double resize_tap_weight(const ResizeTap& t, int k) {
    const double w0 = t.w0, w1 = t.w1, w2 = t.w2, wl = t.wl;   // read all four, then select among values (never among addresses)
    return k == 0 ? w0 : (k == t.count - 1 ? wl : (k == 1 ? w1 : w2));
}

__host__ __device__ __forceinline__ int resize_tap_index(const ResizeTap& t, int k, int n_in) {
    const int i = t.first + k;
    return i < 0 ? 0 : (i > n_in - 1 ? n_in - 1 : i);
}

// The two axes of an image: the area rule looks at both.
__host__ __device__ __forceinline__ void resize_axes(int interpolation, int nx_in, int nx_out, int ny_in, int ny_out, ResizeAxis& ax, ResizeAxis& ay) {
#pragma clang fp contract(off)
    ax.n_in = nx_in, ax.n_out = nx_out, ay.n_in = ny_in, ay.n_out = ny_out;
    ax.inv = (double)nx_out / (double)nx_in, ay.inv = (double)ny_out / (double)ny_in;
    ax.scale = 1.0 / ax.inv, ay.scale = 1.0 / ay.inv;
    ax.block = ay.block = 0;
    int form = interpolation == kResizeNearest ? kFormNearest : (interpolation == kResizeCubic ? kFormCubic : kFormLinear);
    if (interpolation == kResizeArea) {
        if (ax.scale >= 1.0 && ay.scale >= 1.0) {
            const int ix = (int)ax.scale, iy = (int)ay.scale;
            const double ex = ax.scale - (double)ix, ey = ay.scale - (double)iy;
            if ((ex < 0.0 ? -ex : ex) < DBL_EPSILON && (ey < 0.0 ? -ey : ey) < DBL_EPSILON) {
                form = kFormAreaBlock;
                ax.block = ix, ay.block = iy;
            } else {
                form = kFormAreaRun;
            }
        } else {
            form = kFormAreaLinear;
        }
    }
    ax.form = ay.form = form;
}

// LINEAR's two clamps and its pair of weights
__host__ __device__ __forceinline__ void resize_linear_pair(int s, float f, int n_in, ResizeTap& t) {
    if (s < 0) s = 0, f = 0.f;
    if (s >= n_in - 1) s = n_in - 1, f = 0.f;
    t.first = s, t.count = 2;
    t.w0 = 1.0 - (double)f;
    t.wl = (double)f;
}

__host__ __device__ __forceinline__ ResizeTap resize_tap(const ResizeAxis& a, int d) {
#pragma clang fp contract(off)
    ResizeTap t;
    t.first = 0, t.count = 1;
    t.w0 = 1.0, t.w1 = t.w2 = t.wl = 0.0;
    const int n = a.n_in;
    const double scale = a.scale;
    if (a.form == kFormNearest) {
        const int s = (int)floor((double)d * scale);
        t.first = s < n - 1 ? s : n - 1;
    } else if (a.form == kFormLinear || a.form == kFormCubic) {
        float f = (float)(((double)d + 0.5) * scale - 0.5);   // cv2 rounds the coordinate to float32 before the floor
        const int s = (int)floor((double)f);
        f = (float)((double)f - (double)s);
        if (a.form == kFormLinear) {
            resize_linear_pair(s, f, n, t);
        } else {
            const double A = -0.75, x = (double)f, x1 = x + 1.0, y = 1.0 - x;
            t.first = s - 1, t.count = 4;
            t.w0 = ((A * x1 - 5.0 * A) * x1 + 8.0 * A) * x1 - 4.0 * A;
            t.w1 = ((A + 2.0) * x - (A + 3.0)) * x * x + 1.0;
            t.w2 = ((A + 2.0) * y - (A + 3.0)) * y * y + 1.0;
            t.wl = 1.0 - t.w0 - t.w1 - t.w2;
        }
    } else if (a.form == kFormAreaLinear) {
        const int s = (int)floor((double)d * scale);
        float f = (float)((double)(d + 1) - (double)(s + 1) * a.inv);
        f = f <= 0.f ? 0.f : (float)((double)f - floor((double)f));
        resize_linear_pair(s, f, n, t);
    } else if (a.form == kFormAreaBlock) {
        t.first = d * a.block, t.count = a.block;
        t.w0 = t.w1 = t.w2 = t.wl = 1.0;   // the sum; resize divides it by the block's pixel count
    } else if (a.form == kFormAreaRun) {
        const double f1 = (double)d * scale, f2 = f1 + scale;
        const double left = (double)n - f1, cell = scale < left ? scale : left;
        int s1 = (int)ceil(f1), s2 = (int)floor(f2);
        s2 = s2 < n - 1 ? s2 : n - 1;
        s1 = s1 < s2 ? s1 : s2;
        const bool head = (double)s1 - f1 > 1e-3, tail = f2 - (double)s2 > 1e-3;
        const double over = f2 - (double)s2, over1 = over < 1.0 ? over : 1.0;
        const double wh = (double)(float)(((double)s1 - f1) / cell), wm = (double)(float)(1.0 / cell);
        const double wt = (double)(float)((over1 < cell ? over1 : cell) / cell);
        const int mid = s2 - s1;
        t.first = s1 - (head ? 1 : 0);
        t.count = (head ? 1 : 0) + mid + (tail ? 1 : 0);
        t.w0 = head ? wh : (mid > 0 ? wm : wt);
        t.wl = tail ? wt : (mid > 0 ? wm : wh);
        t.w1 = t.w2 = wm;
    }
    if (a.form == kFormAreaRun || a.form == kFormAreaBlock) {
        // a run lies inside the axis by the rule; whatever the arithmetic gave, nothing is read outside it
        if (t.first < 0) t.first = 0;
        if (t.first > n - 1) t.first = n - 1;
        if (t.count < 0) t.count = 0;
        if (t.count > n - t.first) t.count = n - t.first;
    }
    return t;
}

}  // namespace emd
