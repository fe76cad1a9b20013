// The 1-D line transform that fft.hip (the harvester's spectrum) and exitwave.hip (the focal-series reconstruction) share, one
// definition of each: the LDS swizzle, the complex helpers, the twiddle table's entry and fft_line.
//
// The transform is a Stockham autosort of radix-4 passes and a last radix-2 pass where log2 S is odd, on ONE line of S complex
// doubles in LDS (64 KiB at 4096): a pass reads all its inputs into registers, a barrier, and writes them back.  Element i lives at
// swz(i) = i ^ ((i >> 3) & 3): every read of consecutive elements by consecutive lanes stays conflict-free in the 16-lane groups of
// a 16-byte LDS read, and the first pass's stores (4 j + r over 8 consecutive lanes: two 16-byte slots of eight without the swizzle,
// 4-way) land on eight distinct slots; the second pass's stores stay 2-way, which a 16-byte store's issue cost covers.
//
// The inverse transform is by conjugation: conjugate on load, fft_line, conjugate and scale by 1 / S (exact: S is a power of two)
// on store.
#pragma once

#include <hip/hip_runtime.h>

namespace {

typedef double2 cplx;

__device__ __forceinline__ int swz(int i) { return i ^ ((i >> 3) & 3); }
__device__ __forceinline__ cplx cadd(cplx a, cplx b) { return make_double2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ cplx csub(cplx a, cplx b) { return make_double2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ cplx cmul(cplx a, cplx w) { return make_double2(a.x * w.x - a.y * w.y, a.x * w.y + a.y * w.x); }

// tw[k] = exp(-2 pi i k / S), k = blockIdx.x * 256 + threadIdx.x < S: the body of each file's twiddle kernel
__device__ __forceinline__ void twiddle_entry(cplx* __restrict__ tw, int S) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k < S) {
        double s, c;
        sincospi(-2.0 * (double)k / (double)S, &s, &c);   // 2 k / S is exact
        tw[k] = make_double2(c, s);
    }
}

// Forward, unnormalised transform of line[swz(0..S-1)] in place, natural order in and out, by the 256 threads of the workgroup.
// Begins and ends with a barrier.  tw: exp(-2 pi i k / S).
__device__ void fft_line(cplx* line, int S, const cplx* __restrict__ tw) {
    const int tid = threadIdx.x;
    const int Q = S >> 2;
    int Ns = 1;
    for (; Ns * 4 <= S; Ns <<= 2) {
        const int tstep = Q / Ns;   // exp(-2 pi i k / (4 Ns)) = tw[k * tstep]
        cplx v[4][4];
        __syncthreads();
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int j = tid + 256 * u;
            if (j < Q) {
                const int k = j & (Ns - 1);
                v[u][0] = line[swz(j)];
                v[u][1] = cmul(line[swz(j + Q)], tw[k * tstep]);
                v[u][2] = cmul(line[swz(j + 2 * Q)], tw[2 * k * tstep]);
                v[u][3] = cmul(line[swz(j + 3 * Q)], tw[3 * k * tstep]);
            }
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int j = tid + 256 * u;
            if (j < Q) {
                const int k = j & (Ns - 1);
                const int o = ((j - k) << 2) + k;
                const cplx t0 = cadd(v[u][0], v[u][2]), t1 = csub(v[u][0], v[u][2]), t2 = cadd(v[u][1], v[u][3]);
                const cplx d = csub(v[u][1], v[u][3]);
                const cplx t3 = make_double2(d.y, -d.x);   // -i d
                line[swz(o)] = cadd(t0, t2);
                line[swz(o + Ns)] = cadd(t1, t3);
                line[swz(o + 2 * Ns)] = csub(t0, t2);
                line[swz(o + 3 * Ns)] = csub(t1, t3);
            }
        }
    }
    if (Ns < S) {   // log2 S odd: the last pass is radix-2, Ns = S / 2; a thread rewrites the two elements it read
        __syncthreads();
        for (int j = tid; j < Ns; j += 256) {
            const cplx a = line[swz(j)], b = cmul(line[swz(j + Ns)], tw[j]);
            line[swz(j)] = cadd(a, b);
            line[swz(j + Ns)] = csub(a, b);
        }
    }
    __syncthreads();
}

}  // namespace
