// The exact median of one image's values by a four-pass radix selection on integer histograms, shared by
// wavelet.hip (the non-zero |dd_1| of the noise estimate) and harvest.hip (the signed pixels of the statistics table).  One
// definition of the layout, the keys, the counting step and the resolve.
//
// A value becomes a 32-bit key that orders as an unsigned integer.  Pass q = 0..3 counts keys by their bits [31 - 8q .. 24 - 8q]:
// pass 0 all of them in one histogram, pass q > 0 for either middle rank those whose higher bits equal that rank's prefix.
// select_resolve then finds the bin that holds each rank, which extends the prefix by 8 bits; after pass 3 the prefixes are the
// two middle keys.  All counts are integers: the atomics cannot change a result, so it is the same bits on every run.
//
// A caller chooses three things: the key (and which values it leaves out), hence the count, which is whatever pass 0 counted; and
// where the resolve runs (at the head of the next pass's workgroups, or in a launch of its own).
#pragma once

#include "emd_common.hpp"

namespace {

constexpr int kSelHistWords = 2 * 256;   // hist:  [B][4 passes][2 ranks][256], zero before pass 0
constexpr int kStateWords = 4;           // state: [B][4 passes][kStateWords] = (prefix 0, prefix 1, rank 0, rank 1) that pass q
                                         // works with, the ranks inside the prefixes' bins; slot 0 is never used
__host__ __device__ inline long select_hist_at(long b, int q) { return (b * 4 + q) * kSelHistWords; }
__host__ __device__ inline long select_state_at(long b, int q) { return (b * 4 + q) * kStateWords; }
// what the two slices add to a workspace of 256-byte aligned parts
inline size_t select_hist_bytes(int B) { return emd::round256((size_t)B * 4 * kSelHistWords * sizeof(unsigned)); }
inline size_t select_state_bytes(int B) { return emd::round256((size_t)B * 4 * kStateWords * sizeof(unsigned)); }

// |v|: the bit patterns of non-negative floats order as unsigned integers; 0 for either zero.
__device__ __forceinline__ unsigned magnitude_key(float v) { return __float_as_uint(v) & 0x7fffffffu; }

// The order-preserving key of a signed float: negative -> all bits flipped, else the sign bit set.  -0 is +0 first (they are equal).
__device__ __forceinline__ unsigned signed_key(float v) {
    unsigned u = __float_as_uint(v);
    if (u == 0x80000000u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float signed_key_value(unsigned key) {
    return __uint_as_float((key & 0x80000000u) ? (key & 0x7fffffffu) : ~key);
}

// One key into a workgroup's LDS histograms: pass 0 (h[0] alone, for both ranks), and pass q = 1..3.
__device__ __forceinline__ void select_count_first(unsigned (*h)[256], unsigned key) { atomicAdd(&h[0][key >> 24], 1u); }
__device__ __forceinline__ void select_count(unsigned (*h)[256], unsigned key, int q, unsigned prefix0, unsigned prefix1) {
    const int shift = 24 - 8 * q;
    const unsigned bin = (key >> shift) & 255u, high = key >> (shift + 8);
    if (high == prefix0) atomicAdd(&h[0][bin], 1u);
    if (high == prefix1) atomicAdd(&h[1][bin], 1u);
}

// The workgroup's LDS histograms (RANKS of them) into the pass's slice hb, after a barrier behind the last count; 256 threads.
template <int RANKS>
__device__ __forceinline__ void select_flush(const unsigned (*h)[256], unsigned* __restrict__ hb) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int r = 0; r < RANKS; ++r) {
        if (h[r][tid]) atomicAdd(&hb[r * 256 + tid], h[r][tid]);
    }
}

// From the histograms of pass q and the state that pass worked with (in; not read when q = 0): the state of pass q + 1 into out,
// kStateWords words of LDS (after pass 3: the prefixes are the two middle keys).  At pass 0 the middle ranks of n counted keys are
// (n - 1) / 2 and n / 2, n being the histogram's total.  When nothing was counted no bin matches at any pass: every word of out
// stays 0.  Every thread of the 256 calls it; out is valid for all of them after the call.
__device__ void select_resolve(const unsigned* __restrict__ hist, const unsigned* __restrict__ in, int q, unsigned (*sc)[256],
                               unsigned* out) {
    const int tid = threadIdx.x;
    const unsigned n0 = hist[tid], n1 = q ? hist[256 + tid] : n0;
    __syncthreads();   // sc and out may still be read
    sc[0][tid] = n0;
    sc[1][tid] = n1;
    if (tid < kStateWords) out[tid] = 0;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
        const unsigned a0 = tid >= off ? sc[0][tid - off] : 0u, a1 = tid >= off ? sc[1][tid - off] : 0u;
        __syncthreads();
        sc[0][tid] += a0;
        sc[1][tid] += a1;
        __syncthreads();
    }
    unsigned prefix0 = 0, prefix1 = 0, rank0, rank1;
    if (q) {
        prefix0 = in[0];
        prefix1 = in[1];
        rank0 = in[2];
        rank1 = in[3];
    } else {
        const unsigned n = sc[0][255];
        rank0 = (n - 1) / 2;   // n = 0: no bin has a count, so the rank is not looked at
        rank1 = n / 2;
    }
    // exactly one bin holds each rank: the counts of a pass add up to the rank's range
    const unsigned i0 = sc[0][tid], i1 = sc[1][tid];
    if (n0 && i0 - n0 <= rank0 && rank0 < i0) {
        out[0] = (prefix0 << 8) | (unsigned)tid;
        out[2] = rank0 - (i0 - n0);
    }
    if (n1 && i1 - n1 <= rank1 && rank1 < i1) {
        out[1] = (prefix1 << 8) | (unsigned)tid;
        out[3] = rank1 - (i1 - n1);
    }
    __syncthreads();
}

}  // namespace
