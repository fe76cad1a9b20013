// Dataset diversity on the device (the rules are in include/emdenoise.h): the arithmetic of the reference's
// misc_py/img_stats.py (gram, and the mean squared difference of two images' matrices), restated from its formulas.
//   zero_counts_kernel      the non-finite counts to 0
//   row_norms_kernel        n[b][i] = sum_k x[b][i][k]^2 in double, one wave per row, and the image's count of non-finite pixels
//   gram_tile_kernel<PAIR>  one 128 x 128 tile (tj >= ti) of x x^T on v_mfma_f32_32x32x2_f32, in chains of at most 256 columns that
//                           are folded into a float32 running total.  PAIR: the chains of two images side by side, the total of
//                           their difference, and the tile's sum of E^2 in double (no matrix is written); else the tile of D and
//                           its mirror image (through LDS, so that both are stored along rows)
//   ssd_final_kernel        a pair's tile sums in tile order / H^2, the status, NaN for a skipped pair
// No floating-point atomics, fixed summation orders, launches only.
#include <climits>

#include "emd_common.hpp"
#include "wave_reduce.hpp"

// E = (dn_i + dn_j) - 2 G, E * E and the sums round one operation at a time, as the header writes them.
#pragma clang fp contract(off)

namespace {

constexpr int kTile = EMD_DIVERSITY_TILE;       // rows and columns of x x^T per workgroup (4 waves of 64 x 64)
constexpr int kTileK = EMD_DIVERSITY_TILE_K;    // columns of x staged in LDS at a time
constexpr int kChain = EMD_DIVERSITY_CHAIN;     // columns per accumulator chain
constexpr int kLdk = kTileK + 1;                // LDS row stride in floats: 32 rows at one k fall on 32 banks
constexpr int kMaxB = 65535;
constexpr int kMaxW = 32768;
constexpr int kMaxHPair = 8192;
constexpr int kMaxHDist = 4096;
constexpr int kMaxP = 1 << 20;
static_assert(kChain % kTileK == 0 && kTile == 128 && kTileK == 32, "the staging maps below are written for 128 x 32 blocks");

using f32x16 = __attribute__((ext_vector_type(16))) float;

__device__ __forceinline__ bool nonfinite_bits(float v) { return (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u; }

// The non-finite counts start from a launch, not from a memset node (a small memset node replayed wrong bytes).
__global__ __launch_bounds__(256) void zero_counts_kernel(int* __restrict__ nonfinite, int B) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b < B) nonfinite[b] = 0;
}

// One wave per row: lane l adds the squares of the columns l, l + 64, ... in that order, then the butterfly of wave_sum.
__global__ __launch_bounds__(256) void row_norms_kernel(const float* __restrict__ x, int H, int W, double* __restrict__ norms,
                                                        int* __restrict__ nonfinite) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), b = blockIdx.y;
    if (row >= H) return;
    const float* xr = x + ((size_t)b * H + row) * W;
    double s = 0.0;
    int bad = 0;
    for (int k = lane; k < W; k += 64) {
        const float v = xr[k];
        s += (double)v * (double)v;
        bad += nonfinite_bits(v);
    }
    s = emd::wave_sum(s);
    bad = emd::wave_sum(bad);
    if (lane == 0) {
        norms[(size_t)b * H + row] = s;
        if (bad) atomicAdd(&nonfinite[b], bad);
    }
}

// The workgroup's share of a 32-column block: rows [rA, rA + 128) and [rB, rB + 128), 8 float4 a thread.  Rows >= H and columns >= W
// are never read: their addresses are clamped into the image and the values replaced by zeros.
__device__ __forceinline__ void fetch_block(const float* __restrict__ xi, int H, int W, int rA, int rB, int k0, bool vec,
                                            float4 (&R)[8]) {
    const float* p[8];
    bool in[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int idx = threadIdx.x + 256 * (q & 3);
        const int row = (q < 4 ? rA : rB) + (idx >> 3);
        in[q] = row < H;
        p[q] = xi + (size_t)(in[q] ? row : H - 1) * W;
    }
    const int k = k0 + (threadIdx.x & 7) * 4;
    if (vec && k0 + kTileK <= W) {   // one branch around all eight loads, none around each
#pragma unroll
        for (int q = 0; q < 8; ++q) R[q] = *reinterpret_cast<const float4*>(p[q] + k);
    } else {
        const int last = W - 1;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            float4 v;
            v.x = p[q][k < last ? k : last];
            v.y = p[q][k + 1 < last ? k + 1 : last];
            v.z = p[q][k + 2 < last ? k + 2 : last];
            v.w = p[q][k + 3 < last ? k + 3 : last];
            if (k >= W) v.x = 0.f;
            if (k + 1 >= W) v.y = 0.f;
            if (k + 2 >= W) v.z = 0.f;
            if (k + 3 >= W) v.w = 0.f;
            R[q] = v;
        }
    }
#pragma unroll
    for (int q = 0; q < 8; ++q)
        if (!in[q]) R[q] = make_float4(0.f, 0.f, 0.f, 0.f);
}

// sm: [2 operands][128 rows][kLdk]
__device__ __forceinline__ void store_block(float* sm, const float4 (&R)[8]) {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int idx = threadIdx.x + 256 * (q & 3);
        float* d = sm + (q < 4 ? 0 : kTile * kLdk) + (idx >> 3) * kLdk + (idx & 7) * 4;
        d[0] = R[q].x;
        d[1] = R[q].y;
        d[2] = R[q].z;
        d[3] = R[q].w;
    }
}

// 16 steps of k = (2 s, 2 s + 1) in ascending order on the wave's 2 x 2 tiles of 32 x 32: lane l holds A[i = l & 31][k = l >> 5]
// and B[k = l >> 5][j = l & 31], one float each.
__device__ __forceinline__ void mma_block(const float* sa, const float* sb, f32x16 (&acc)[2][2]) {
#pragma unroll
    for (int s = 0; s < kTileK / 2; ++s) {
        const float a0 = sa[2 * s], a1 = sa[32 * kLdk + 2 * s];
        const float b0 = sb[2 * s], b1 = sb[32 * kLdk + 2 * s];
        acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
    }
}

__device__ __forceinline__ void clear(f32x16 (&acc)[2][2]) {
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n) acc[m][n] = (f32x16)(0.f);
}

// Grid: unit * tiles + t, t the upper tile (ti, tj >= ti) in row-major order; unit = the pair (PAIR) or the image.
// PAIR:  tile_sums[unit][t] = weight * sum over the tile of E^2, weight 1 on the diagonal and 2 off it (exact).  A pair with an index
//        outside [0, B) or an image with a non-finite pixel is left alone: nothing is read through it, ssd_final_kernel reports it.
// else:  D[unit][i][j] and D[unit][j][i] for the tile.
template <bool PAIR>
__global__ __launch_bounds__(256) void gram_tile_kernel(const float* __restrict__ x, int B, int H, int W, int T, int tiles, int vec,
                                                        const int* __restrict__ pairs, const double* __restrict__ norms,
                                                        const int* __restrict__ nonfinite, double* __restrict__ tile_sums,
                                                        float* __restrict__ D) {
    __shared__ __attribute__((aligned(16))) float sm[2 * kTile * kLdk];
    const int unit = blockIdx.x / tiles, t = blockIdx.x - unit * tiles;
    int ia = unit, ib = unit;
    if (PAIR) {
        ia = pairs[2 * unit];
        ib = pairs[2 * unit + 1];
        if ((unsigned)ia >= (unsigned)B || (unsigned)ib >= (unsigned)B) return;
        if (nonfinite[ia] != 0 || nonfinite[ib] != 0) return;
    }
    int ti = 0, rem = t;
    while (rem >= T - ti) {
        rem -= T - ti;
        ++ti;
    }
    const int tj = ti + rem;
    const int rA = ti * kTile, rB = tj * kTile;
    const size_t image = (size_t)H * W;
    const float* xa = x + (size_t)ia * image;
    const float* xb = x + (size_t)ib * image;

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wr = wave >> 1, wc = wave & 1;
    const float* sa = sm + (wr * 64 + (lane & 31)) * kLdk + (lane >> 5);
    const float* sb = sm + kTile * kLdk + (wc * 64 + (lane & 31)) * kLdk + (lane >> 5);

    // One accumulator set runs a chain of image a, is set aside (hold), runs the same columns of image b, and the two are folded:
    // hold and tot are idle while the matrix cores work, so only acc has to sit where the MFMAs want it.
    f32x16 acc[2][2], hold[2][2], tot[2][2];   // tot: G (single image) or Gd = the folded (chain of a) - (chain of b)
    clear(acc);
    clear(tot);
    float4 R[8];
    const int nkb = (W + kTileK - 1) / kTileK;
    constexpr int kPerChain = kChain / kTileK;
    fetch_block(xa, H, W, rA, rB, 0, vec != 0, R);
    for (int kb0 = 0; kb0 < nkb; kb0 += kPerChain) {
        const int nb = nkb - kb0 < kPerChain ? nkb - kb0 : kPerChain;
        for (int i = 0; i < nb; ++i) {   // image a's chain; the next block is in flight while this one is multiplied
            store_block(sm, R);
            __syncthreads();
            const bool more = i + 1 < nb;
            if (more || PAIR || kb0 + nb < nkb)
                fetch_block(more || !PAIR ? xa : xb, H, W, rA, rB, (more ? kb0 + i + 1 : (PAIR ? kb0 : kb0 + nb)) * kTileK, vec != 0, R);
            mma_block(sa, sb, acc);
            __syncthreads();
        }
        if (PAIR) {
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int n = 0; n < 2; ++n) hold[m][n] = acc[m][n];
            clear(acc);
            for (int i = 0; i < nb; ++i) {   // the same columns of image b
                store_block(sm, R);
                __syncthreads();
                const bool more = i + 1 < nb;
                if (more || kb0 + nb < nkb) fetch_block(more ? xb : xa, H, W, rA, rB, (more ? kb0 + i + 1 : kb0 + nb) * kTileK, vec != 0, R);
                mma_block(sa, sb, acc);
                __syncthreads();
            }
        }
#pragma unroll
        for (int m = 0; m < 2; ++m)   // the chain's end
#pragma unroll
            for (int n = 0; n < 2; ++n) tot[m][n] += PAIR ? hold[m][n] - acc[m][n] : acc[m][n];
        clear(acc);
    }

    // C/D map of the 32 x 32 forms: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
    const int i0 = rA + wr * 64 + 4 * (lane >> 5), j0 = rB + wc * 64 + (lane & 31);
    const int top = H - 1;
    const double* na = norms + (size_t)ia * H;
    const double* nb = norms + (size_t)ib * H;
    if (PAIR) {
        double s = 0.0;
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int n = 0; n < 2; ++n) {
                const int j = j0 + n * 32, jc = j < top ? j : top;
                const double dnj = na[jc] - nb[jc];
#pragma unroll
                for (int reg = 0; reg < 16; ++reg) {
                    const int i = i0 + m * 32 + (reg & 3) + 8 * (reg >> 2), ic = i < top ? i : top;
                    const double dni = na[ic] - nb[ic];
                    const double E = (dni + dnj) - 2.0 * (double)tot[m][n][reg];
                    if (i < H && j < H) s += E * E;
                }
            }
        s = emd::wave_sum(s);
        double* red = reinterpret_cast<double*>(sm);   // the main loop ended on a barrier
        if (lane == 0) red[wave] = s;
        __syncthreads();
        if (threadIdx.x == 0) {
            const double sum = ((red[0] + red[1]) + red[2]) + red[3];
            tile_sums[(size_t)unit * tiles + t] = ti == tj ? sum : 2.0 * sum;
        }
    } else {
        float* Db = D + (size_t)unit * H * H;
        float* st = sm + wave * (32 * kLdk);
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int n = 0; n < 2; ++n) {
                const int j = j0 + n * 32;
                const double nj = na[j < top ? j : top];
                if (ti != tj) __syncthreads();   // the previous sub-tile's mirror has been read
#pragma unroll
                for (int reg = 0; reg < 16; ++reg) {
                    const int r = (reg & 3) + 8 * (reg >> 2);
                    const int i = i0 + m * 32 + r;
                    const double ni = na[i < top ? i : top];
                    const float d = (float)((ni + nj) - 2.0 * (double)tot[m][n][reg]);
                    if (i < H && j < H) Db[(size_t)i * H + j] = d;
                    if (ti != tj) st[(r + 4 * (lane >> 5)) * kLdk + (lane & 31)] = d;
                }
                if (ti != tj) {   // the mirror image: 32 lanes along i
                    __syncthreads();
                    const int ib0 = rA + wr * 64 + m * 32, jb0 = rB + wc * 64 + n * 32;
#pragma unroll
                    for (int q = 0; q < 16; ++q) {
                        const int r = lane & 31, c = 2 * q + (lane >> 5);
                        const int i = ib0 + r, jj = jb0 + c;
                        if (i < H && jj < H) Db[(size_t)jj * H + i] = st[r * kLdk + c];
                    }
                }
            }
    }
}

// One wave per pair: lane l adds the tiles l, l + 64, ... in that order, then the butterfly.
__global__ __launch_bounds__(64) void ssd_final_kernel(const int* __restrict__ pairs, int B, int H, int tiles,
                                                       const int* __restrict__ nonfinite, const double* __restrict__ tile_sums,
                                                       double* __restrict__ ssd, int* __restrict__ status) {
    const int p = blockIdx.x, lane = threadIdx.x;
    const int ia = pairs[2 * p], ib = pairs[2 * p + 1];
    int code = EMD_DIVERSITY_OK;
    if ((unsigned)ia >= (unsigned)B || (unsigned)ib >= (unsigned)B)
        code = EMD_DIVERSITY_BAD_INDEX;
    else if (nonfinite[ia] != 0 || nonfinite[ib] != 0)
        code = EMD_DIVERSITY_NONFINITE;
    double s = 0.0;
    if (code == EMD_DIVERSITY_OK) {
        for (int t = lane; t < tiles; t += 64) s += tile_sums[(size_t)p * tiles + t];
        s = emd::wave_sum(s) / ((double)H * (double)H);
    } else {
        s = __longlong_as_double(0x7ff8000000000000LL);
    }
    if (lane == 0) {
        ssd[p] = s;
        status[p] = code;
    }
}

int tiles_per_side(int H) { return emd::tiles_of(H, kTile); }
int upper_tiles(int H) {
    const int T = tiles_per_side(H);
    return T * (T + 1) / 2;
}
size_t norms_bytes(int B, int H) { return emd::round256((size_t)B * H * sizeof(double)); }
size_t counts_bytes(int B) { return emd::round256((size_t)B * sizeof(int)); }

bool shape_ok(const char* who, int B, int H, int W, int max_h) {
    if (B < 0 || B > kMaxB) {
        emd::set_error("%s: 0 <= B <= %d (got %d)", who, kMaxB, B);
        return false;
    }
    if (H < 1 || H > max_h || W < 1 || W > kMaxW) {
        emd::set_error("%s: 1 <= H <= %d, 1 <= W <= %d (got %d x %d)", who, max_h, kMaxW, H, W);
        return false;
    }
    return true;
}

int launch_norms(const float* x, int B, int H, int W, double* norms, int* nonfinite, hipStream_t st) {
    hipLaunchKernelGGL(zero_counts_kernel, dim3((unsigned)emd::tiles_of(B, 256)), dim3(256), 0, st, nonfinite, B);
    hipLaunchKernelGGL(row_norms_kernel, dim3((unsigned)emd::tiles_of(H, 4), (unsigned)B), dim3(256), 0, st, x, H, W, norms, nonfinite);
    return emd::check_launch("row_norms_kernel");
}

int vec_ok(const float* x, int W) { return W % 4 == 0 && emd::aligned16(x); }

}  // namespace

extern "C" int emd_row_sq_norms_f64(const float* x, int B, int H, int W, double* norms, int* nonfinite, emd_stream_t stream) {
    if (!shape_ok("emd_row_sq_norms_f64", B, H, W, kMaxHPair)) return EMD_E_INVALID;
    if (B == 0) return EMD_OK;
    const emd::Range r[] = {{x, (size_t)B * H * W * sizeof(float), 4, false, true},
                            {norms, (size_t)B * H * sizeof(double), 8, false, false},
                            {nonfinite, (size_t)B * sizeof(int), 4, false, false}};
    const int rc = emd::check_ranges("emd_row_sq_norms_f64", r, 3, "norms must be 8-byte aligned, x and nonfinite 4-byte");
    if (rc != EMD_OK) return rc;
    return launch_norms(x, B, H, W, norms, nonfinite, static_cast<hipStream_t>(stream));
}

extern "C" size_t emd_row_distances_workspace_bytes(int B, int H, int W) {
    if (B < 1 || B > kMaxB || H < 1 || H > kMaxHDist || W < 1 || W > kMaxW) return 0;
    return norms_bytes(B, H) + counts_bytes(B);
}

extern "C" int emd_row_distances_f32(const float* x, int B, int H, int W, float* D, void* workspace, size_t workspace_bytes,
                                     emd_stream_t stream) {
    if (!shape_ok("emd_row_distances_f32", B, H, W, kMaxHDist)) return EMD_E_INVALID;
    if (B == 0) return EMD_OK;
    const size_t need = emd_row_distances_workspace_bytes(B, H, W);
    const emd::Range r[] = {{workspace, need, 16, false, false},
                            {x, (size_t)B * H * W * sizeof(float), 4, false, true},
                            {D, (size_t)B * H * H * sizeof(float), 4, false, false}};
    int rc = emd::check_ranges("emd_row_distances_f32", r, 3, "the workspace must be 16-byte aligned, x and D 4-byte", &workspace_bytes);
    if (rc != EMD_OK) return rc;
    double* norms = static_cast<double*>(workspace);
    int* nonfinite = reinterpret_cast<int*>(static_cast<char*>(workspace) + norms_bytes(B, H));
    hipStream_t st = static_cast<hipStream_t>(stream);
    rc = launch_norms(x, B, H, W, norms, nonfinite, st);
    if (rc != EMD_OK) return rc;
    const int tiles = upper_tiles(H);
    hipLaunchKernelGGL(gram_tile_kernel<false>, dim3((unsigned)(B * tiles)), dim3(256), 0, st, x, B, H, W, tiles_per_side(H), tiles,
                       vec_ok(x, W), (const int*)nullptr, (const double*)norms, (const int*)nonfinite, (double*)nullptr, D);
    return emd::check_launch("gram_tile_kernel (distances)");
}

extern "C" size_t emd_gram_ssd_workspace_bytes(int B, int H, int W, int P) {
    if (B < 1 || B > kMaxB || H < 1 || H > kMaxHPair || W < 1 || W > kMaxW || P < 1 || P > kMaxP) return 0;
    return norms_bytes(B, H) + counts_bytes(B) + emd::round256((size_t)P * upper_tiles(H) * sizeof(double));
}

extern "C" int emd_gram_ssd_f64(const float* x, int B, int H, int W, const int* pairs, int P, double* ssd, int* status, void* workspace,
                                size_t workspace_bytes, emd_stream_t stream) {
    if (!shape_ok("emd_gram_ssd_f64", B, H, W, kMaxHPair)) return EMD_E_INVALID;
    if (P < 0 || P > kMaxP) {
        emd::set_error("emd_gram_ssd_f64: 0 <= P <= %d (got %d)", kMaxP, P);
        return EMD_E_INVALID;
    }
    const int tiles = upper_tiles(H);
    if ((long long)P * tiles > INT_MAX) {
        emd::set_error("emd_gram_ssd_f64: P times the %d tiles of an image exceeds 2^31 - 1 (P = %d): split the pair list", tiles, P);
        return EMD_E_INVALID;
    }
    if (B == 0 || P == 0) return EMD_OK;
    const size_t need = emd_gram_ssd_workspace_bytes(B, H, W, P);
    const emd::Range r[] = {{workspace, need, 16, false, false},
                            {x, (size_t)B * H * W * sizeof(float), 4, false, true},
                            {pairs, (size_t)P * 2 * sizeof(int), 4, false, true},
                            {ssd, (size_t)P * sizeof(double), 8, false, false},
                            {status, (size_t)P * sizeof(int), 4, false, false}};
    int rc = emd::check_ranges("emd_gram_ssd_f64", r, 5, "the workspace must be 16-byte aligned, ssd 8-byte, x, pairs and status 4-byte",
                               &workspace_bytes);
    if (rc != EMD_OK) return rc;
    char* w = static_cast<char*>(workspace);
    double* norms = reinterpret_cast<double*>(w);
    int* nonfinite = reinterpret_cast<int*>(w + norms_bytes(B, H));
    double* tile_sums = reinterpret_cast<double*>(w + norms_bytes(B, H) + counts_bytes(B));
    hipStream_t st = static_cast<hipStream_t>(stream);
    rc = launch_norms(x, B, H, W, norms, nonfinite, st);
    if (rc != EMD_OK) return rc;
    hipLaunchKernelGGL(gram_tile_kernel<true>, dim3((unsigned)(P * tiles)), dim3(256), 0, st, x, B, H, W, tiles_per_side(H), tiles,
                       vec_ok(x, W), pairs, (const double*)norms, (const int*)nonfinite, tile_sums, (float*)nullptr);
    rc = emd::check_launch("gram_tile_kernel (pairs)");
    if (rc != EMD_OK) return rc;
    hipLaunchKernelGGL(ssd_final_kernel, dim3((unsigned)P), dim3(64), 0, st, pairs, B, H, tiles, (const int*)nonfinite,
                       (const double*)tile_sums, ssd, status);
    return emd::check_launch("ssd_final_kernel");
}
