// Device primitives of the matrix-core kernels: the vector and address-space types, the hand-written waits, loads and stores, the DPP
// lane exchanges and the XCD tile-order remap.  ONE definition of each: a hazard fixed here is fixed in every kernel.
#pragma once

#include <hip/hip_runtime.h>

namespace emd {

typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;      // native vectors for the staging registers:
typedef __attribute__((ext_vector_type(4))) unsigned u32x4;   // HIP's float4/uint4 structs end up in scratch
typedef __attribute__((ext_vector_type(2))) unsigned u32x2;

typedef const __attribute__((address_space(1))) void* gptr_t;   // the operand types of __builtin_amdgcn_global_load_lds
typedef __attribute__((address_space(3))) void* lptr_t;

template <int N>
__device__ __forceinline__ void wait_vm() {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N < 63 ? N : 63) : "memory");
}
__device__ __forceinline__ void wait_lgkm0() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

// Fragment reads by hand: the compiler neither sees them nor waits for them (it would wait with lgkmcnt(0), i.e. also for the NEXT
// unit's reads issued behind them); the wait in front of a unit's MFMAs lets the younger reads stay in flight and ties the registers.
template <int OFF>
__device__ __forceinline__ bf16x8 lds_read16(const unsigned char* p) {
    bf16x8 v;
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"((lptr_t)p), "n"(OFF) : "memory");
    return v;
}

// Epilogue accesses: scalar base (a pixel of the tile row, uniform) + 32-bit lane offset, 16 bytes per lane; the stores non-temporal
// (the outputs are not re-read by this launch: L2 is kept for the patch halos).  Inline asm: the address form costs one VGPR per lane
// instead of a 64-bit pointer per access, and the loads are waited for by hand (wait_vm) -- the compiler does not see them.
// 16 bytes per lane, not 4: tools/dmabench.hip measures dword stores of this shape at 2.9 TB/s against 6.0 for dwordx4.
// The s_nop covers the store-data hazard the compiler cannot see inside the asm: a store of more than 64 bits reads its data late, and a
// VALU write to those registers must stay >= 2 wait states behind it on this ISA (LLVM's hazard recognizer: 2 for gfx940+).  Rounds 1-3
// had "s_nop 0" (ONE wait state), which held while the compiler happened to put other work first; round 4's epilogue with plain residual
// loads got a v_lshl_add_u64 (the next load's address, allocated INTO the dead store-data registers) two instructions behind the
// store, and the last four lanes of every 16 stored the address words instead of two channels -- intermittently, 64 values per tile
// (tools/sep2_debug.py).  s_nop 3 = four wait states, behind every 16-byte store below.
__device__ __forceinline__ void store_nt_s(const void* sbase, unsigned voff, f32x4 v) {
    asm volatile("global_store_dwordx4 %0, %1, %2 nt\n\ts_nop 3" ::"v"(voff), "v"(v), "s"(sbase) : "memory");
}
__device__ __forceinline__ void store_nt_s(const void* sbase, unsigned voff, u32x4 v) {
    asm volatile("global_store_dwordx4 %0, %1, %2 nt\n\ts_nop 3" ::"v"(voff), "v"(v), "s"(sbase) : "memory");
}
__device__ __forceinline__ f32x4 load_s(const void* sbase, unsigned voff) {
    f32x4 v;
    asm volatile("global_load_dwordx4 %0, %1, %2" : "=v"(v) : "v"(voff), "s"(sbase) : "memory");
    return v;
}
__device__ __forceinline__ float load_s1(const void* sbase, unsigned voff) {
    float v;
    asm volatile("global_load_dword %0, %1, %2" : "=v"(v) : "v"(voff), "s"(sbase) : "memory");
    return v;
}
// One dword per lane (EPI = 1: a lane = one channel, the layout the MFMA leaves): no data hazard to cover, no transpose before it.
__device__ __forceinline__ void store_nt_d(const void* sbase, unsigned voff, unsigned v) {
    asm volatile("global_store_dword %0, %1, %2 nt" ::"v"(voff), "v"(v), "s"(sbase) : "memory");
}
// One dword per lane through a 64-bit lane address, cached (sep_pipe.hip's folded epilogue: the tap planes are read back by the next launch).
__device__ __forceinline__ void store_d(void* dst, float v) {
    asm volatile("global_store_dword %0, %1, off" ::"v"(dst), "v"(v) : "memory");
}
// The pointer form of the 16-byte non-temporal store.  Inline asm on purpose: behind a run-time flag, "if (nt) __builtin_nontemporal_store
// else plain store" is merged into ONE plain store by the optimizer (the merged store keeps only the metadata both sides share).
__device__ __forceinline__ void store_nt16(void* dst, f32x4 v) {
    asm volatile("global_store_dwordx4 %0, %1, off nt\n\ts_nop 3" ::"v"(dst), "v"(v) : "memory");
}
__device__ __forceinline__ void store_nt16(void* dst, u32x4 v) {
    asm volatile("global_store_dwordx4 %0, %1, off nt\n\ts_nop 3" ::"v"(dst), "v"(v) : "memory");
}

// The value of the other lane of an (even, odd) lane pair: a DPP quad permute [1,0,3,2] -- what __shfl_xor(v, 1) returns, without
// the trip through the LDS crossbar (ds_bpermute) that the HIP shuffle compiles to.
__device__ __forceinline__ unsigned swap_pair(unsigned v) {
    return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, true);
}
__device__ __forceinline__ float dpp_f(float v, int ctrl_is_xor2) {
    return ctrl_is_xor2 ? __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, true))
                        : __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true));
}
// 4 x 4 transpose inside a lane quad (two DPP exchange rounds): in, lane i holds column i of the block (r[k] = a[k][i]); out, row i
// (r[k] = a[i][k]).  It turns the MFMA C/D layout (a lane = one channel, four pixels) into one pixel's four consecutive channels.
__device__ __forceinline__ void quad_transpose(float (&r)[4], int li) {
    const bool b0 = li & 1, b1 = li & 2;
    float s0 = b0 ? r[0] : r[1], s1 = b0 ? r[2] : r[3];
    s0 = dpp_f(s0, 0);
    s1 = dpp_f(s1, 0);
    r[0] = b0 ? s0 : r[0]; r[1] = b0 ? r[1] : s0;
    r[2] = b0 ? s1 : r[2]; r[3] = b0 ? r[3] : s1;
    float t0 = b1 ? r[0] : r[2], t1 = b1 ? r[1] : r[3];
    t0 = dpp_f(t0, 1);
    t1 = dpp_f(t1, 1);
    r[0] = b1 ? t0 : r[0]; r[2] = b1 ? r[2] : t0;
    r[1] = b1 ? t1 : r[1]; r[3] = b1 ? r[3] : t1;
}
// the value of the lane 4 further on (lanes of an even channel quad) / 4 back (odd quad): the split32 pair exchange
__device__ __forceinline__ unsigned xchg4(unsigned v, bool oddq) {
    const unsigned up = (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x104, 0xF, 0xF, true);   // row_shl:4
    const unsigned dn = (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xF, 0xF, true);   // row_shr:4
    return oddq ? dn : up;
}

// Workgroup ids are dealt to the 8 XCDs round-robin (id mod 8).  With `on`, XCD k takes the k-th contiguous eighth of the 3-D tile list
// instead: the tiles that share halo rows meet in one L2.  bx, by, bz come in as blockIdx; `on` needs a tile count divisible by 8.
// (sep_pipe.hip keeps this block written out: called from there, the helper changes that kernel's register allocation.  The operand
// order of `total` is deliberate too: z * (x * y) compiles to the instructions the written-out blocks gave, x * y * z commutes one s_mul.)
__device__ __forceinline__ void xcd_remap(bool on, int& bx, int& by, int& bz) {
    if (on) {
        const unsigned total = gridDim.z * (gridDim.x * gridDim.y);
        const unsigned id = blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z);
        const unsigned t = (id & 7) * (total >> 3) + (id >> 3);
        bx = t % gridDim.x;
        by = (t / gridDim.x) % gridDim.y;
        bz = t / (gridDim.x * gridDim.y);
    }
}

}  // namespace emd
