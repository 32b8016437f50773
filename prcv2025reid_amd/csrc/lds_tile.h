// LDS tile primitives shared by the gfx950 kernels: address-space types, the source swizzles of the LDS images, LDS-DMA from
// inline assembly, transposed fragment reads and counted waits.  The ONE definition of each ("hipcc and the
// vector-memory counter"); the kernel files only use them.
#pragma once
#include "common.h"

namespace ldstile {

typedef const __attribute__((address_space(1))) void* gptr_t;    // operands of __builtin_amdgcn_global_load_lds
typedef __attribute__((address_space(3))) void* lptr_t;
typedef __attribute__((ext_vector_type(4))) short s4;             // result of one ds_read_b64_tr_b16
typedef __attribute__((address_space(3))) s4* lds_s4_ptr;
typedef __attribute__((address_space(3))) char* lds_cptr;

// physical 16-byte chunk of logical chunk c in row `row` of a [rows][64] 16-bit tile (128-byte rows).
// Two rows share one 256-byte bank row; rows r and r+2 would otherwise collide on every ds_read_b128.
__device__ __forceinline__ int swz(int row, int c) { return c ^ ((row >> 1) & 7); }
// the same for images whose rows are a multiple of 512 bytes (a row starts a bank row: the row's low four bits spread the chunks)
__device__ __forceinline__ int swz512(int row, int c) { return c ^ (row & 15); }

// One LDS-DMA wave-instruction of such a [rows][64] image: rows rblk .. rblk + 7 (1 KiB, lane-linear in LDS), the swizzle applied to the
// SOURCE chunk.  src_of(row, chunk) = global address of that 16-byte chunk (the caller's row clamp and column offset).
template <typename SrcOf>
__device__ __forceinline__ void stage_rows8(char* lds, int rblk, int lane, SrcOf src_of) {
    const int row = rblk + (lane >> 3);
    __builtin_amdgcn_global_load_lds((gptr_t)src_of(row, swz(row, lane & 7)), (lptr_t)(lds + rblk * 128), 16, 0, 0);
}

// 32-bit LDS address of a pointer into a __shared__ array
__device__ __forceinline__ uint32_t lds_addr(const void* ptr) { return (uint32_t)(uintptr_t)(lds_cptr)(char*)ptr; }

// One LDS-DMA wave-instruction (64 lanes x 16 bytes -> 1 KiB of LDS at `lds_base`, wave-uniform) issued from inline assembly: hipcc then
// has no vector-memory operation of the ring in its scoreboard.  With the builtin it places `s_waitcnt vmcnt(0)` in front of every
// ds_read_b64_tr_b16 while a DMA is outstanding -- the transposed reads of every step then wait for the WHOLE ring (first form of the
// adapter-gradient kernel: 10 GB/s per workgroup whatever the ring depth).  Consequently no other compiler-visible global access may sit
// inside a loop that keeps such a ring full (the compiler's own waits for it would drain the ring as well): outputs are kept in
// registers and written after the loop, or stored from inline assembly too.
// M0 = LDS base: clobbered by every call; nothing else in the kernels that use these touches M0.
#define REID_LDS_DMA(name, width, modifier)                                                                                        \
    __device__ __forceinline__ void name(const void* src, uint32_t lds_base) {                                                     \
        const uint32_t m0v = __builtin_amdgcn_readfirstlane(lds_base);                                                             \
        asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_" width " %0, off" modifier ::"v"(src), "s"(m0v) : "memory"); \
    }
REID_LDS_DMA(dma16, "dwordx4", "")
REID_LDS_DMA(dma16_coherent, "dwordx4", " sc1")                   // sc1: past the non-coherent caches (atomics' home)
REID_LDS_DMA(dma4, "dword", "")                                   // 64 lanes x 4 bytes -> 256 bytes of LDS
#undef REID_LDS_DMA

// Counted waits.  vmcnt completes in issue order: N = the newest vector-memory operations allowed to stay in flight.
template <int N> __device__ __forceinline__ void wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
__device__ __forceinline__ void wait_lgkm0() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }
// run-time, wave-uniform n (above 20: everything)
__device__ __forceinline__ void wait_vm(int n) {
    switch (n) {
#define REID_VM_CASE(N) case N: wait_vm<N>(); break;
        REID_VM_CASE(1) REID_VM_CASE(2) REID_VM_CASE(3) REID_VM_CASE(4) REID_VM_CASE(5) REID_VM_CASE(6) REID_VM_CASE(7) REID_VM_CASE(8)
        REID_VM_CASE(9) REID_VM_CASE(10) REID_VM_CASE(11) REID_VM_CASE(12) REID_VM_CASE(13) REID_VM_CASE(14) REID_VM_CASE(15) REID_VM_CASE(16)
        REID_VM_CASE(17) REID_VM_CASE(18) REID_VM_CASE(19) REID_VM_CASE(20)
#undef REID_VM_CASE
        default: wait_vm<0>(); break;
    }
}

// One hardware transpose read (ds_read_b64_tr_b16, cdna_hip_programming.md T10), and two of them as one MFMA operand: elements 0..3
// from `lo`, 4..7 from `hi`.
__device__ __forceinline__ s4 tr_read(const char* addr) { return __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4_ptr)addr); }
__device__ __forceinline__ bf16x8 tr_join(s4 lo, s4 hi) { return bf16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]}; }

// 16x16x32 operand from a row-major [k][col] 16-bit image of row pitch `pitch` bytes: its 16 MFMA rows are image COLUMNS col0 .. col0 + 15,
// its k are image rows k0 .. k0 + 31.  Each tr read covers a 4-row x 16-col block: lane 4q+p' of a 16-lane group supplies the address of
// block row q, columns 4p'..4p'+3, and lane i receives column i of the 4 rows.  The MFMA sums over k, so any assignment of image rows to
// (lane group fq, element j) is valid as long as BOTH operands use it: element j<4 is row 4fq+j, element j>=4 is row 16+4fq+(j-4).  A
// 32-lane half then touches 8 consecutive rows per read, which a 32-byte row padding spreads over all 64 banks (conflict free).
__device__ __forceinline__ bf16x8 tr_frag(const char* img, int pitch, int k0, int col0, int lane) {
    const int l16 = lane & 15, fq = lane >> 4;
    const int q = l16 >> 2, pp = l16 & 3;
    const char* a0 = img + (k0 + 4 * fq + q) * pitch + (col0 + 4 * pp) * 2;
    return tr_join(tr_read(a0), tr_read(a0 + 16 * pitch));
}

}  // namespace ldstile
