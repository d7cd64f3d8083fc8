// The gfx950 device primitives every MFMA kernel family of libflairhip shares: the LDS-DMA statement and its zero
// source, the hand-written wait / barrier forms that go with it, the division of block-uniform indices by host-made
// multipliers, the transposing LDS read and the 32x32 MFMA step.
// One copy: a change to one of these idioms (a hazard nop, the M0 rule) is made here and nowhere else.
#pragma once
#include "ffa_common.h"

// One LDS-DMA instruction: 64 lanes x 16 bytes from per-lane global addresses `src` to LDS at lds_base + lane * 16.
//   * lds_base is wave-uniform and travels through M0.  M0 is compiler-reserved and not preserved around a statement,
//     so it is saved, written and restored inside this ONE statement; the s_nop 0 sits between the M0 write and the
//     load that reads it.
//   * Inline asm on purpose: with __builtin_amdgcn_global_load_lds in the kernel hipcc (ROCm 7.2) stops counting
//     lgkmcnt and drains it to 0 in front of every MFMA step (532 of 789 waits were lgkmcnt(0) in conv3x3_ring_kernel;
//     without the builtin they are counted), which stalls every step on the fragment reads just issued for later
//     steps.
//   * The DMA is invisible to the compiler: its completion is waited for by hand with the vmcnt forms below (the
//     compiler's own vmcnt waits can only become stricter through the extra entries in the queue), and a block must
//     drain vmcnt(0) before it ends -- nothing of it may still be writing its LDS.
__device__ __forceinline__ void ffa_lds_dma16(const unsigned char* src, unsigned lds_base) {
  unsigned keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(src), "s"(lds_base)
      : "memory");
}

// The same with a wave-uniform source: `base` stays in a scalar register pair, the lane contributes the 32-bit byte
// offset `voff` -- no 64-bit vector address is built per instruction.
__device__ __forceinline__ void ffa_lds_dma16_uniform(const unsigned char* base, unsigned voff, unsigned lds_base) {
  unsigned keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(voff), "s"(base), "s"(lds_base)
      : "memory");
}

// n / d and the remainder for a block-uniform n < 2^31 on the scalar unit.  m = 0xffffffff / d comes from the host
// (ffa_udiv_magic_of); mulhi(n, m) is the quotient or one short of it (n / d - n * m / 2^32 < 2 n / 2^32 < 1), so one
// correction step makes it exact for every d >= 1.
__device__ __forceinline__ unsigned ffa_udiv_magic(unsigned n, unsigned d, unsigned m, unsigned& rem) {
  unsigned q = __umulhi(n, m);
  unsigned r = n - q * d;
  if (r >= d) {
    ++q;
    r -= d;
  }
  rem = r;
  return q;
}
static inline unsigned ffa_udiv_magic_of(int d) { return 0xffffffffu / (unsigned)d; }

// 16 zero bytes in global memory: the source of LDS-DMA pieces that lie outside the image (padding, ragged edges).
// Internal linkage: every translation unit that uses it has a copy of its own (-fno-gpu-rdc).
static __device__ __attribute__((aligned(16))) const unsigned int ffa_zero16[4] = {0u, 0u, 0u, 0u};

// Waits written by hand, each ONE asm statement with a memory clobber: neither the compiler's own LDS accesses nor its
// loads move across it.  vmcnt(N): this wave's LDS-DMA has landed except for its newest N vector-memory operations.
template <int N>
__device__ __forceinline__ void ffa_wait_vm() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"i"(N) : "memory");
}
// ... then the block meets (raw s_barrier: a __syncthreads() would add vmcnt(0) and end the prefetch); LDS reads
// requested for later steps stay in flight across the barrier
template <int N>
__device__ __forceinline__ void ffa_wait_vm_barrier() {
  asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"i"(N) : "memory");
}
// the same, and this wave's own LDS stores are in LDS too
template <int N>
__device__ __forceinline__ void ffa_wait_vm_lgkm_barrier() {
  asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" ::"i"(N) : "memory");
}
// LDS stores only: the DMA in flight stays in flight
__device__ __forceinline__ void ffa_wait_lgkm_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// 4 pixels x 16 channels of bf16, transposed: lane (16-lane group member li) passes the address of
// pixel row (li >> 2), 8-byte segment (li & 3); it receives channel li of the four pixels.
__device__ __forceinline__ ffa_s16x4 ffa_lds_read_tr16(const unsigned char* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16(
      (__attribute__((address_space(3))) ffa_s16x4*)(const_cast<unsigned char*>(p)));
}

// One 32x32 MFMA step over a 16-byte fragment per lane (ffa_common.h): PER instructions.
template <typename T>
struct Mma;
template <>
struct Mma<ffa_bf16> {
  static constexpr int PER = 1;
  static __device__ __forceinline__ void run(const ffa_u32x4& a, const ffa_u32x4& b, ffa_f32x16& c) {
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(ffa_bf16x8, a), __builtin_bit_cast(ffa_bf16x8, b),
                                                c, 0, 0, 0);
  }
};
template <>
struct Mma<float> {
  static constexpr int PER = 4;
  static __device__ __forceinline__ void run(const ffa_u32x4& a, const ffa_u32x4& b, ffa_f32x16& c) {
    c = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.x), __uint_as_float(b.x), c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.y), __uint_as_float(b.y), c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.z), __uint_as_float(b.z), c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.w), __uint_as_float(b.w), c, 0, 0, 0);
  }
};
