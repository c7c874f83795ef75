// Device primitives every kernel file shares (gfx950 only), each written once: the LDS-DMA issue, the s_waitcnt encodings and
// the barriers built on them, the zero block, the XCD-aware block remap, Philox with its uniform and Box-Muller maps, and the
// small arithmetic helpers.
// A kernel file does not call the DMA builtin or write a s_waitcnt immediate itself: it uses these.
#pragma once
#include "gad_common.h"

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// 64 bytes of zeros in device memory: the DMA source of padding / out-of-range tile slots (one per translation unit).
// A user names the member of its element type (g_zero_block.f32, .b16, .u32) and needs no cast.  The views are members and not
// an accessor function on purpose: through a function's returned pointer hipcc generated different code for the kernels.
union ZeroBlock {
  float f32[16];
  unsigned short b16[32];
  unsigned int u32[16];
};
static __device__ __attribute__((aligned(64))) ZeroBlock g_zero_block;

// LDS-DMA: 64 lanes x 16 B -> LDS [dst, dst + 1 KiB), lane-linear; src is per lane
__device__ __forceinline__ void glds16(const void* src, void* lds_dst_wave_uniform) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                   (__attribute__((address_space(3))) void*)lds_dst_wave_uniform, 16, 0, 0);
}

// s_waitcnt immediate (gfx9) that waits for vmcnt <= n only: vmcnt = n (6 bits, split over bits 3:0 and 15:14),
// expcnt = 7 (bits 6:4, no wait), lgkmcnt = 15 (bits 11:8, no wait)
constexpr int vmcnt_imm(int n) { return (n & 15) | ((n >> 4) << 14) | 0x0F70; }
static_assert(vmcnt_imm(0) == 0x0F70, "vmcnt(0)");
static_assert(vmcnt_imm(5) == 0x0F75, "vmcnt low bits");
static_assert(vmcnt_imm(20) == 0x4F74, "vmcnt high bits");

// counted wait for LDS-DMA / loads: all but the N youngest vector-memory operations of this wave are done
template <int N>
__device__ __forceinline__ void wait_vm() {
  static_assert(N >= 0 && N < 64, "vmcnt is 6 bits on gfx9");
  __builtin_amdgcn_s_waitcnt(vmcnt_imm(N));
}
// ... followed by the workgroup barrier.  Not __syncthreads(): its workgroup-scope fence makes the compiler drain EVERY
// outstanding vector-memory operation (vmcnt(0)) - also the LDS-DMA of the stage-steps that are meant to stay in flight.
// The "memory" clobber keeps the compiler from moving LDS reads across; the stage published here is covered by the count.
template <int N>
__device__ __forceinline__ void barrier_vm() {
  static_assert(N >= 0 && N < 64, "vmcnt is 6 bits on gfx9");
  asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(N) : "memory");
}
// A barrier that publishes LDS-DMA'd tiles when nothing is meant to stay in flight: the DMA is a VMEM operation (vmcnt), and
// the compiler's own waitcnt placement at __syncthreads() only covers it when it happens to track the LDS side effect - so
// wait for it explicitly.
__device__ __forceinline__ void barrier_after_dma() {
  wait_vm<0>();
  __syncthreads();
}
// The raw barrier after LDS reads alone (immediate 0xC07F: lgkmcnt(0), vmcnt and expcnt at "no wait"): every wave is done
// reading, and the next tile's LDS-DMA stays in flight across it.
__device__ __forceinline__ void barrier_lgkm0() {
  __builtin_amdgcn_s_waitcnt(0xC07F);
  __builtin_amdgcn_s_barrier();
}

// Workgroup id -> work item, XCD-aware and bijective: hardware deals consecutive workgroup ids round-robin to the 8 XCDs
// (each with its own L2); this hands every XCD a CONTIGUOUS range of work items, so tiles that share an operand panel
// (neighbouring tile_n of one tile_m, the halo rows of neighbouring row tiles) meet in one L2.
__device__ __forceinline__ int xcd_remap(int bid, int nwg) {
  int xcd = bid & 7, q = nwg >> 3, rr = nwg & 7;
  return (xcd < rr ? xcd * (q + 1) : rr * (q + 1) + (xcd - rr) * q) + (bid >> 3);
}

// Philox-4x32-10 (Salmon et al. 2011): counter c, key (k0, k1)
__device__ __forceinline__ uint4 philox4x32_10(uint4 c, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c.x;
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c.z;
    const uint32_t hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0;
    const uint32_t hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
    c = make_uint4(hi1 ^ c.y ^ k0, lo1, hi0 ^ c.w ^ k1, lo0);
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return c;
}

// u = (x + 1/2) 2^-32 in (0, 1]: fl32(fl32(x) * 2^-32 + 2^-33), one fma (the restatement in tests/ does the same in fp64)
__device__ __forceinline__ float jl_uniform(uint32_t x) {
  return __builtin_fmaf((float)x, 0x1p-32f, 0x1p-33f);
}

// one Philox block -> four standard normals: Box-Muller on (u0, u1) and (u2, u3), in the order cos, sin, cos, sin
// (the projector's normal entries and the DDPM step's variance noise)
__device__ __forceinline__ void jl_normal4(uint4 x, float b[4]) {
  const float r01 = sqrtf(-2.0f * logf(jl_uniform(x.x)));
  const float r23 = sqrtf(-2.0f * logf(jl_uniform(x.z)));
  const float h1 = 2.0f * jl_uniform(x.y), h3 = 2.0f * jl_uniform(x.w);
  b[0] = r01 * cospif(h1);
  b[1] = r01 * sinpif(h1);
  b[2] = r23 * cospif(h3);
  b[3] = r23 * sinpif(h3);
}

// exact-fp32 16x16 MFMA step (k = 4)
__device__ __forceinline__ f32x4 mfma16(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

__device__ __forceinline__ float silu_f(float z) { return z / (1.f + expf(-z)); }
__device__ __forceinline__ float gelu_f(float x) { return 0.5f * x * (1.f + erff(x * 0.70710678118654752f)); }

// wave64 fp64 sum by xor butterflies (all lanes get the total)
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
