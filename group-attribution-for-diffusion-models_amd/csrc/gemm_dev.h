// Device-side building blocks of the fp32 contraction kernels of gemm_f32.hip, winograd.hip and wino4_fused.hip (gfx950 only):
// launch-argument struct, tile slots and loaders, the XOR-swizzled KC tile image and its fragment reads, the K step, the
// epilogue; and the declarations the planner shares with the Winograd launchers.  The Winograd device pieces are wino_dev.h's;
// the LDS-DMA issue, the waits and the zero block are gad_dev.h's.
#pragma once
#include "gad_dev.h"

namespace gadk {

constexpr int BK = 32;
constexpr int NTHREADS = 256;

// physical float offset of logical 16-B chunk q (0..7) of KC-tile row r
__device__ __forceinline__ int kc_off(int r, int q) { return r * BK + ((q ^ ((r >> 1) & 7)) << 2); }

// division by a launch-invariant divisor: q = (mulhi(n, mul) + n) >> shift, exact for 0 <= n < 2^31
struct FastDiv {
  unsigned mul, shift;
  __device__ __forceinline__ int div(int n) const { return (int)((__umulhi((unsigned)n, mul) + (unsigned)n) >> shift); }
};

struct DevArgs {
  FastDiv fdC, fdKW, fdHoWo, fdWo, fdRpg, fdTaps;
  int kperm, taps;   // kperm: K steps visit (channel chunk, tap) instead of (tap, channel chunk)
  const float* A;
  const float* B;
  float* C;
  const unsigned short* Bh;   // bf16 copy of B ([N][ldb], k contiguous): bf16 patch conv streams it by LDS-DMA
  const float* A2;   // two-source conv gather (virtual channel concat): channels >= a_split come from A2
  int a_split, ldx2;
  // K-concatenated dense operands (fused LoRA side path): for k >= k_split the products read Ak2 / Bk2 at k - k_split
  const float* Ak2;
  const float* Bk2;
  int lda2, ldb2, k_split;
  int M, N, K;
  int lda, ldb, ldc;
  int batch_inner;
  long sA0, sA1, sB0, sB1, sC0, sC1;
  gad_conv_geom g;
  float alpha;
  const float* bias;
  const float* rowadd;
  int rows_per_group, ld_rowadd;
  const float* residual;
  int ldr;
  float* ws;
  int tiles_m, tiles_n, splitk, ktiles_per_split;
  int epi_vec;       // the output (and bias / rowadd / residual / workspace) can be written / read as aligned float4
};

__device__ __forceinline__ f32x4 ldg4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ f32x4 zero4() { return f32x4{0.f, 0.f, 0.f, 0.f}; }
__device__ __forceinline__ f32x4 keep_if(f32x4 v, bool ok) { return ok ? v : zero4(); }

// ------------------------------------------------------------------------------------
// Tile loaders.  Each thread owns NS float4 slots of the tile.
//   load(k0, v, mask): issue the global loads of the K step starting at k0.  Loads are
//     UNCONDITIONAL (an invalid slot reads the tensor's base address) so that all of a
//     thread's loads are in flight together behind the MFMAs of the current step;
//     `mask` bit i says whether slot i is real data.
//   store(lds, v, mask): zero the invalid slots and write the tile into LDS.
// KC-type: slot i = (row (tid>>3)+32 i, float4 column tid&7)
// MC-type: slot i = (k row tid/F4 + (256/F4) i, float4 column tid%F4),  F4 = ROWS/4
// ------------------------------------------------------------------------------------
// the wave's index as a SCALAR: LDS-DMA destinations (M0) derived from it need no per-launch v_readfirstlane in the K loop
__device__ __forceinline__ int wave_id() { return __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }

template <int ROWS>
struct KCSlots {
  static constexpr int NS = ROWS / 32;
  __device__ static int row(int i) { return (threadIdx.x >> 3) + 32 * i; }
  // logical float4 column (k chunk) this lane supplies for its row: the lane's LDS position is fixed by
  // the DMA (physical chunk = lane & 7), so the swizzle is applied to what it loads
  // (row(i) >> 1) & 7 == (tid >> 4) & 7 for every slot i, so the column is slot independent
  __device__ static int kq4() { return ((threadIdx.x & 7) ^ ((threadIdx.x >> 4) & 7)) * 4; }
  __device__ static float* dma_dst(float* tile, int i) { return tile + (wave_id() * 8 + 32 * i) * BK; }
  __device__ static void store(float* lds, const f32x4* v, unsigned mask) {   // register path (VEC == 1)
#pragma unroll
    for (int i = 0; i < NS; ++i)
      *reinterpret_cast<f32x4*>(lds + row(i) * BK + (threadIdx.x & 7) * 4) = keep_if(v[i], (mask >> i) & 1u);
  }
};
template <int ROWS>
struct MCSlots {
  static constexpr int NS = ROWS / 32;
  static constexpr int F4 = ROWS / 4;
  static constexpr int KSTEP = NTHREADS / F4;
  __device__ static int krow(int i) { return threadIdx.x / F4 + KSTEP * i; }
  __device__ static int rq4() { return (threadIdx.x % F4) * 4; }
  __device__ static float* dma_dst(float* tile, int i) { return tile + (wave_id() * (KSTEP / 4) + KSTEP * i) * ROWS; }
  __device__ static void store(float* lds, const f32x4* v, unsigned mask) {   // register path (VEC == 1)
#pragma unroll
    for (int i = 0; i < NS; ++i)
      *reinterpret_cast<f32x4*>(lds + krow(i) * ROWS + rq4()) = keep_if(v[i], (mask >> i) & 1u);
  }
};

// Loader protocol: prep(k0) once per K step (shared decode), then per slot i either
//   src(i)            -> per-lane source address of the float4 (or the zero block)   [VEC == 4, LDS-DMA]
//   slot(i, v, mask)  -> register-staged scalar gather of the 4 floats               [VEC == 1]
// both called from between MFMA groups so the address arithmetic sits in the MFMA shadow.
// branch-free source select: offsets are always computed (possibly from out-of-range coordinates), masked
// to 0 when invalid and added to either the tensor base or the zero block
__device__ __forceinline__ const float* sel_src(const float* base, long off, bool ok) {
  const float* b = ok ? base : g_zero_block.f32;
  return b + (off & -(long)ok);
}

constexpr int EPI_LD = 40;                       // scratch row stride in floats
constexpr int EPI_WAVE = 32 * EPI_LD;            // floats of scratch per wave (5 KB; 20 KB per workgroup)

// ------------------------------------------------------------------------------------
// Fragment reads.  K step of 32 = 4 groups of 8; in group g, MFMA step j (0..3) feeds
// lane half h with k = 8g + 4h + j  (so a KC tile is read as one b128 per group).
// ------------------------------------------------------------------------------------
template <bool KC, int ROWS>
__device__ __forceinline__ f32x4 read_frag(const float* lds, int row, int g, int h) {
  if (KC) {
    return *reinterpret_cast<const f32x4*>(lds + kc_off(row, 2 * g + h));
  } else {
    const float* p = lds + (8 * g + 4 * h) * ROWS + row;
    return f32x4{p[0], p[ROWS], p[2 * ROWS], p[3 * ROWS]};
  }
}

// ------------------------------------------------------------------------------------
// Epilogue shared by every contraction kernel: the wave block's accumulators (C/D map: col = lane & 31,
// row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)) go to C with alpha, bias[n], rowadd[m / rows_per_group][n] and
// residual[m][n] fused - or, for a split of a split-K launch (direct = false), raw to the workspace slab.
//
// The C/D map gives a lane ONE column and 16 rows, so stores straight from the accumulators are 64 dword wave-stores per
// 32 x 128 block, and the epilogue's time is the count of those instructions (measured on the 36-step 3x3 tiles:
// 124.7 TF/s as is, 134.8 without the epilogue, 133.4 with the same bytes as dwordx4 stores;
// profiles/r02_resident_workgroups_experiment.txt).  So each 32 x 32 block is transposed through a wave-private
// LDS scratch (the operand tiles are dead after the last K step's barrier): 16 ds_write_b32 at a 40-float row stride
// (rows r and r + 4 of the two lane halves land on disjoint bank halves), 4 ds_read_b128 giving a lane 4 consecutive
// columns of one row, and 4 dwordx4 stores of 8 rows x 128 B each; bias / rowadd / residual are read as float4 too.
// Per element the arithmetic and its order are unchanged (bit-identical to the scalar form, which remains for outputs
// that cannot take aligned float4: N % 4 != 0, odd leading dimensions).
// ------------------------------------------------------------------------------------

template <int TM, int TN, int BM, int BN, int WM = 2, int WN = 2>
__device__ __forceinline__ void store_block(const DevArgs& p, const f32x16 (&acc)[TM][TN], int row0, int col0, int wm, int wn,
                                            int h, int l31, float* C, int ldc, const float* R, bool direct,
                                            float* scratch = nullptr) {
  if (scratch != nullptr && p.epi_vec) {
    const int lane = l31 + 32 * h;
    const int rr = lane >> 3, c4 = (lane & 7) * 4;
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int n = col0 + wn * (BN / WN) + j * 32 + c4;
      const bool n_ok = n < p.N;                 // N % 4 == 0: the float4 is all inside or all outside
      float b0 = 0.f, b1 = 0.f, b2 = 0.f, b3 = 0.f;
      if (direct && p.bias && n_ok) {
        const f32x4 t = ldg4(p.bias + n);
        b0 = t[0]; b1 = t[1]; b2 = t[2]; b3 = t[3];
      }
#pragma unroll
      for (int i = 0; i < TM; ++i) {
#pragma unroll
        for (int e = 0; e < 16; ++e) scratch[((e & 3) + 8 * (e >> 2) + 4 * h) * EPI_LD + l31] = acc[i][j][e];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int r = rr + 8 * q;
          f32x4 v = *reinterpret_cast<const f32x4*>(scratch + r * EPI_LD + c4);
          const int m = row0 + wm * (BM / WM) + i * 32 + r;
          if (m >= p.M || !n_ok) continue;
          if (direct) {
            v = f32x4{__builtin_fmaf(v[0], p.alpha, b0), __builtin_fmaf(v[1], p.alpha, b1), __builtin_fmaf(v[2], p.alpha, b2),
                      __builtin_fmaf(v[3], p.alpha, b3)};
            if (p.rowadd) v += ldg4(p.rowadd + (long)p.fdRpg.div(m) * p.ld_rowadd + n);
            if (R) v += ldg4(R + (long)m * p.ldr + n);
          }
          *reinterpret_cast<f32x4*>(C + (long)m * ldc + n) = v;
        }
      }
    }
    return;
  }
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    int n = col0 + wn * (BN / WN) + j * 32 + l31;
    if (n >= p.N) continue;
    float bias = (direct && p.bias) ? p.bias[n] : 0.f;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        int m = row0 + wm * (BM / WM) + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
        if (m >= p.M) continue;
        float v = acc[i][j][e];
        if (direct) {
          v = __builtin_fmaf(v, p.alpha, bias);
          if (p.rowadd) v += p.rowadd[(long)p.fdRpg.div(m) * p.ld_rowadd + n];
          if (R) v += R[(long)m * p.ldr + n];
        }
        C[(long)m * ldc + n] = v;
      }
    }
  }
}

// ------------------------------------------------------------------------------------
// One K step of a (BM x BN) block on LDS tiles la / lb = 16 "pieces" of TM*TN MFMAs (4 fragment groups x 4 MFMA steps).
// stage(piece) is the caller's staging of the NEXT step into the other buffer, issued one slot per piece from the first
// pieces on and pinned there by sched_barrier so its address VALU runs in the shadow of the 64-cycle MFMAs; the fragments
// of group g+1 are read during group g.
// ------------------------------------------------------------------------------------
template <bool KCA, bool KCB, int BM, int BN, class Stage>
__device__ __forceinline__ void mfma_kstep(const float* la, const float* lb, f32x16 (&acc)[BM / 64][BN / 64], int wm, int wn, int h,
                                           int l31, Stage&& stage) {
  constexpr int TM = BM / 64, TN = BN / 64;
  f32x4 fa[2][TM], fb[2][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i) fa[0][i] = read_frag<KCA, BM>(la, wm * (BM / 2) + i * 32 + l31, 0, h);
#pragma unroll
  for (int j = 0; j < TN; ++j) fb[0][j] = read_frag<KCB, BN>(lb, wn * (BN / 2) + j * 32 + l31, 0, h);
#pragma unroll
  for (int g = 0; g < 4; ++g) {
#pragma unroll
    for (int s = 0; s < 4; ++s) {
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[g & 1][i][s], fb[g & 1][j][s], acc[i][j], 0, 0, 0);
      stage(g * 4 + s);
      if (s == 1 && g < 3) {   // prefetch the next group's fragments into the other register set
#pragma unroll
        for (int i = 0; i < TM; ++i) fa[(g + 1) & 1][i] = read_frag<KCA, BM>(la, wm * (BM / 2) + i * 32 + l31, g + 1, h);
#pragma unroll
        for (int j = 0; j < TN; ++j) fb[(g + 1) & 1][j] = read_frag<KCB, BN>(lb, wn * (BN / 2) + j * 32 + l31, g + 1, h);
      }
      // within the piece: alternate 1 MFMA with <= 7 VALU so the staging arithmetic never holds back
      // the next MFMA by more than its 64-cycle shadow
#pragma unroll
      for (int q = 0; q < TM * TN; ++q) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x002, 7, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  }
}

// ------------------------------------------------------------------------------------
// Host side of the Winograd routes, shared by the planner (gemm_f32.hip) and the launchers (winograd.hip, wino4_fused.hip).
// ------------------------------------------------------------------------------------
inline FastDiv make_fastdiv(unsigned d) {
  FastDiv f;
  if (d == 0) d = 1;
  unsigned l = 0;
  while ((1ull << l) < d) ++l;
  f.shift = l;
  f.mul = (unsigned)((((1ull << l) - d) << 32) / d + 1);
  if (d == 1) f.mul = 0;
  return f;
}

constexpr int GAD_GEMM_INTERNAL_WINO4 = 1 << 30;   // set by gad_gemm on its own batched sub-launches (names the kernel instance apart)
struct WinoPlan {
  int f;                     // 2: F(2x2,3x3) fused kernels; 4: F(4x4,3x3)
  int fused4;                // f = 4: 0 = 36 batched products on the generic engine + output kernel, 1 = the six-position product kernel
                             // (24 half-transformed panels) + output kernel, 2 = wino4_fused_kernel (products and the whole output
                             // transform in one launch: no product ever reaches memory)
  int bm, bn, tiles_m, tiles_n;
  long T;                    // tiles (2x2 or 4x4 output pixels each)
  int64_t bytes;             // scratch: V (f = 2), V + M (f = 4)
};
struct WinoWgradPlan {
  long T;
  int64_t wy_bytes, v_bytes, du_bytes, bytes;
};

// ---- sub-launch arguments: the size queries and the launches build them here, once ----
// the 36 batched products of a Winograd form, C[pos] = A[pos] B[pos] (pos-major panels, no epilogue), as one launch of the
// generic engine on its own plan (tile shapes measured within 4 % of each other here)
inline gad_gemm_args products36(const gad_gemm_args* a, const float* A, const float* B, float* C, int am, int bm, int M, int N, int K) {
  gad_gemm_args sub = *a;
  sub.A = A; sub.B = B; sub.C = C;
  sub.a_mode = am; sub.b_mode = bm;
  sub.M = M; sub.N = N; sub.K = K;
  sub.lda = am == GAD_A_MC ? M : K; sub.ldb = bm == GAD_B_MC ? N : K; sub.ldc = N;
  sub.batch = 36; sub.batch_inner = 1;
  sub.strideA0 = (int64_t)M * K; sub.strideB0 = (int64_t)N * K; sub.strideC0 = (int64_t)M * N;
  sub.strideA1 = sub.strideB1 = sub.strideC1 = 0;
  sub.tile_hint = 0; sub.splitk_hint = 0;
  sub.flags = GAD_GEMM_INTERNAL_WINO4;
  sub.B_wino = nullptr; sub.B_wino4 = nullptr; sub.wino_ws = nullptr; sub.wino_ws_bytes = 0;
  sub.A2 = nullptr;
  return sub;
}
// weight gradient: dU[pos] = Wy[pos]^T V[pos]
inline gad_gemm_args wino_wgrad_products_args(const gad_gemm_args* a, const WinoWgradPlan& wq, float* Wy, float* V, float* dU) {
  return products36(a, Wy, V, dU, GAD_A_MC, GAD_B_MC, a->M, a->g.C, (int)wq.T);
}
// three-launch F(4x4) forward: M[pos] = V[pos] U[pos]^T, then the output transform applies the epilogue
inline gad_gemm_args wino4_products_args(const gad_gemm_args* a, const WinoPlan& wp, float* V, float* Mb) {
  gad_gemm_args sub = products36(a, V, a->B_wino4, Mb, GAD_A_KC, GAD_B_KC, (int)wp.T, a->N, a->g.C);
  sub.alpha = 1.f; sub.bias = nullptr; sub.rowadd = nullptr; sub.residual = nullptr;
  return sub;
}

// winograd.hip: a = the route's canonical arguments, d = their dev_args
int launch_wino(const gad_gemm_args* a, const WinoPlan& wp, const DevArgs& d, void* stream);
int launch_wino_wgrad(const gad_gemm_args* a, const WinoWgradPlan& wq, void* stream);
// wino4_fused.hip: all 36 products + the output transform, one launch
void launch_wino4_fused(const DevArgs& w, int bm, hipStream_t st);

}  // namespace gadk
