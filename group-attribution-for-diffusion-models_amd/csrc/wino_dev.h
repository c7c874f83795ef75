// Device-side pieces of the Winograd routes (gfx950), each written once for winograd.hip, wino4_fused.hip and norm.hip: the
// transform matrices of F(2x2, 3x3) and F(4x4, 3x3), the transform kernels' arguments and tile decode, the tile-to-pixel map
// of the fused epilogues, and the k-contiguous LDS-DMA loader of the product kernels.
// Standard points (Lavin & Gray 2016).  F(2x2): {0, +-1, inf}
//   B^T = [1 0 -1 0; 0 1 1 0; 0 -1 1 0; 0 1 0 -1],   G = [1 0 0; .5 .5 .5; .5 -.5 .5; 0 0 1],   A^T = [1 1 1 0; 0 1 -1 -1]
// F(4x4): {0, +-1, +-2, inf}
//   B^T = [4 0 -5 0 1 0; 0 -4 -4 1 1 0; 0 4 -4 -1 1 0; 0 -2 -1 2 1 0; 0 2 -1 -2 1 0; 0 4 0 -5 0 1]
//   G   = [1/4 0 0; -1/6 -1/6 -1/6; -1/6 1/6 -1/6; 1/24 1/12 1/6; 1/24 -1/12 1/6; 0 0 1]
//   A^T = [1 1 1 1 1 0; 0 1 -1 2 -2 0; 0 1 1 4 4 0; 0 1 -1 8 -8 1]
#pragma once
#include "gemm_dev.h"

namespace gadk {

// ---- F(2x2, 3x3) ----
__device__ __forceinline__ void wino2_bt(const f32x4 (&d)[4], f32x4 (&t)[4]) {      // B^T d
  t[0] = d[0] - d[2];
  t[1] = d[1] + d[2];
  t[2] = d[2] - d[1];
  t[3] = d[1] - d[3];
}
// column nu of A^T: [1 0], [1 1], [1 -1], [0 -1]
__device__ __forceinline__ void wino2_at_col(int nu, float (&w)[2]) {
  w[0] = nu < 3 ? 1.f : 0.f;
  w[1] = nu == 0 ? 0.f : (nu == 1 ? 1.f : -1.f);
}

// ---- F(4x4, 3x3) ----
__device__ __forceinline__ void wino4_bt(const f32x4 (&d)[6], f32x4 (&t)[6]) {      // B^T d: one direction of the input transform
  t[0] = 4.f * d[0] - 5.f * d[2] + d[4];
  t[1] = -4.f * (d[1] + d[2]) + d[3] + d[4];
  t[2] = 4.f * (d[1] - d[2]) - d[3] + d[4];
  t[3] = 2.f * (d[3] - d[1]) - d[2] + d[4];
  t[4] = 2.f * (d[1] - d[3]) - d[2] + d[4];
  t[5] = 4.f * d[1] - 5.f * d[3] + d[5];
}
__device__ __forceinline__ void wino4_at(const f32x4 (&m)[6], f32x4 (&y)[4]) {      // A^T m: one direction of the output transform
  const f32x4 s12 = m[1] + m[2], d12 = m[1] - m[2], s34 = m[3] + m[4], d34 = m[3] - m[4];
  y[0] = m[0] + s12 + s34;
  y[1] = d12 + 2.f * d34;
  y[2] = s12 + 4.f * s34;
  y[3] = d12 + 8.f * d34 + m[5];
}
__device__ __forceinline__ void wino4_a(const f32x4 (&d)[4], f32x4 (&t)[6]) {       // A d (weight gradient: the output-gradient tiles)
  const f32x4 s02 = d[0] + d[2], s13 = d[1] + d[3], a = d[0] + 4.f * d[2], b = 2.f * d[1] + 8.f * d[3];
  t[0] = d[0];
  t[1] = s02 + s13;
  t[2] = s02 - s13;
  t[3] = a + b;
  t[4] = a - b;
  t[5] = d[3];
}
__device__ __forceinline__ void wino4_g(float a, float b, float c, float (&o)[6]) {   // G [a b c]^T
  o[0] = 0.25f * a;
  o[1] = (-1.f / 6.f) * (a + b + c);
  o[2] = (-1.f / 6.f) * (a - b + c);
  o[3] = (1.f / 24.f) * a + (1.f / 12.f) * b + (1.f / 6.f) * c;
  o[4] = (1.f / 24.f) * a - (1.f / 12.f) * b + (1.f / 6.f) * c;
  o[5] = c;
}
__device__ __forceinline__ void wino4_gt(const f32x4 (&m)[6], f32x4 (&o)[3]) {      // G^T m (weight gradient: dU -> dW)
  const f32x4 s12 = m[1] + m[2], d21 = m[2] - m[1], s34 = m[3] + m[4], d34 = m[3] - m[4];
  o[0] = 0.25f * m[0] - (1.f / 6.f) * s12 + (1.f / 24.f) * s34;
  o[1] = (1.f / 6.f) * d21 + (1.f / 12.f) * d34;
  o[2] = (1.f / 6.f) * (s34 - s12) + m[5];
}
// column nu of A^T: [1 0 0 0], [1 1 1 1], [1 -1 1 -1], [1 2 4 8], [1 -2 4 -8], [0 0 0 1].  Scalar selects on purpose: the
// product kernels fold with a position that is a loop variable, and their schedules depend on this form.
__device__ __forceinline__ void wino4_at_col(int nu, float (&w)[4]) {
  const float sg = (nu == 2 || nu == 4) ? -1.f : 1.f, two = nu >= 3 ? 2.f : 1.f;
  w[0] = nu == 5 ? 0.f : 1.f;
  w[1] = (nu == 0 || nu == 5) ? 0.f : sg * two;
  w[2] = (nu == 0 || nu == 5) ? 0.f : two * two;
  w[3] = nu == 0 ? 0.f : (nu == 5 ? 1.f : sg * two * two * two);
}

// ---- transform kernels: one thread per (tile, channel quad) ----
struct WinoIn {
  const float* x;
  float* V;
  int H, W, C, ldx, up;      // source map H x W (before the fused nearest-2x upsample when up = 1), C channels
  int TH, TW;                // tiles per image = (He / F) x (We / F)
  long T;                    // B * TH * TW
};

struct WinoOut {
  const float* Mb;           // [36][T][N]
  float* y;
  const float* bias;
  const float* rowadd;
  const float* residual;
  int N, ldc, ldr, ld_rowadd, Ho, Wo, TH, TW;
  long T;
  float alpha;
};

// item idx of a transform launch (one thread per tile and channel quad, C4 quads per tile) -> tile, first channel c of the quad,
// image n, tile row ty, tile column tx
struct WinoTile {
  long tile;
  int c, n, ty, tx;
};
__device__ __forceinline__ long wino_item() { return (long)blockIdx.x * 256 + threadIdx.x; }
__device__ __forceinline__ WinoTile wino_tile(long idx, int C4, int TH, int TW) {
  WinoTile t;
  t.tile = idx / C4;
  t.c = (int)(idx - t.tile * C4) * 4;
  const int per = TH * TW;
  t.n = (int)(t.tile / per);
  const int r = (int)(t.tile - (long)t.n * per);
  t.ty = r / TW;
  t.tx = r - t.ty * TW;
  return t;
}

// tile m of a product kernel -> its image and the first pixel of its F x F output block (p.M counts tiles; p.fdHoWo / p.fdWo
// divide by the tiles per image / per tile row)
template <int F>
__device__ __forceinline__ long tile_pixel0(const DevArgs& p, int m, int& img) {
  constexpr int SH = F == 2 ? 1 : 2;
  const int tiles_img = (p.g.Ho >> SH) * (p.g.Wo >> SH), TW = p.g.Wo >> SH;
  img = p.fdHoWo.div(m);
  const int rem = m - img * tiles_img;
  const int ty = p.fdWo.div(rem), tx = rem - ty * TW;
  return ((long)img * p.g.Ho + F * ty) * p.g.Wo + F * tx;
}

// ---- product kernels ----
// dense [row][k] rows by LDS-DMA for a workgroup of NTH threads, with a 64-bit step offset (position x panel stride + k): slot i of
// a thread = row (tid >> 3) + (NTH / 8) i, 16-byte chunk (tid & 7) swizzled by the row (KCSlots' image); rows beyond the operand
// clamp to the last one (they feed outputs the epilogue never stores)
template <int ROWS, int NTH = NTHREADS>
struct WinoKC {
  static constexpr int RPS = NTH / 8, NS = ROWS / RPS;
  static_assert(ROWS % RPS == 0, "whole slots");
  const float* ptr[NS];
  long off;
  __device__ void init(const float* b, int ld, int row0, int nrows) {
#pragma unroll
    for (int i = 0; i < NS; ++i) {
      int r = row0 + (int)(threadIdx.x >> 3) + RPS * i;
      r = r < nrows ? r : nrows - 1;
      ptr[i] = b + (long)r * ld + ((threadIdx.x & 7) ^ ((threadIdx.x >> 4) & 7)) * 4;
    }
    off = 0;
  }
  __device__ __forceinline__ const float* src(int i) const { return ptr[i] + off; }
  __device__ static float* dma_dst(float* tile, int i) { return tile + (wave_id() * 8 + RPS * i) * BK; }
};

}  // namespace gadk
