// Winograd routes of the fp32 3x3 / stride 1 / pad 1 convolution on gfx950 (MI355X): the transform kernels of F(2x2, 3x3) and
// F(4x4, 3x3), the product kernels that fold the output transform in, the weight-gradient transforms, and the launchers of both
// routes.  gemm_f32.hip plans (use_wino, use_wino_wgrad, route_of) and calls launch_wino / launch_wino_wgrad; the one-launch
// F(4x4) form is wino4_fused.hip (its own compiler flag); the matrices and the shared device pieces are wino_dev.h.
//
// F(2x2, 3x3): 16 multiplies per 2x2 output tile and channel pair instead of 36 (2.25x fewer MFMA FLOPs), fp32 throughout.
//   y_tile = A^T [ sum_c U[.,.][co][c] (.) V[.,.][tile][c] ] A,   U = G w G^T (per weight version, wino_weights_kernel),
//   V = B^T d B (per launch, wino_input_kernel).
// wino_gemm_kernel runs the 16 per-position products [tiles x Cin] x [Cin x Cout] of one (64 tiles x 128 channels) or
// (128 x 64) block back to back as ONE K loop of 16 Cin/32 steps on the lean dense loaders (V and U are k-contiguous
// rows: LDS-DMA, no masks); after the last step of a position the 32-register product block is folded into the four
// output-pixel accumulators with the position's A^T (x) A^T coefficient (+1 / 0 / -1: exact), so M = U (.) V never
// exists in memory, and the shared float4 epilogue (bias, time-embedding row, residual) writes the four pixels of
// every tile.  Transforms add a rounding per add (the input transform has unit coefficients, the weight transform
// halves): the result differs from the direct kernels' by fp32 reassociation noise of a few ulp of the accumulated
// magnitude, not bit for bit.
//
// F(4x4, 3x3): 36 multiplies per 4x4 output tile and channel pair instead of 144 (4x fewer MFMA FLOPs) and a transformed input
// of only 2.25x the input.  Sixteen output-pixel accumulator sets do not fit a wave, so the element-wise products go through
// memory: wino4_input_kernel (V = B^T d B, 6x6 patches), then either the generic engine as ONE batched launch of 36
// [tiles x Cin] x [Cin x Cout] products (M [36][tiles][Cout]) or wino4_gemm_kernel (six positions per block, the nu direction
// of the output transform folded: Mh [24][tiles][Cout]), then wino4_output_kernel (y = A^T M A + the fused epilogue).
// fp32 throughout; the larger transform coefficients cost about a decimal digit against the direct kernels (measured
// max error 4e-6 of the output scale vs 4e-7), still an order of magnitude inside the contraction tolerance of the tests.
//
// Weight gradient of the same convolutions in F(4x4, 3x3) form (the transposed algorithm):
//   dW = G^T [ sum_tiles (A dy A^T) (.) (B^T x B) ] G        per (co, ci)
// wino4_dy_kernel transforms the 4x4 output-gradient tiles (A = (A^T)^T, 6 x 4), wino4_input_kernel the 6x6 input patches as
// in the forward pass, the generic engine runs the 36 products [Cout x tiles] x [tiles x Cin] (K = tiles: long, split) as one
// batched launch, wino4_dw_kernel applies G^T . G and writes the [Cout][3][3][Cin] gradient.
#include "gemm_dev.h"
#include "wino_dev.h"

using namespace gadk;

namespace {

// ---- input-side transforms: V[pos][tile][c] = (B^T d B)[pos] ----
// The tile decode (wino_tile's arithmetic) and the masked gather of the (F + 2)^2 patch (pad 1, zeros outside the map, the
// nearest-2x upsample fused) are written out in both kernels: through shared functions hipcc commons the gather's address
// arithmetic differently and reorders the decode, and these two kernels are kept instruction for instruction.
__global__ __launch_bounds__(256) void wino_input_kernel(const WinoIn p) {    // p.TH / p.TW / p.T count 2x2 tiles
  const int C4 = p.C >> 2;
  const long idx = wino_item();
  if (idx >= p.T * C4) return;
  const long tile = idx / C4;
  const int c = (int)(idx - tile * C4) * 4;
  const int per = p.TH * p.TW;
  const int n = (int)(tile / per);
  const int r = (int)(tile - (long)n * per);
  const int ty = r / p.TW, tx = r - ty * p.TW;
  const int He = p.H << p.up, We = p.W << p.up;
  const float* img = p.x + (long)n * p.H * p.W * p.ldx + c;
  f32x4 t[4][4];                                 // t[i][dx] = (B^T d)[i][dx]
#pragma unroll
  for (int dx = 0; dx < 4; ++dx) {
    const int xx = 2 * tx - 1 + dx;
    const bool xok = xx >= 0 && xx < We;
    f32x4 d[4], col[4];
#pragma unroll
    for (int dy = 0; dy < 4; ++dy) {
      const int yy = 2 * ty - 1 + dy;
      const bool ok = xok && yy >= 0 && yy < He;
      d[dy] = ok ? ldg4(img + ((long)(yy >> p.up) * p.W + (xx >> p.up)) * p.ldx) : zero4();
    }
    wino2_bt(d, col);
#pragma unroll
    for (int i = 0; i < 4; ++i) t[i][dx] = col[i];
  }
  const long pos_stride = p.T * p.C;
  float* out = p.V + tile * p.C + c;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    // B^T again, each row stored as it is formed: hipcc's schedule follows that order (v = wino2_bt(t[i]) changes the kernel)
    *reinterpret_cast<f32x4*>(out + (long)(4 * i + 0) * pos_stride) = t[i][0] - t[i][2];
    *reinterpret_cast<f32x4*>(out + (long)(4 * i + 1) * pos_stride) = t[i][1] + t[i][2];
    *reinterpret_cast<f32x4*>(out + (long)(4 * i + 2) * pos_stride) = t[i][2] - t[i][1];
    *reinterpret_cast<f32x4*>(out + (long)(4 * i + 3) * pos_stride) = t[i][1] - t[i][3];
  }
}

__global__ __launch_bounds__(256) void wino4_input_kernel(const WinoIn p) {   // p.TH / p.TW / p.T count 4x4 tiles
  const int C4 = p.C >> 2;
  const long idx = wino_item();
  if (idx >= p.T * C4) return;
  const long tile = idx / C4;
  const int c = (int)(idx - tile * C4) * 4;
  const int per = p.TH * p.TW;
  const int n = (int)(tile / per);
  const int r = (int)(tile - (long)n * per);
  const int ty = r / p.TW, tx = r - ty * p.TW;
  const int He = p.H << p.up, We = p.W << p.up;
  const float* img = p.x + (long)n * p.H * p.W * p.ldx + c;
  f32x4 t[6][6];                                 // t[i][dx] = (B^T d)[i][dx]
#pragma unroll
  for (int dx = 0; dx < 6; ++dx) {
    const int xx = 4 * tx - 1 + dx;
    const bool xok = xx >= 0 && xx < We;
    f32x4 d[6], col[6];
#pragma unroll
    for (int dy = 0; dy < 6; ++dy) {
      const int yy = 4 * ty - 1 + dy;
      const bool ok = xok && yy >= 0 && yy < He;
      d[dy] = ok ? ldg4(img + ((long)(yy >> p.up) * p.W + (xx >> p.up)) * p.ldx) : zero4();
    }
    wino4_bt(d, col);
#pragma unroll
    for (int i = 0; i < 6; ++i) t[i][dx] = col[i];
  }
  const long pos_stride = p.T * p.C;
  float* out = p.V + tile * p.C + c;
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    f32x4 v[6];
    wino4_bt(t[i], v);
#pragma unroll
    for (int j = 0; j < 6; ++j) *reinterpret_cast<f32x4*>(out + (long)(6 * i + j) * pos_stride) = v[j];
  }
}

// Wy[pos][tile][c] = (A dy A^T)[pos]: p.x = dy [B][H][W][C], p.V = Wy [36][T][C]
__global__ __launch_bounds__(256) void wino4_dy_kernel(const WinoIn p) {
  const int C4 = p.C >> 2;
  const long idx = wino_item();
  if (idx >= p.T * C4) return;
  const WinoTile w = wino_tile(idx, C4, p.TH, p.TW);
  const float* img = p.x + ((long)w.n * p.H * p.W + (long)(4 * w.ty) * p.W + 4 * w.tx) * p.ldx + w.c;
  f32x4 t[6][4];                                 // t[i][dx] = (A d)[i][dx]
#pragma unroll
  for (int dx = 0; dx < 4; ++dx) {
    f32x4 d[4], col[6];
#pragma unroll
    for (int dy = 0; dy < 4; ++dy) d[dy] = ldg4(img + ((long)dy * p.W + dx) * p.ldx);
    wino4_a(d, col);
#pragma unroll
    for (int i = 0; i < 6; ++i) t[i][dx] = col[i];
  }
  const long pos_stride = p.T * p.C;
  float* out = p.V + w.tile * p.C + w.c;
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    f32x4 v[6];
    wino4_a(t[i], v);
#pragma unroll
    for (int j = 0; j < 6; ++j) *reinterpret_cast<f32x4*>(out + (long)(6 * i + j) * pos_stride) = v[j];
  }
}

// ---- weight transforms ----
// U[pos][co][ci] = (G w G^T)[pos] for 32 x 32 (co, ci) tiles of the 3x3 weights listed in `table`
// (rows {src offset, dst offset, Cout, Cin, co0, ci0} in floats; src storage [Cout][3][3][Cin])
__global__ __launch_bounds__(256) void wino_weights_kernel(const float* src, float* dst, const long* table) {
  const long* row = table + 6 * (long)blockIdx.x;
  const long soff = row[0], doff = row[1];
  const int Cout = (int)row[2], Cin = (int)row[3], co0 = (int)row[4], ci0 = (int)row[5];
  const int ci = ci0 + (threadIdx.x & 31);
  if (ci >= Cin) return;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int co = co0 + (threadIdx.x >> 5) + 8 * q;
    if (co >= Cout) continue;
    const float* w = src + soff + (long)co * 9 * Cin + ci;
    float g[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int s = 0; s < 3; ++s) g[r][s] = w[(long)(r * 3 + s) * Cin];
    float gg[4][3];                       // G g, G = [1 0 0; .5 .5 .5; .5 -.5 .5; 0 0 1] written out: through a helper (as wino4_g) hipcc allocates this kernel differently
#pragma unroll
    for (int s = 0; s < 3; ++s) {
      gg[0][s] = g[0][s];
      gg[1][s] = 0.5f * (g[0][s] + g[1][s] + g[2][s]);
      gg[2][s] = 0.5f * (g[0][s] - g[1][s] + g[2][s]);
      gg[3][s] = g[2][s];
    }
    float* u = dst + doff + (long)co * Cin + ci;
    const long ps = (long)Cout * Cin;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      u[(long)(4 * i + 0) * ps] = gg[i][0];
      u[(long)(4 * i + 1) * ps] = 0.5f * (gg[i][0] + gg[i][1] + gg[i][2]);
      u[(long)(4 * i + 2) * ps] = 0.5f * (gg[i][0] - gg[i][1] + gg[i][2]);
      u[(long)(4 * i + 3) * ps] = gg[i][2];
    }
  }
}

// U[36][co][ci] = G w G^T, 32 x 32 (co, ci) tiles as in wino_weights_kernel (dst region of 36 Cout Cin floats per weight)
__global__ __launch_bounds__(256) void wino4_weights_kernel(const float* src, float* dst, const long* table) {
  const long* row = table + 6 * (long)blockIdx.x;
  const long soff = row[0], doff = row[1];
  const int Cout = (int)row[2], Cin = (int)row[3], co0 = (int)row[4], ci0 = (int)row[5];
  const int ci = ci0 + (threadIdx.x & 31);
  if (ci >= Cin) return;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int co = co0 + (threadIdx.x >> 5) + 8 * q;
    if (co >= Cout) continue;
    const float* w = src + soff + (long)co * 9 * Cin + ci;
    float gg[6][3];                               // G g (columns s = 0..2)
#pragma unroll
    for (int sx = 0; sx < 3; ++sx) {
      float o[6];
      wino4_g(w[(long)(0 * 3 + sx) * Cin], w[(long)(1 * 3 + sx) * Cin], w[(long)(2 * 3 + sx) * Cin], o);
#pragma unroll
      for (int i = 0; i < 6; ++i) gg[i][sx] = o[i];
    }
    float* u = dst + doff + (long)co * Cin + ci;
    const long ps = (long)Cout * Cin;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      float o[6];
      wino4_g(gg[i][0], gg[i][1], gg[i][2], o);
#pragma unroll
      for (int j = 0; j < 6; ++j) u[(long)(6 * i + j) * ps] = o[j];
    }
  }
}

// dW[co][r][s][ci] = (G^T dU G)[r][s] from dU [36][Cout][Cin]; one thread per (co, 4 ci)
__global__ __launch_bounds__(256) void wino4_dw_kernel(const float* dU, float* dW, int Cout, int Cin, int ldc) {
  const int C4 = Cin >> 2;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long)Cout * C4) return;
  const int co = (int)(idx / C4), ci = (int)(idx - (long)co * C4) * 4;
  const long ps = (long)Cout * Cin;
  const float* src = dU + (long)co * Cin + ci;
  f32x4 t[3][6];                                 // t[r][nu] = (G^T dU)[r][nu]
#pragma unroll
  for (int nu = 0; nu < 6; ++nu) {
    f32x4 m[6], col[3];
#pragma unroll
    for (int xi = 0; xi < 6; ++xi) m[xi] = ldg4(src + (long)(6 * xi + nu) * ps);
    wino4_gt(m, col);
#pragma unroll
    for (int r = 0; r < 3; ++r) t[r][nu] = col[r];
  }
  float* dst = dW + (long)co * ldc + ci;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    f32x4 o[3];
    wino4_gt(t[r], o);
#pragma unroll
    for (int sx = 0; sx < 3; ++sx) *reinterpret_cast<f32x4*>(dst + (long)(r * 3 + sx) * Cin) = o[sx];
  }
}

// ---- F(4x4) output transform: y = A^T M A + the fused epilogue ----
// HALF: Mb holds the 24 half-transformed panels Mh[4 xi + j] of wino4_gemm_kernel (nu direction already folded)
template <bool HALF>
__global__ __launch_bounds__(256) void wino4_output_kernel(const WinoOut p) {
  const int N4 = p.N >> 2;
  const long idx = wino_item();
  if (idx >= p.T * N4) return;
  const WinoTile w = wino_tile(idx, N4, p.TH, p.TW);
  const int n = w.c, img = w.n;
  const long pos_stride = p.T * p.N;
  const float* src = p.Mb + w.tile * p.N + n;
  f32x4 t[4][HALF ? 4 : 6];                      // t[i][nu] = (A^T M)[i][nu]   (HALF: t[i][j] = y[i][j] already)
#pragma unroll
  for (int nu = 0; nu < (HALF ? 4 : 6); ++nu) {
    f32x4 m[6], col[4];
#pragma unroll
    for (int xi = 0; xi < 6; ++xi) m[xi] = ldg4(src + (long)((HALF ? 4 : 6) * xi + nu) * pos_stride);
    wino4_at(m, col);
#pragma unroll
    for (int i = 0; i < 4; ++i) t[i][nu] = col[i];
  }
  const f32x4 b = p.bias ? ldg4(p.bias + n) : zero4();
  const f32x4 ra = p.rowadd ? ldg4(p.rowadd + (long)img * p.ld_rowadd + n) : zero4();
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    f32x4 y[4];
    if constexpr (HALF) {
#pragma unroll
      for (int j = 0; j < 4; ++j) y[j] = t[i][j];
    } else {
      f32x4 row6[6];
#pragma unroll
      for (int j = 0; j < 6; ++j) row6[j] = t[i][HALF ? 0 : j];
      wino4_at(row6, y);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const long pix = ((long)img * p.Ho + 4 * w.ty + i) * p.Wo + 4 * w.tx + j;
      f32x4 v = f32x4{__builtin_fmaf(y[j][0], p.alpha, b[0]), __builtin_fmaf(y[j][1], p.alpha, b[1]),
                      __builtin_fmaf(y[j][2], p.alpha, b[2]), __builtin_fmaf(y[j][3], p.alpha, b[3])};
      if (p.rowadd) v += ra;
      if (p.residual) v += ldg4(p.residual + pix * p.ldr + n);
      *reinterpret_cast<f32x4*>(p.y + pix * p.ldc + n) = v;
    }
  }
}

// ---- product kernels ----
// one output pixel (di, dj) of every 2x2 tile of the block: p.M counts TILES; same arithmetic order as store_block
template <int TM, int TN, int BM, int BN>
__device__ __forceinline__ void store_block_wino(const DevArgs& p, const f32x16 (&acc)[TM][TN], int row0, int col0, int wm, int wn,
                                                 int h, int l31, int di, int dj, float* scratch) {
  const int lane = l31 + 32 * h;
  const int rr = lane >> 3, c4 = (lane & 7) * 4;
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int n = col0 + wn * (BN / 2) + j * 32 + c4;
    const bool n_ok = n < p.N;
    float b0 = 0.f, b1 = 0.f, b2 = 0.f, b3 = 0.f;
    if (p.bias && n_ok) {
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
        const int m = row0 + wm * (BM / 2) + i * 32 + r;
        if (m >= p.M || !n_ok) continue;
        int img;
        const long pix = tile_pixel0<2>(p, m, img) + (long)di * p.g.Wo + dj;
        v = f32x4{__builtin_fmaf(v[0], p.alpha, b0), __builtin_fmaf(v[1], p.alpha, b1), __builtin_fmaf(v[2], p.alpha, b2),
                  __builtin_fmaf(v[3], p.alpha, b3)};
        if (p.rowadd) v += ldg4(p.rowadd + (long)img * p.ld_rowadd + n);
        if (p.residual) v += ldg4(p.residual + pix * p.ldr + n);
        *reinterpret_cast<f32x4*>(p.C + pix * p.ldc + n) = v;
      }
    }
  }
}

// The products of one (BM tiles x BN channels) block for NPOS positions back to back as one K loop on the engine's K step, each
// finished product block folded into four accumulators Y:
//   F = 2: all 16 positions; Y[2 di + dj] += (A^T (x) A^T)[(di, dj)][pos] acc, the four output pixels of the tile, stored with the
//          fused epilogue.  p.A = V [16][T][Cin] (p.sA0 = T Cin), p.B = U [16][Cout][Cin] (p.sB0 = Cout Cin), p.M = T tiles,
//          p.N = Cout, p.K = Cin; grid = tiles_m x tiles_n.
//   F = 4: block (xi, tile_m, tile_n) runs the SIX positions M[xi][nu] = V[6 xi + nu] U[6 xi + nu]^T; Y[j] += A^T[j][nu] acc (the
//          output transform's nu direction), stored raw as Mh[4 xi + j][tile][n]: 24 values per tile and channel reach memory
//          instead of 36, one pipeline prologue serves six products.  p.A = V [36][T][Cin], p.B = U [36][Cout][Cin],
//          p.C = Mh [24][T][Cout] (p.sC0 = T Cout); grid = 6 x tiles_m x tiles_n, xi slowest: neighbouring blocks share the V
//          rows / U panel.
// p by value: through a reference hipcc re-reads the arguments after every store of the epilogue (2600 -> 3250 instructions).
template <int F, int BM, int BN>
__device__ __forceinline__ void wino_products(const DevArgs p) {
  constexpr int TM = BM / 64, TN = BN / 64, NPOS = F == 2 ? 16 : 6;
  using AL = WinoKC<BM>;
  using BL = WinoKC<BN>;
  constexpr int A_TILE = BK * BM;
  constexpr int B_TILE = BK * BN;
  __shared__ __attribute__((aligned(16))) float lds[2 * (A_TILE + B_TILE)];

  int t = xcd_remap(blockIdx.x, gridDim.x), xi6 = 0;
  if (F == 4) {
    const int per_xi = p.tiles_m * p.tiles_n;
    xi6 = t / per_xi;
    t -= xi6 * per_xi;
  }
  const int tile_m = t / p.tiles_n, tile_n = t - tile_m * p.tiles_n;
  const int row0 = tile_m * BM, col0 = tile_n * BN;
  const int kc = p.K / BK;                       // K steps per position
  const int nsteps = NPOS * kc;
  const int pos0 = F == 4 ? 6 * xi6 : 0;

  AL al;
  BL bl;
  al.init(p.A, p.lda, row0, p.M);
  bl.init(p.B, p.ldb, col0, p.N);
  al.off = (long)pos0 * p.sA0;
  bl.off = (long)pos0 * p.sB0;

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int wm = wave >> 1, wn = wave & 1, h = lane >> 5, l31 = lane & 31;

  f32x16 acc[TM][TN], Y[4][TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        acc[i][j][e] = 0.f;
#pragma unroll
        for (int q = 0; q < 4; ++q) Y[q][i][j][e] = 0.f;
      }

  auto stage_slot = [&](int piece, float* ta, float* tb) {
    constexpr int NSA = AL::NS, NSB = BL::NS;
    if (piece < NSA) glds16(al.src(piece), AL::dma_dst(ta, piece));
    else if (piece < NSA + NSB) glds16(bl.src(piece - NSA), BL::dma_dst(tb, piece - NSA));
  };
#pragma unroll
  for (int q = 0; q < AL::NS + BL::NS; ++q) stage_slot(q, lds, lds + A_TILE);
  barrier_after_dma();

  int pos = 0, kk = 0;                           // position and K step of the step being multiplied
  for (int s = 0; s < nsteps; ++s) {
    float* cur = lds + (s & 1) * (A_TILE + B_TILE);
    float* nxt = lds + ((s + 1) & 1) * (A_TILE + B_TILE);
    {                                            // offsets of step s + 1 (the step past the end re-reads the last one)
      int pn = pos, kn = kk + 1;
      if (kn == kc) { kn = 0; ++pn; }
      if (pn == NPOS) { pn = NPOS - 1; kn = kc - 1; }
      al.off = (long)(pos0 + pn) * p.sA0 + kn * BK;
      bl.off = (long)(pos0 + pn) * p.sB0 + kn * BK;
    }
    mfma_kstep<true, true, BM, BN>(cur, cur + A_TILE, acc, wm, wn, h, l31, [&](int piece) { stage_slot(piece, nxt, nxt + A_TILE); });
    if (++kk == kc) {                            // position done: fold its product block into the four accumulators
      float w[4];
      if (F == 2) {
        float r[2], c[2];
        wino2_at_col(pos >> 2, r);
        wino2_at_col(pos & 3, c);
        w[0] = r[0] * c[0]; w[1] = r[0] * c[1]; w[2] = r[1] * c[0]; w[3] = r[1] * c[1];
      } else {
        wino4_at_col(pos, w);
      }
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
          for (int e = 0; e < 16; ++e) {
            const float a = acc[i][j][e];
            Y[0][i][j][e] = __builtin_fmaf(w[0], a, Y[0][i][j][e]);
            Y[1][i][j][e] = __builtin_fmaf(w[1], a, Y[1][i][j][e]);
            Y[2][i][j][e] = __builtin_fmaf(w[2], a, Y[2][i][j][e]);
            Y[3][i][j][e] = __builtin_fmaf(w[3], a, Y[3][i][j][e]);
            acc[i][j][e] = 0.f;
          }
      kk = 0;
      ++pos;
    }
    barrier_after_dma();
  }

  float* scratch = lds + (tid >> 6) * EPI_WAVE;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    if (F == 2) store_block_wino<TM, TN, BM, BN>(p, Y[q], row0, col0, wm, wn, h, l31, q >> 1, q & 1, scratch);
    else store_block<TM, TN, BM, BN>(p, Y[q], row0, col0, wm, wn, h, l31, p.C + (long)(4 * xi6 + q) * p.sC0, p.N, nullptr, false, scratch);
  }
}
template <int BM, int BN>
__global__ __launch_bounds__(NTHREADS, 2) void wino_gemm_kernel(const DevArgs p) {
  wino_products<2, BM, BN>(p);
}
template <int BM, int BN>
__global__ __launch_bounds__(NTHREADS, 2) void wino4_gemm_kernel(const DevArgs p) {
  wino_products<4, BM, BN>(p);
}

}  // namespace

extern "C" int gad_wino_weights(const float* src, float* dst, const int64_t* table, int64_t n_tiles, void* stream) {
  GAD_CHECK(src && dst && table && n_tiles > 0 && n_tiles < (1L << 31), "gad_wino_weights: bad arguments");
  static_assert(sizeof(long) == sizeof(int64_t), "table rows are 64-bit");
  hipLaunchKernelGGL(wino_weights_kernel, dim3((unsigned)n_tiles), dim3(256), 0, (hipStream_t)stream, src, dst, (const long*)table);
  GAD_LAUNCH_CHECK("gad_wino_weights");
  return 0;
}

extern "C" int gad_wino4_weights(const float* src, float* dst, const int64_t* table, int64_t n_tiles, void* stream) {
  GAD_CHECK(src && dst && table && n_tiles > 0 && n_tiles < (1L << 31), "gad_wino4_weights: bad arguments");
  hipLaunchKernelGGL(wino4_weights_kernel, dim3((unsigned)n_tiles), dim3(256), 0, (hipStream_t)stream, src, dst, (const long*)table);
  GAD_LAUNCH_CHECK("gad_wino4_weights");
  return 0;
}

namespace gadk {

int launch_wino_wgrad(const gad_gemm_args* a, const WinoWgradPlan& wq, void* stream) {
  const gad_conv_geom& g = a->g;
  hipStream_t st = (hipStream_t)stream;
  GAD_CHECK(a->wino_ws && a->wino_ws_bytes >= wq.bytes && gad_aligned16(a->wino_ws),
            "gad_gemm: Winograd weight-gradient workspace too small or misaligned (%lld < %lld)", (long long)a->wino_ws_bytes, (long long)wq.bytes);
  float* Wy = (float*)a->wino_ws;
  float* V = Wy + wq.wy_bytes / 4;
  float* dU = V + wq.v_bytes / 4;
  // the forward launch of the same convolution already made B^T x B (its V, same geometry => same [36][T][Cin] image): a caller
  // that kept it passes it as B_wino4 with GAD_GEMM_WINO_SKIP_INPUT and the input transform is not run again
  const bool have_v = (a->flags & GAD_GEMM_WINO_SKIP_INPUT) && a->B_wino4 != nullptr;
  if (have_v) {
    GAD_CHECK(gad_aligned16(a->B_wino4), "gad_gemm: the kept Winograd input image (B_wino4 of a weight-gradient launch) must be 16-byte aligned");
    V = const_cast<float*>(a->B_wino4);
  }
  WinoIn wy;                                     // dy [B][Ho][Wo][Cout] -> Wy
  wy.x = a->A; wy.V = Wy;
  wy.H = g.Ho; wy.W = g.Wo; wy.C = a->M; wy.ldx = a->lda; wy.up = 0;
  wy.TH = g.Ho / 4; wy.TW = g.Wo / 4; wy.T = wq.T;
  WinoIn wi;                                     // x -> V, as in the forward pass
  wi.x = a->B; wi.V = V;
  wi.H = g.H; wi.W = g.W; wi.C = g.C; wi.ldx = g.ldx; wi.up = g.upsample ? 1 : 0;
  wi.TH = wy.TH; wi.TW = wy.TW; wi.T = wq.T;
  const long iy = wq.T * (a->M / 4), ix = wq.T * (g.C / 4);
  GAD_CHECK(gad_ceil_div(iy, 256) < (1L << 31) && gad_ceil_div(ix, 256) < (1L << 31), "gad_gemm: Winograd transform grid too large");
  hipLaunchKernelGGL(wino4_dy_kernel, dim3((unsigned)gad_ceil_div(iy, 256)), dim3(256), 0, st, wy);
  if (!have_v) hipLaunchKernelGGL(wino4_input_kernel, dim3((unsigned)gad_ceil_div(ix, 256)), dim3(256), 0, st, wi);
  GAD_LAUNCH_CHECK("gad_gemm(winograd wgrad transforms)");
  const gad_gemm_args sub = wino_wgrad_products_args(a, wq, Wy, V, dU);
  if (const int rc = gad_gemm(&sub, stream)) return rc;
  const long items = (long)a->M * (g.C / 4);
  hipLaunchKernelGGL(wino4_dw_kernel, dim3((unsigned)gad_ceil_div(items, 256)), dim3(256), 0, st, dU, a->C, a->M, g.C, a->ldc);
  GAD_LAUNCH_CHECK("gad_gemm(winograd wgrad output transform)");
  return 0;
}

int launch_wino(const gad_gemm_args* a, const WinoPlan& wp, const DevArgs& d, void* stream) {
  const gad_conv_geom& g = a->g;
  hipStream_t st = (hipStream_t)stream;
  GAD_CHECK(a->wino_ws && a->wino_ws_bytes >= wp.bytes && gad_aligned16(a->wino_ws) && gad_aligned16(wp.f == 2 ? a->B_wino : a->B_wino4),
            "gad_gemm: Winograd workspace too small or misaligned (%lld < %lld)", (long long)a->wino_ws_bytes, (long long)wp.bytes);
  WinoIn wi;
  wi.x = a->A; wi.V = (float*)a->wino_ws;
  wi.H = g.H; wi.W = g.W; wi.C = g.C; wi.ldx = g.ldx; wi.up = g.upsample ? 1 : 0;
  wi.TH = g.Ho / wp.f; wi.TW = g.Wo / wp.f; wi.T = wp.T;
  const long items = wp.T * (g.C / 4);
  GAD_CHECK(gad_ceil_div(items, 256) < (1L << 31), "gad_gemm: Winograd input transform grid too large");
  const bool only_input = (a->flags & GAD_GEMM_WINO_ONLY_INPUT) != 0, skip_input = (a->flags & GAD_GEMM_WINO_SKIP_INPUT) != 0;
  auto products = [&](const float* U) {          // the product kernels of F(2x2) and of the one-launch F(4x4): V x U + output transform
    DevArgs w = d;
    w.A = wi.V; w.B = U;
    w.M = (int)wp.T; w.N = a->N; w.K = g.C;
    w.lda = g.C; w.ldb = g.C;
    w.sA0 = wp.T * (long)g.C; w.sB0 = (long)a->N * g.C;
    w.fdHoWo = make_fastdiv((unsigned)(wi.TH * wi.TW));
    w.fdWo = make_fastdiv((unsigned)wi.TW);
    w.tiles_m = wp.tiles_m; w.tiles_n = wp.tiles_n;
    return w;
  };
  if (wp.f == 4) {
    if (!skip_input) {
      hipLaunchKernelGGL(wino4_input_kernel, dim3((unsigned)gad_ceil_div(items, 256)), dim3(256), 0, st, wi);
      GAD_LAUNCH_CHECK("gad_gemm(winograd F4 input transform)");
    }
    if (only_input) return 0;
    if (wp.fused4 == 2) {                        // products + the whole output transform in one launch
      GAD_CHECK((long)wp.tiles_m * wp.tiles_n < (1L << 31), "gad_gemm: Winograd grid too large");
      launch_wino4_fused(products(a->B_wino4), wp.bm, st);
      GAD_LAUNCH_CHECK("gad_gemm(winograd F4 fused products + output transform)");
      return 0;
    }
    float* Mb = wi.V + 36 * wp.T * (long)g.C;
    WinoOut wo;
    wo.Mb = Mb; wo.y = a->C; wo.bias = a->bias; wo.rowadd = a->rowadd; wo.residual = a->residual;
    wo.N = a->N; wo.ldc = a->ldc; wo.ldr = a->ldr; wo.ld_rowadd = a->ld_rowadd;
    wo.Ho = g.Ho; wo.Wo = g.Wo; wo.TH = wi.TH; wo.TW = wi.TW; wo.T = wp.T; wo.alpha = a->alpha;
    const long oitems = wp.T * (a->N / 4);
    if (wp.fused4 == 1) {
      DevArgs w = d;
      w.A = wi.V; w.B = a->B_wino4; w.C = Mb;
      w.M = (int)wp.T; w.N = a->N; w.K = g.C;
      w.lda = g.C; w.ldb = g.C; w.ldc = a->N;
      w.sA0 = wp.T * (long)g.C; w.sB0 = (long)a->N * g.C; w.sC0 = wp.T * (long)a->N;
      w.tiles_m = wp.tiles_m; w.tiles_n = wp.tiles_n;
      w.splitk = 1; w.bias = nullptr; w.rowadd = nullptr; w.residual = nullptr; w.alpha = 1.f;
      w.epi_vec = 1;                             // Mh is 16-byte aligned scratch, N % 4 == 0
      dim3 grid((unsigned)((long)wp.tiles_m * wp.tiles_n * 6)), block(NTHREADS);
      if (wp.bm == 64) hipLaunchKernelGGL((wino4_gemm_kernel<64, 128>), grid, block, 0, st, w);
      else hipLaunchKernelGGL((wino4_gemm_kernel<128, 64>), grid, block, 0, st, w);
      GAD_LAUNCH_CHECK("gad_gemm(winograd F4 products)");
      hipLaunchKernelGGL(wino4_output_kernel<true>, dim3((unsigned)gad_ceil_div(oitems, 256)), dim3(256), 0, st, wo);
      GAD_LAUNCH_CHECK("gad_gemm(winograd F4 output transform)");
      return 0;
    }
    const gad_gemm_args sub = wino4_products_args(a, wp, wi.V, Mb);
    if (const int rc = gad_gemm(&sub, stream)) return rc;
    hipLaunchKernelGGL(wino4_output_kernel<false>, dim3((unsigned)gad_ceil_div(oitems, 256)), dim3(256), 0, st, wo);
    GAD_LAUNCH_CHECK("gad_gemm(winograd F4 output transform)");
    return 0;
  }
  if (!skip_input) {
    hipLaunchKernelGGL(wino_input_kernel, dim3((unsigned)gad_ceil_div(items, 256)), dim3(256), 0, st, wi);
    GAD_LAUNCH_CHECK("gad_gemm(winograd input transform)");
  }
  if (only_input) return 0;
  const DevArgs w = products(a->B_wino);
  dim3 grid((unsigned)((long)wp.tiles_m * wp.tiles_n)), block(NTHREADS);
  if (wp.bm == 64) hipLaunchKernelGGL((wino_gemm_kernel<64, 128>), grid, block, 0, st, w);
  else hipLaunchKernelGGL((wino_gemm_kernel<128, 64>), grid, block, 0, st, w);
  GAD_LAUNCH_CHECK("gad_gemm(winograd)");
  return 0;
}

}  // namespace gadk
