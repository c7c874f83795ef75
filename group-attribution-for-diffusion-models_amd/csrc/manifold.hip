// Improved precision / recall manifolds (Kynkaanniemi et al.; reference src/attributions/global_scores/precision_recall.py
// compute_kth / calc_pr) on fp16 features, without a distance matrix.
//
//   gad_manifold_radii   kth[i]     = the (k+1)-th smallest d16(F_i, F_j) over all j (i included: kthvalue(nhood_size + 1))
//   gad_manifold_cover   covered[i] = any_j d16(P_i, T_j) <= kth_T[j]
//
// The distance is DEFINED as d2 = max(0, (|a|^2 + |b|^2) - 2 a.b) with the norms and the dot product accumulated in fp32 from the
// exact fp16 values, and d16 = (half) sqrtf(d2), rounded to nearest even.  The build passes no fast-math flag and hipcc's default
// is -fhip-fp32-correctly-rounded-divide-sqrt, so sqrtf is the correctly rounded one (v_sqrt_f32 plus its fma fix-up, fp32
// denormals on): d16 is a function of d2 alone.  Rounding and sqrt are monotonic, so the radii are selected on d2 and rounded once.
//
// One engine, manifold_kernel<COVER>: a workgroup of four waves (2 x 2) owns 128 probe rows and walks its share of the 128-column
// target tiles; per tile the dot products are a 128 x 128 x D contraction on v_mfma_f32_32x32x16_f16 with both operands streamed
// HBM/L2 -> LDS by LDS-DMA (glds16, two 64-deep stage buffers, barrier_after_dma per step - gad_dev.h; the 16-B chunk index
// XOR-swizzled by the row on the DMA's SOURCE address and on the fragment read, as hgemm_kernel of half.hip does).  Rows / columns past the
// end and k >= D are DMA'd from the zero block, never from the matrices; a column past the end gets |b|^2 = +inf, so its d2 is
// +inf and takes part in nothing.
//   radii: each wave passes its 64 x 64 quadrant of d2 through a private LDS patch (aliasing the stage buffers), after which
//          lane r owns probe row r and keeps the 8 smallest d2 it has seen in registers.
//   cover: the comparison happens on the accumulator layout (column on the lane, its 32 rows in registers): one bit per row.
// The target axis is split over gridDim.y; every (split, column half) writes its partial - 8 floats or one byte per row - to
// the workspace and a second kernel merges them in index order.  No atomics: the results are a function of the inputs alone.
#include <hip/hip_fp16.h>
#include <math.h>

#include "gad_dev.h"

namespace {

typedef unsigned short u16;
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

constexpr int BM = 128, BN = 128, BK = 64, NW = 4, NT = NW * 64, TM = 2, TN = 2;
constexpr int RPI = 8;                                   // tile rows per DMA wave-instruction (8 rows x 128 B = 1 KiB)
constexpr int DI = BM / RPI / NW;                        // DMA instructions per wave, operand and K step
constexpr int A_BYTES = BM * BK * 2, STAGE = A_BYTES + BN * BK * 2;
constexpr int ELD = 68;                                  // patch row stride in floats (272 B: 16-byte aligned rows, 4 banks apart)
constexpr int PATCH_BYTES = NW * 64 * ELD * 4;
constexpr int LDS_BYTES = PATCH_BYTES > 2 * STAGE ? PATCH_BYTES : 2 * STAGE;
constexpr int KP = 8;                                    // smallest d2 kept per row and partial (k + 1 <= 8)
constexpr int TARGET_WG = 512;                           // 256 CUs x 2 resident workgroups
constexpr int MT = 256;                                  // threads of the pre-pass and merge kernels
static_assert(BM == BN && DI * RPI * NW == BM, "one dealing of tile rows to DMA instructions for both operands");

struct MDev {
  const u16* P; const u16* T;      // probe rows / target rows (the same matrix for the radii)
  int Np, Nt, D;
  int64_t ldp, ldt;
  const float* na; const float* nb;  // squared norms
  const u16* kth;                  // cover: radii of the targets
  float* part;                     // radii: [parts][Np][KP]
  unsigned char* flags;            // cover: [parts][Np]
  int col_tiles, tiles_per_split;
};

__device__ __forceinline__ float h2f(u16 h) { return __half2float(__ushort_as_half(h)); }
__device__ __forceinline__ u16 f2h(float f) { return __half_as_ushort(__float2half_rn(f)); }

// v into the ascending list of the KP smallest
__device__ __forceinline__ void insert(float (&list)[KP], float v) {
#pragma unroll
  for (int j = 0; j < KP; ++j) {
    const float lo = fminf(list[j], v);
    v = fmaxf(list[j], v);
    list[j] = lo;
  }
}

// |row|^2 in fp32: one wave per row, 8 halves per lane and pass, the lanes' sums folded by the xor butterfly
__global__ __launch_bounds__(MT) void norms_kernel(const u16* __restrict__ F, int N, int D, int64_t ld, float* __restrict__ out) {
  const int row = blockIdx.x * (MT / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= N) return;
  const u16* f = F + (int64_t)row * ld;
  float s = 0.f;
  for (int c = lane * 8; c < D; c += 64 * 8) {
    const f16x8 v = *reinterpret_cast<const f16x8*>(f + c);
#pragma unroll
    for (int j = 0; j < 8; ++j) s = fmaf((float)v[j], (float)v[j], s);
  }
  s = wave_sum(s);
  if (lane == 0) out[row] = s;
}

template <bool COVER>
__global__ __launch_bounds__(NT, 2) void manifold_kernel(const MDev p) {
  extern __shared__ __attribute__((aligned(1024))) unsigned char lds[];
  const int row0 = blockIdx.x * BM, split = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int lrow = lane >> 3, slot = lane & 7;
  const int l31 = lane & 31, h = lane >> 5;
  // DMA instruction ii of an operand covers tile rows [8 ii, 8 ii + 8); wave w issues ii = 4 i + w, so the swizzle (row >> 1) & 7 of
  // row 8 ii + lrow does not depend on i: one source chunk per lane
  const int ch = (slot ^ (((wave * RPI + lrow) >> 1) & 7)) * 8;
  const u16* const zero = g_zero_block.b16;   // the DMA source of everything outside the matrices

  const u16* asrc[DI];
  const u16* bsrc[DI];
#pragma unroll
  for (int i = 0; i < DI; ++i) {
    const int m = row0 + (i * NW + wave) * RPI + lrow;
    asrc[i] = m < p.Np ? p.P + (int64_t)m * p.ldp + ch : nullptr;
  }
  auto stage = [&](int buf, int kk) {
    unsigned char* dst = lds + buf * STAGE + wave * 1024;
    const bool inside = kk + ch < p.D;                  // D % 8 == 0: a chunk is whole or absent
#pragma unroll
    for (int i = 0; i < DI; ++i) {
      const u16* src = inside && asrc[i] ? asrc[i] + kk : zero;
      glds16(src, dst + i * (NW * 1024));
    }
#pragma unroll
    for (int i = 0; i < DI; ++i) {
      const u16* src = inside && bsrc[i] ? bsrc[i] + kk : zero;
      glds16(src, dst + A_BYTES + i * (NW * 1024));
    }
  };

  f32x16 acc[TM][TN];
  const int swl = (l31 >> 1) & 7;
  const int a_base = (wm * TM * 32 + l31) * (BK * 2);
  const int b_base = A_BYTES + (wn * TN * 32 + l31) * (BK * 2);
  auto compute = [&](int buf) {
    const unsigned char* sb = lds + buf * STAGE;
#pragma unroll
    for (int kk = 0; kk < BK / 16; ++kk) {
      const int off = ((2 * kk + h) ^ swl) * 16;
      f16x8 af[TM], bf[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i) af[i] = *reinterpret_cast<const f16x8*>(sb + a_base + i * 32 * BK * 2 + off);
#pragma unroll
      for (int j = 0; j < TN; ++j) bf[j] = *reinterpret_cast<const f16x8*>(sb + b_base + j * 32 * BK * 2 + off);
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[i], bf[j], acc[i][j], 0, 0, 0);
    }
  };

  // an accumulator register e of tile (i, j) is row 32 i + 8 (e >> 2) + 4 h + (e & 3), column 32 j + l31 of the wave's quadrant
  float na[TM * 16];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int m = row0 + wm * 64 + i * 32 + 8 * (e >> 2) + 4 * h + (e & 3);
      na[i * 16 + e] = m < p.Np ? p.na[m] : 0.f;
    }

  float list[KP];
#pragma unroll
  for (int j = 0; j < KP; ++j) list[j] = INFINITY;
  unsigned hit = 0;                                     // cover: bit 16 i + e
  float* patch = reinterpret_cast<float*>(lds) + wave * (64 * ELD);

  const int steps = (p.D + BK - 1) / BK;
  const int ct0 = split * p.tiles_per_split, ct1 = min(p.col_tiles, ct0 + p.tiles_per_split);
  for (int ct = ct0; ct < ct1; ++ct) {
    const int col0 = ct * BN;
#pragma unroll
    for (int i = 0; i < DI; ++i) {
      const int n = col0 + (i * NW + wave) * RPI + lrow;
      bsrc[i] = n < p.Nt ? p.T + (int64_t)n * p.ldt + ch : nullptr;
    }
    float nb[TN], thr[TN];
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int n = col0 + wn * 64 + j * 32 + l31;
      nb[j] = n < p.Nt ? p.nb[n] : INFINITY;            // a column past the end: d2 = +inf
      thr[j] = -1.f;
      if constexpr (COVER) thr[j] = n < p.Nt ? h2f(p.kth[n]) : -1.f;
    }
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    stage(0, 0);
    barrier_after_dma();
    for (int st = 0; st < steps; ++st) {
      if (st + 1 < steps) stage((st + 1) & 1, (st + 1) * BK);
      compute(st & 1);
      barrier_after_dma();                              // the next stage has landed; every wave is past this stage's reads
    }

    if constexpr (COVER) {
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
          for (int e = 0; e < 16; ++e) {
            const float d2 = fmaxf(0.f, (na[i * 16 + e] + nb[j]) - 2.f * acc[i][j][e]);
            const float d16 = h2f(f2h(sqrtf(d2)));     // the fp16-rounded distance (an exact fp32 value)
            hit |= (d16 <= thr[j] ? 1u : 0u) << (16 * i + e);
          }
    } else {
      // the stage buffers are free (last barrier above): the quadrant goes through the wave's patch, row-major
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
          for (int e = 0; e < 16; ++e) {
            const int r = i * 32 + 8 * (e >> 2) + 4 * h + (e & 3);
            patch[r * ELD + j * 32 + l31] = fmaxf(0.f, (na[i * 16 + e] + nb[j]) - 2.f * acc[i][j][e]);
          }
      __builtin_amdgcn_wave_barrier();                  // (the LDS operations of one wave complete in order)
#pragma unroll 4
      for (int c = 0; c < 64; c += 4) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(patch + lane * ELD + c);
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (v[q] < list[KP - 1]) insert(list, v[q]);
      }
      __syncthreads();                                  // the next tile's DMA lands where the other waves' patches are
    }
  }

  const int part = split * 2 + wn;
  if constexpr (COVER) {
    // a row's columns sit on the 32 lanes of a half-wave: OR them, then lane l31 writes the row of bit l31
#pragma unroll
    for (int o = 1; o < 32; o <<= 1) hit |= (unsigned)__shfl_xor((int)hit, o, 64);
    const int m = row0 + wm * 64 + (l31 >> 4) * 32 + 8 * ((l31 & 15) >> 2) + 4 * h + (l31 & 3);
    if (m < p.Np) p.flags[(int64_t)part * p.Np + m] = (unsigned char)((hit >> l31) & 1u);
  } else {
    const int m = row0 + wm * 64 + lane;
    if (m < p.Np) {
      float* dst = p.part + ((int64_t)part * p.Np + m) * KP;
      *reinterpret_cast<f32x4*>(dst) = f32x4{list[0], list[1], list[2], list[3]};
      *reinterpret_cast<f32x4*>(dst + 4) = f32x4{list[4], list[5], list[6], list[7]};
    }
  }
}

// the parts' lists in index order -> the (k+1)-th smallest d2 of the row, rounded once
__global__ __launch_bounds__(MT) void radii_merge_kernel(const float* __restrict__ part, int N, int parts, int k, u16* __restrict__ kth) {
  const int m = blockIdx.x * MT + threadIdx.x;
  if (m >= N) return;
  float list[KP];
#pragma unroll
  for (int j = 0; j < KP; ++j) list[j] = INFINITY;
  for (int s = 0; s < parts; ++s) {
    const float* src = part + ((int64_t)s * N + m) * KP;
    const f32x4 v0 = *reinterpret_cast<const f32x4*>(src), v1 = *reinterpret_cast<const f32x4*>(src + 4);
#pragma unroll
    for (int q = 0; q < 4; ++q) insert(list, v0[q]);
#pragma unroll
    for (int q = 0; q < 4; ++q) insert(list, v1[q]);
  }
  float d2 = list[0];
#pragma unroll
  for (int j = 1; j < KP; ++j) d2 = j == k ? list[j] : d2;
  kth[m] = f2h(sqrtf(d2));
}

__global__ __launch_bounds__(MT) void cover_merge_kernel(const unsigned char* __restrict__ flags, int N, int parts,
                                                         unsigned char* __restrict__ covered) {
  const int m = blockIdx.x * MT + threadIdx.x;
  if (m >= N) return;
  unsigned char any = 0;
  for (int s = 0; s < parts; ++s) any |= flags[(int64_t)s * N + m];
  covered[m] = any;
}

// What the size queries and the launches size themselves by.
struct Plan {
  int row_tiles, col_tiles, splits, tiles_per_split, parts;
  int64_t off_na, off_nb, off_part, bytes;
};

int64_t align256(int64_t v) { return (v + 255) / 256 * 256; }

Plan plan_of(int64_t Np, int64_t Nt, bool cover) {
  Plan pl;
  pl.row_tiles = (int)gad_ceil_div(Np, BM);
  pl.col_tiles = (int)gad_ceil_div(Nt, BN);
  int want = (int)gad_ceil_div(TARGET_WG, pl.row_tiles);
  want = want < 1 ? 1 : want > pl.col_tiles ? pl.col_tiles : want;
  pl.tiles_per_split = (int)gad_ceil_div(pl.col_tiles, want);
  pl.splits = (int)gad_ceil_div(pl.col_tiles, pl.tiles_per_split);
  pl.parts = pl.splits * 2;                             // the two column halves of a workgroup's tile write their own partial
  pl.off_na = 0;
  pl.off_nb = cover ? align256(Np * 4) : 0;             // the radii's targets are its probes
  pl.off_part = pl.off_nb + align256(Nt * 4);
  pl.bytes = pl.off_part + align256((int64_t)pl.parts * Np * (cover ? 1 : KP * 4));
  return pl;
}

const int MAX_ROWS = 1 << 23;                           // gridDim.x of the tile kernel; every offset is 64-bit

int check_matrix(const char* fn, const char* what, const void* F, int32_t N, int32_t D, int32_t ld) {
  GAD_CHECK(N >= 1 && N <= MAX_ROWS, "%s: %s has %d rows, must be 1 .. %d", fn, what, N, MAX_ROWS);
  GAD_CHECK(D >= 8 && D % 8 == 0, "%s: D=%d must be a positive multiple of 8", fn, D);
  GAD_CHECK(ld >= D, "%s: row stride of %s %d < D=%d", fn, what, ld, D);
  GAD_CHECK(ld % 8 == 0, "%s: row stride of %s %d must be a multiple of 8 (rows are read as 16-byte chunks)", fn, what, ld);
  if (F) GAD_CHECK(gad_aligned16(F), "%s: %s must be 16-byte aligned", fn, what);
  return 0;
}

int check_radii(const void* F, int32_t N, int32_t D, int32_t ld, int32_t k) {
  GAD_CHECK(k >= 1 && k <= KP - 1, "gad_manifold_radii: k=%d must be 1 .. %d", k, KP - 1);
  if (check_matrix("gad_manifold_radii", "F", F, N, D, ld)) return 1;
  GAD_CHECK(N >= k + 1, "gad_manifold_radii: N=%d rows have no %d-th neighbour (N >= k + 1)", N, k);
  return 0;
}

int check_cover(const void* P, int32_t Np, int32_t ldp, const void* T, int32_t Nt, int32_t ldt, int32_t D) {
  if (check_matrix("gad_manifold_cover", "P", P, Np, D, ldp)) return 1;
  return check_matrix("gad_manifold_cover", "T", T, Nt, D, ldt);
}

template <bool COVER>
int launch_tiles(const MDev& d, const Plan& pl, hipStream_t st) {
  auto kern = manifold_kernel<COVER>;
  // more than 64 KiB of dynamic LDS has to be reserved; per launch, so that it holds on whichever device is current
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES);
  GAD_CHECK(e == hipSuccess, "gad_manifold: cannot reserve %d bytes of LDS: %s", LDS_BYTES, hipGetErrorString(e));
  hipLaunchKernelGGL(kern, dim3(pl.row_tiles, pl.splits), dim3(NT), LDS_BYTES, st, d);
  GAD_LAUNCH_CHECK("manifold_kernel");
  return 0;
}

}  // namespace

#define ST ((hipStream_t)stream)

extern "C" int64_t gad_manifold_radii_workspace_bytes(int32_t N, int32_t D, int32_t ld, int32_t k) {
  if (check_radii(nullptr, N, D, ld, k)) return -1;
  return plan_of(N, N, false).bytes;
}

extern "C" int gad_manifold_radii(const void* F, int32_t N, int32_t D, int32_t ld, int32_t k, void* kth_out, void* ws,
                                  int64_t ws_bytes, void* stream) {
  GAD_CHECK(F && kth_out && ws, "gad_manifold_radii: null pointer (F, kth_out or ws)");
  if (check_radii(F, N, D, ld, k)) return 1;
  GAD_CHECK((reinterpret_cast<uintptr_t>(kth_out) & 1) == 0, "gad_manifold_radii: kth_out must be 2-byte aligned");
  GAD_CHECK(gad_aligned16(ws), "gad_manifold_radii: workspace must be 16-byte aligned");
  const Plan pl = plan_of(N, N, false);
  GAD_CHECK(ws_bytes >= pl.bytes, "gad_manifold_radii: workspace of %lld bytes, %lld needed", (long long)ws_bytes, (long long)pl.bytes);
  unsigned char* w = static_cast<unsigned char*>(ws);
  float* norms = reinterpret_cast<float*>(w + pl.off_na);
  hipLaunchKernelGGL(norms_kernel, dim3((unsigned)gad_ceil_div(N, MT / 64)), dim3(MT), 0, ST, static_cast<const u16*>(F), N, D,
                     (int64_t)ld, norms);
  GAD_LAUNCH_CHECK("gad_manifold_radii (norms)");
  MDev d = {};
  d.P = d.T = static_cast<const u16*>(F);
  d.Np = d.Nt = N, d.D = D, d.ldp = d.ldt = ld;
  d.na = d.nb = norms;
  d.part = reinterpret_cast<float*>(w + pl.off_part);
  d.col_tiles = pl.col_tiles, d.tiles_per_split = pl.tiles_per_split;
  if (int rc = launch_tiles<false>(d, pl, ST)) return rc;
  hipLaunchKernelGGL(radii_merge_kernel, dim3((unsigned)gad_ceil_div(N, MT)), dim3(MT), 0, ST, d.part, N, pl.parts, k,
                     static_cast<u16*>(kth_out));
  GAD_LAUNCH_CHECK("gad_manifold_radii (merge)");
  return 0;
}

extern "C" int64_t gad_manifold_cover_workspace_bytes(int32_t Np, int32_t ldp, int32_t Nt, int32_t ldt, int32_t D) {
  if (check_cover(nullptr, Np, ldp, nullptr, Nt, ldt, D)) return -1;
  return plan_of(Np, Nt, true).bytes;
}

extern "C" int gad_manifold_cover(const void* P, int32_t Np, int32_t ldp, const void* T, int32_t Nt, int32_t ldt, int32_t D,
                                  const void* kth_T, uint8_t* covered_out, void* ws, int64_t ws_bytes, void* stream) {
  GAD_CHECK(P && T && kth_T && covered_out && ws, "gad_manifold_cover: null pointer (P, T, kth_T, covered_out or ws)");
  if (check_cover(P, Np, ldp, T, Nt, ldt, D)) return 1;
  GAD_CHECK((reinterpret_cast<uintptr_t>(kth_T) & 1) == 0, "gad_manifold_cover: kth_T must be 2-byte aligned");
  GAD_CHECK(gad_aligned16(ws), "gad_manifold_cover: workspace must be 16-byte aligned");
  const Plan pl = plan_of(Np, Nt, true);
  GAD_CHECK(ws_bytes >= pl.bytes, "gad_manifold_cover: workspace of %lld bytes, %lld needed", (long long)ws_bytes, (long long)pl.bytes);
  unsigned char* w = static_cast<unsigned char*>(ws);
  float* na = reinterpret_cast<float*>(w + pl.off_na);
  float* nb = reinterpret_cast<float*>(w + pl.off_nb);
  hipLaunchKernelGGL(norms_kernel, dim3((unsigned)gad_ceil_div(Np, MT / 64)), dim3(MT), 0, ST, static_cast<const u16*>(P), Np, D,
                     (int64_t)ldp, na);
  GAD_LAUNCH_CHECK("gad_manifold_cover (probe norms)");
  hipLaunchKernelGGL(norms_kernel, dim3((unsigned)gad_ceil_div(Nt, MT / 64)), dim3(MT), 0, ST, static_cast<const u16*>(T), Nt, D,
                     (int64_t)ldt, nb);
  GAD_LAUNCH_CHECK("gad_manifold_cover (target norms)");
  MDev d = {};
  d.P = static_cast<const u16*>(P), d.T = static_cast<const u16*>(T);
  d.Np = Np, d.Nt = Nt, d.D = D, d.ldp = ldp, d.ldt = ldt;
  d.na = na, d.nb = nb;
  d.kth = static_cast<const u16*>(kth_T);
  d.flags = w + pl.off_part;
  d.col_tiles = pl.col_tiles, d.tiles_per_split = pl.tiles_per_split;
  if (int rc = launch_tiles<true>(d, pl, ST)) return rc;
  hipLaunchKernelGGL(cover_merge_kernel, dim3((unsigned)gad_ceil_div(Np, MT)), dim3(MT), 0, ST, d.flags, Np, pl.parts, covered_out);
  GAD_LAUNCH_CHECK("gad_manifold_cover (merge)");
  return 0;
}
