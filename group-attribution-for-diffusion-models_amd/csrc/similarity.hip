// Cosine similarity of every training row against every generated row (reference text_to_image/pixel_similarity.py,
// clip_similarity.py, baselines.py: x /= x.norm(); q /= q.norm(); x @ q), without normalised copies of either matrix.
//
//   gad_cosine_rows   sim[n][m] = (x_n . q_m) / (|x_n| |q_m|)      X [N][D] fp32 or uint8 through a 256-entry table, Q [M][D] fp32
//
// One engine, cosine_kernel<U8>: a workgroup of four waves owns 128 rows of X and one block of 64 columns (rows of Q); wave w
// owns rows [32 w, 32 w + 32) against all 64 columns, two 32 x 32 accumulators on v_mfma_f32_32x32x2_f32 - exact fp32 operands,
// one k-ordered fmaf chain per output, no bf16 / fp16 rounding.  The squared norms come from the fragments the MFMAs consume:
// the lane that feeds row r's operand also squares it, so |x_n|^2 costs no second read of X, and |q_m|^2 is taken by wave 0 of
// the first row tile alone (one workgroup column), not by every workgroup.
//
// Staging is through registers, not LDS-DMA.  The uint8 operand has to become fp32 before the MFMA can read it and an LDS-DMA
// cannot decode on the way in, so that path needs a register pass whatever the fp32 path does; and the two paths are required
// to agree bit for bit, which they do by construction when both fill ONE fp32 LDS image [row][64 + 4 floats] (rows padded by
// one 16-byte slot: the 16 rows of a ds_read_b128 lane group fall on 16 distinct slots) and share everything after it.  The
// loop is the one-register-set pipeline: write step t to LDS, barrier, issue the global loads of step t + 1, run the 64 MFMAs
// of step t behind them, barrier.  At two to three workgroups per CU (52 KiB of LDS each) the other workgroups' MFMAs cover
// the write pass.  Rows past N, columns past M and k past D are zeros selected in registers - the matrices are not read there
// (a 16-byte chunk is whole or absent: D % 4 == 0 for fp32, D % 16 == 0 for uint8).
//
// D is split over gridDim.y in whole 64-wide steps; every split writes its partial dots [split][N][M] and partial squared
// norms [split][N], [split][M] to the workspace, and merge_kernel adds them in split order and forms the quotient.  No atomics,
// no cross-workgroup communication: the result is a function of the inputs (and of `splits`) alone.  The automatic split
// count depends on N and D only, so a column block computes the same bits whichever M it is launched with.
#include <math.h>

#include "gad_dev.h"

namespace {

constexpr int BM = 128, BN = 64, BK = 64, NW = 4, NT = NW * 64, TN = BN / 32;
constexpr int LDT = BK + 4;                              // tile row stride in floats (272 B)
constexpr int CH = BK / 4;                               // 16-byte fp32 chunks per tile row
constexpr int XF = BM * CH / NT, QF = BN * CH / NT;      // fp32 chunks per thread and step: X 8, Q 4
constexpr int XU = BM * (BK / 16) / NT;                  // uint8 chunks (16 elements) per thread and step: 2
constexpr int LDS_FLOATS = (BM + BN) * LDT + 256;        // the two tiles and the decode table
constexpr int TARGET_WG = 512;                           // 256 CUs x 2 resident workgroups
constexpr int MT = 256;                                  // threads of the merge kernel
constexpr int MAX_SPLITS = 4096;
static_assert(XF * NT == BM * CH && QF * NT == BN * CH && XU * NT * 16 == BM * BK, "whole chunks per thread");

struct CDev {
  const void* X; const float* Q; const float* lut;
  int64_t ldx, ldq, D;
  int N, M;
  int steps, steps_per_split;
  float* pdot; float* pnx; float* pnq;                   // [splits][N][M], [splits][N], [splits][M]
};

template <bool U8>
__global__ __launch_bounds__(NT, 2) void cosine_kernel(const CDev p) {
  __shared__ __attribute__((aligned(16))) float lds[LDS_FLOATS];
  float* const xa = lds;
  float* const qb = lds + BM * LDT;
  float* const tab = lds + (BM + BN) * LDT;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, h = lane >> 5;
  const int row0 = blockIdx.x * BM, split = blockIdx.y, col0 = blockIdx.z * BN;
  const bool q_norms = blockIdx.x == 0 && wave == 0;

  if constexpr (U8) {                                    // NT == 256 entries, published before the first decode
    tab[tid] = p.lut[tid];
    __syncthreads();
  }

  // ---- what this thread stages: fp32 chunk f = i NT + tid is tile row f / CH, chunk f % CH; uint8 chunk likewise with BK / 16
  const float* qsrc[QF];
#pragma unroll
  for (int i = 0; i < QF; ++i) {
    const int f = i * NT + tid, m = col0 + f / CH;
    qsrc[i] = m < p.M ? p.Q + (int64_t)m * p.ldq + (f % CH) * 4 : nullptr;
  }
  const float* xsrc[XF];
  const unsigned char* usrc[XU];
  if constexpr (U8) {
#pragma unroll
    for (int i = 0; i < XU; ++i) {
      const int f = i * NT + tid, n = row0 + f / (BK / 16);
      usrc[i] = n < p.N ? static_cast<const unsigned char*>(p.X) + (int64_t)n * p.ldx + (f % (BK / 16)) * 16 : nullptr;
    }
  } else {
#pragma unroll
    for (int i = 0; i < XF; ++i) {
      const int f = i * NT + tid, n = row0 + f / CH;
      xsrc[i] = n < p.N ? static_cast<const float*>(p.X) + (int64_t)n * p.ldx + (f % CH) * 4 : nullptr;
    }
  }

  f32x4 qreg[QF];
  f32x4 xreg[U8 ? 1 : XF];
  u32x4 ureg[U8 ? XU : 1];
  bool uin[U8 ? XU : 1];
  auto fetch = [&](int64_t k0) {
#pragma unroll
    for (int i = 0; i < QF; ++i) {
      const int f = i * NT + tid;
      const bool in = qsrc[i] && k0 + (f % CH) * 4 < p.D;
      qreg[i] = in ? *reinterpret_cast<const f32x4*>(qsrc[i] + k0) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
    if constexpr (U8) {
#pragma unroll
      for (int i = 0; i < XU; ++i) {
        const int f = i * NT + tid;
        uin[i] = usrc[i] && k0 + (f % (BK / 16)) * 16 < p.D;
        ureg[i] = uin[i] ? *reinterpret_cast<const u32x4*>(usrc[i] + k0) : u32x4{0u, 0u, 0u, 0u};
      }
    } else {
#pragma unroll
      for (int i = 0; i < XF; ++i) {
        const int f = i * NT + tid;
        const bool in = xsrc[i] && k0 + (f % CH) * 4 < p.D;
        xreg[i] = in ? *reinterpret_cast<const f32x4*>(xsrc[i] + k0) : f32x4{0.f, 0.f, 0.f, 0.f};
      }
    }
  };
  auto deposit = [&]() {
#pragma unroll
    for (int i = 0; i < QF; ++i) {
      const int f = i * NT + tid;
      *reinterpret_cast<f32x4*>(qb + (f / CH) * LDT + (f % CH) * 4) = qreg[i];
    }
    if constexpr (U8) {
#pragma unroll
      for (int i = 0; i < XU; ++i) {
        const int f = i * NT + tid;
        float* dst = xa + (f / (BK / 16)) * LDT + (f % (BK / 16)) * 16;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
          const unsigned v = ureg[i][w];
          f32x4 o;
          o[0] = tab[v & 255u], o[1] = tab[(v >> 8) & 255u], o[2] = tab[(v >> 16) & 255u], o[3] = tab[v >> 24];
          if (!uin[i]) o = f32x4{0.f, 0.f, 0.f, 0.f};    // outside the matrix the VALUE is zero, not the table's entry 0
          *reinterpret_cast<f32x4*>(dst + w * 4) = o;
        }
      }
    } else {
#pragma unroll
      for (int i = 0; i < XF; ++i) {
        const int f = i * NT + tid;
        *reinterpret_cast<f32x4*>(xa + (f / CH) * LDT + (f % CH) * 4) = xreg[i];
      }
    }
  };

  f32x16 acc[TN];
#pragma unroll
  for (int j = 0; j < TN; ++j)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[j][e] = 0.f;
  float sx = 0.f, sq[TN] = {};
  const float* const arow = xa + (wave * 32 + l31) * LDT + h * 4;
  const float* const brow = qb + l31 * LDT + h * 4;
  // the MFMA's two k slots are the two half-waves: group g feeds chunk 2 g + h of the row, its four floats one MFMA each
  auto compute = [&]() {
#pragma unroll
    for (int g = 0; g < CH / 2; ++g) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(arow + g * 8);
      f32x4 b[TN];
#pragma unroll
      for (int j = 0; j < TN; ++j) b[j] = *reinterpret_cast<const f32x4*>(brow + j * 32 * LDT + g * 8);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q], b[j][q], acc[j], 0, 0, 0);
        sx = fmaf(a[q], a[q], sx);
      }
      if (q_norms) {
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
          for (int q = 0; q < 4; ++q) sq[j] = fmaf(b[j][q], b[j][q], sq[j]);
      }
    }
  };

  const int st0 = split * p.steps_per_split;
  const int st1 = min(p.steps, st0 + p.steps_per_split);  // an empty split (forced counts only) writes zeros
  if (st0 < st1) fetch((int64_t)st0 * BK);
  for (int st = st0; st < st1; ++st) {
    deposit();
    __syncthreads();
    if (st + 1 < st1) fetch((int64_t)(st + 1) * BK);
    compute();
    __syncthreads();                                      // every wave is past this step's fragments
  }

  // accumulator register e of tile j is row 8 (e >> 2) + 4 h + (e & 3) of the wave's 32, column 32 j + l31
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int m = col0 + j * 32 + l31;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int n = row0 + wave * 32 + 8 * (e >> 2) + 4 * h + (e & 3);
      if (n < p.N && m < p.M) p.pdot[((int64_t)split * p.N + n) * p.M + m] = acc[j][e];
    }
  }
  // the two half-waves hold the two k slots of a row: one addition, the same on either side
  sx += __shfl_xor(sx, 32, 64);
  const int n = row0 + wave * 32 + l31;
  if (blockIdx.z == 0 && h == 0 && n < p.N) p.pnx[(int64_t)split * p.N + n] = sx;
  if (q_norms) {
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const float s = sq[j] + __shfl_xor(sq[j], 32, 64);
      const int m = col0 + j * 32 + l31;
      if (h == 0 && m < p.M) p.pnq[(int64_t)split * p.M + m] = s;
    }
  }
}

// the splits' partials in split order, then the quotient; 0 / 0 = NaN for a zero row (no eps)
__global__ __launch_bounds__(MT) void merge_kernel(const float* __restrict__ pdot, const float* __restrict__ pnx,
                                                   const float* __restrict__ pnq, int N, int M, int splits,
                                                   float* __restrict__ sim) {
  const int64_t total = (int64_t)N * M, idx = (int64_t)blockIdx.x * MT + threadIdx.x;
  if (idx >= total) return;
  const int64_t n = idx / M, m = idx - n * M;
  float dot = 0.f, nx = 0.f, nq = 0.f;
  for (int s = 0; s < splits; ++s) {
    dot += pdot[(int64_t)s * total + idx];
    nx += pnx[(int64_t)s * N + n];
    nq += pnq[(int64_t)s * M + m];
  }
  sim[idx] = dot / (sqrtf(nx) * sqrtf(nq));
}

// What the size query and the launch size themselves by.
struct Plan {
  int row_tiles, col_blocks, steps, splits, steps_per_split;
  int64_t off_dot, off_nx, off_nq, bytes;
};

int64_t align256(int64_t v) { return (v + 255) / 256 * 256; }

Plan plan_of(int64_t N, int64_t M, int64_t D, int splits) {
  Plan pl;
  pl.row_tiles = (int)gad_ceil_div(N, BM);
  pl.col_blocks = (int)gad_ceil_div(M, BN);
  pl.steps = (int)gad_ceil_div(D, BK);
  if (splits > 0) {                                       // forced: exactly that many, the trailing ones possibly empty
    pl.splits = splits;
    pl.steps_per_split = (int)gad_ceil_div(pl.steps, splits);
  } else {                                                // from N and D alone: a column block's bits do not depend on M
    int want = TARGET_WG / pl.row_tiles;
    want = want < 1 ? 1 : want > pl.steps ? pl.steps : want;
    pl.steps_per_split = (int)gad_ceil_div(pl.steps, want);
    pl.splits = (int)gad_ceil_div(pl.steps, pl.steps_per_split);
  }
  pl.off_dot = 0;
  pl.off_nx = align256((int64_t)pl.splits * N * M * 4);
  pl.off_nq = pl.off_nx + align256((int64_t)pl.splits * N * 4);
  pl.bytes = pl.off_nq + align256((int64_t)pl.splits * M * 4);
  return pl;
}

const int64_t MAX_ROWS = (int64_t)BM * ((1 << 24) - 1);  // every offset is 64-bit; gridDim.x stays far below 2^31
const int64_t MAX_COLS = (int64_t)BN * 65535;            // gridDim.z
const int64_t MAX_D = (int64_t)BK << 30;                 // the step index is an int
const int64_t MAX_SIM = (int64_t)1 << 38;                // N M: the merge kernel's grid

int check_shape(int64_t N, int64_t M, int64_t D, int32_t x_kind, int32_t splits) {
  GAD_CHECK(x_kind == GAD_SIM_X_F32 || x_kind == GAD_SIM_X_U8, "gad_cosine_rows: unknown x_kind %d", x_kind);
  GAD_CHECK(N >= 1 && N <= MAX_ROWS, "gad_cosine_rows: N=%lld must be 1 .. %lld", (long long)N, (long long)MAX_ROWS);
  GAD_CHECK(M >= 1 && M <= MAX_COLS, "gad_cosine_rows: M=%lld must be 1 .. %lld", (long long)M, (long long)MAX_COLS);
  const int qx = x_kind == GAD_SIM_X_U8 ? 16 : 4;
  GAD_CHECK(D >= 1 && D <= MAX_D && D % qx == 0, "gad_cosine_rows: D=%lld must be a positive multiple of %d", (long long)D, qx);
  GAD_CHECK(N * M <= MAX_SIM, "gad_cosine_rows: N M = %lld outputs, at most %lld", (long long)(N * M), (long long)MAX_SIM);
  GAD_CHECK(splits >= 0 && splits <= MAX_SPLITS, "gad_cosine_rows: splits=%d must be 0 (automatic) .. %d", splits, MAX_SPLITS);
  return 0;
}

}  // namespace

#define ST ((hipStream_t)stream)

extern "C" int64_t gad_cosine_rows_workspace_bytes(int64_t N, int64_t M, int64_t D, int32_t x_kind, int32_t splits) {
  if (check_shape(N, M, D, x_kind, splits)) return -1;
  return plan_of(N, M, D, splits).bytes;
}

extern "C" int gad_cosine_rows(const void* X, int32_t x_kind, int64_t ldx, const float* lut, const float* Q, int64_t ldq, float* sim,
                               int64_t N, int64_t M, int64_t D, int32_t splits, void* ws, int64_t ws_bytes, void* stream) {
  GAD_CHECK(X && Q && sim && ws, "gad_cosine_rows: null pointer (X, Q, sim or ws)");
  if (check_shape(N, M, D, x_kind, splits)) return 1;
  const bool u8 = x_kind == GAD_SIM_X_U8;
  GAD_CHECK(!u8 || lut, "gad_cosine_rows: null pointer (lut) with GAD_SIM_X_U8");
  GAD_CHECK(!u8 || (reinterpret_cast<uintptr_t>(lut) & 3) == 0, "gad_cosine_rows: lut must be 4-byte aligned");
  GAD_CHECK(ldx >= D, "gad_cosine_rows: row stride of X %lld < D=%lld", (long long)ldx, (long long)D);
  GAD_CHECK(ldq >= D, "gad_cosine_rows: row stride of Q %lld < D=%lld", (long long)ldq, (long long)D);
  GAD_CHECK(ldx % (u8 ? 16 : 4) == 0, "gad_cosine_rows: row stride of X %lld must be a multiple of %d (rows are read as 16-byte chunks)",
            (long long)ldx, u8 ? 16 : 4);
  GAD_CHECK(ldq % 4 == 0, "gad_cosine_rows: row stride of Q %lld must be a multiple of 4 (rows are read as 16-byte chunks)",
            (long long)ldq);
  GAD_CHECK(gad_aligned16(X) && gad_aligned16(Q), "gad_cosine_rows: X and Q must be 16-byte aligned");
  GAD_CHECK((reinterpret_cast<uintptr_t>(sim) & 3) == 0, "gad_cosine_rows: sim must be 4-byte aligned");
  GAD_CHECK(gad_aligned16(ws), "gad_cosine_rows: workspace must be 16-byte aligned");
  const Plan pl = plan_of(N, M, D, splits);
  GAD_CHECK(ws_bytes >= pl.bytes, "gad_cosine_rows: workspace of %lld bytes, %lld needed", (long long)ws_bytes, (long long)pl.bytes);

  unsigned char* w = static_cast<unsigned char*>(ws);
  CDev d = {};
  d.X = X, d.Q = Q, d.lut = lut;
  d.ldx = ldx, d.ldq = ldq, d.D = D;
  d.N = (int)N, d.M = (int)M;
  d.steps = pl.steps, d.steps_per_split = pl.steps_per_split;
  d.pdot = reinterpret_cast<float*>(w + pl.off_dot);
  d.pnx = reinterpret_cast<float*>(w + pl.off_nx);
  d.pnq = reinterpret_cast<float*>(w + pl.off_nq);
  const dim3 grid(pl.row_tiles, pl.splits, pl.col_blocks);
  if (u8) hipLaunchKernelGGL(cosine_kernel<true>, grid, dim3(NT), 0, ST, d);
  else hipLaunchKernelGGL(cosine_kernel<false>, grid, dim3(NT), 0, ST, d);
  GAD_LAUNCH_CHECK("gad_cosine_rows (tiles)");
  hipLaunchKernelGGL(merge_kernel, dim3((unsigned)gad_ceil_div(N * M, MT)), dim3(MT), 0, ST, d.pdot, d.pnx, d.pnq, (int)N, (int)M,
                     pl.splits, sim);
  GAD_LAUNCH_CHECK("gad_cosine_rows (merge)");
  return 0;
}
