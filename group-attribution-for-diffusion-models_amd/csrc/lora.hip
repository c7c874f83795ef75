// LoRA with dropout on the adapter input (peft: y = base(x) + B(A(dropout(x))) * alpha / r), for up to four projections that
// share their input (an attention block's to_q / to_k / to_v), plus the one-off merge W += s B A.
//
//   forward    mid_j [M][r] = s * ( x o m_j / (1 - p) ) A_j^T                       one read of x for all projections
//   backward   dA_j  [r][C] = dmid_j^T ( x o m_j / (1 - p) )
//              dx    [M][C] += sum_j ( dmid_j A_j ) o m_j / (1 - p)                  on top of the base path's data gradient
//
// The keep mask m_j is never stored and no dropped copy of x is written.  m_j(m, c) is a pure function of
// (seed, offset, layer, j, m, c): Philox-4x32-10 (Random123 constants) with
//     key     = (seed, offset)
//     counter = (c >> 2,  m & 0xffffffff,  m >> 32,  (layer << 2) | j)
// One call serves channels 4 (c >> 2) .. + 3 of row m: channel c takes word c & 3 of the result (x, y, z, w) and is KEPT when
// word >= floor(p * 2^32).  Forward and backward call it with the same arguments; nothing in it knows about grids or tiles.
//
// Both products run on v_mfma_f32_16x16x4_f32 (exact fp32) with the rank zero-padded to 16 per column tile in registers; a
// lane's float4 of x is exactly one Philox block, so one call masks the four k steps (forward) or the four column tiles
// (backward) it feeds.  Column tiles (projection j, 16 ranks) are taken four at a time: three projections at rank <= 16 are
// one pass; more tiles than that re-read x per pass.
//   forward   wave: 32 rows; lane (j = l & 15, kq = l >> 4): A operand x[m0 + 16 mb + j][kc + 4 kq + s], B operand
//             A_j[16 rt + j][kc + 4 kq + s], s = 0..3 the k steps of a 16-channel chunk.  Grid-stride over 32-row blocks.
//   backward  workgroup = one row slab (a plan that depends on M alone), wave w = channel blocks 64 (w + 4 i); per 16 rows a
//             lane holds rows m0 + 4 kq + t (t = 0..3) of channels cb + 4 j .. + 3, the same element set in the dA product (k = the
//             row, column tile e = float4 element e) and in the dx product's result tile, so one mask serves both.  dA partials
//             per slab go to the workspace and a second kernel adds them in slab order: no atomics, bit-reproducible.
// C % 4 == 0 with 16-byte aligned pointers and strides that are multiples of 4 takes float4 accesses; anything else takes
// guarded scalar accesses in the same kernels.  Row offsets are 64-bit.
// p == 0: the forward IS the plain down-projection - n_proj gad_gemm launches, bit-equal to it by construction whatever
// route the planner takes - and the backward runs the mask-free instances; neither touches Philox.
#include <algorithm>

#include "gad_dev.h"

namespace {

constexpr int LD_WAVES = 4;             // waves per workgroup
constexpr int LD_MB = 2;                // forward: 16-row blocks per wave trip
constexpr int LD_UNITS = 4;             // column tiles per pass
constexpr int64_t LD_MAX_SLABS = 256;   // backward: one workgroup per slab, partials = slabs x tiles x 16 x C floats
constexpr int LD_FWD_BLOCKS = 2048;

struct Dev {
  const float* x;
  int64_t ldx, M;
  int C, r, RT, total;          // RT = ceil(r / 16) column tiles per projection, total = n_proj * RT
  const float* A[4];
  float* mid[4];
  const float* dmid[4];
  float* dx;
  int64_t ld_dx;
  float scale, inv_keep;
  uint32_t thr, seed, offset, layer;
  int vec;
};

// 1 / (1 - p) where kept, 0 where dropped, for channels 4 cblock .. + 3 of row m under projection j
__device__ __forceinline__ f32x4 keep4(const Dev& d, int j, int64_t m, uint32_t cblock) {
  const uint4 w = philox4x32_10(make_uint4(cblock, (uint32_t)m, (uint32_t)((uint64_t)m >> 32), (d.layer << 2) | (uint32_t)j), d.seed,
                                d.offset);
  return f32x4{w.x >= d.thr ? d.inv_keep : 0.f, w.y >= d.thr ? d.inv_keep : 0.f, w.z >= d.thr ? d.inv_keep : 0.f,
               w.w >= d.thr ? d.inv_keep : 0.f};
}

// row[c .. c + 3] with zeros at and past C (c is a multiple of 4)
__device__ __forceinline__ f32x4 ld4(const float* row, int c, int C, bool vec) {
  f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
  if (vec) {
    if (c < C) v = *reinterpret_cast<const f32x4*>(row + c);
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (c + e < C) v[e] = row[c + e];
  }
  return v;
}

__device__ __forceinline__ void st4(float* row, int c, int C, bool vec, f32x4 v) {
  if (vec) {
    if (c < C) *reinterpret_cast<f32x4*>(row + c) = v;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (c + e < C) row[c + e] = v[e];
  }
}

template <int UNITS>
__global__ __launch_bounds__(LD_WAVES * 64) void lora_down_fwd_kernel(const Dev d, int u0) {
  const int lane = threadIdx.x & 63;
  const int j16 = lane & 15, kq = lane >> 4;
  const bool vec = d.vec != 0;
  const int64_t wave = (int64_t)blockIdx.x * LD_WAVES + (threadIdx.x >> 6);
  const int64_t stride = (int64_t)gridDim.x * LD_WAVES * (16 * LD_MB);
  for (int64_t m0 = wave * (16 * LD_MB); m0 < d.M; m0 += stride) {
    int64_t mrow[LD_MB];
    bool ok[LD_MB];
#pragma unroll
    for (int mb = 0; mb < LD_MB; ++mb) {
      mrow[mb] = m0 + 16 * mb + j16;
      ok[mb] = mrow[mb] < d.M;
    }
    f32x4 acc[LD_MB][UNITS];
#pragma unroll
    for (int mb = 0; mb < LD_MB; ++mb)
#pragma unroll
      for (int u = 0; u < UNITS; ++u) acc[mb][u] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int kc = 0; kc < d.C; kc += 16) {
      const int c = kc + 4 * kq;
      f32x4 xv[LD_MB], am[LD_MB];
#pragma unroll
      for (int mb = 0; mb < LD_MB; ++mb)
        xv[mb] = ok[mb] ? ld4(d.x + mrow[mb] * d.ldx, c, d.C, vec) : f32x4{0.f, 0.f, 0.f, 0.f};
      int jprev = -1;
#pragma unroll
      for (int u = 0; u < UNITS; ++u) {
        const int unit = u0 + u;
        const int j = unit / d.RT, rt = unit - j * d.RT;
        if (j != jprev) {
#pragma unroll
          for (int mb = 0; mb < LD_MB; ++mb) am[mb] = ok[mb] ? xv[mb] * keep4(d, j, mrow[mb], (uint32_t)(c >> 2)) : xv[mb];
          jprev = j;
        }
        const int rr = 16 * rt + j16;
        const f32x4 b = rr < d.r ? ld4(d.A[j] + (int64_t)rr * d.C, c, d.C, vec) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
          for (int mb = 0; mb < LD_MB; ++mb) acc[mb][u] = mfma16(am[mb][s], b[s], acc[mb][u]);
      }
    }

    // C/D of 16x16x4: column lane & 15, row 4 (lane >> 4) + reg
#pragma unroll
    for (int u = 0; u < UNITS; ++u) {
      const int unit = u0 + u;
      const int j = unit / d.RT, rt = unit - j * d.RT;
      const int rr = 16 * rt + j16;
      if (rr >= d.r) continue;
      float* out = d.mid[j];
#pragma unroll
      for (int mb = 0; mb < LD_MB; ++mb)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          const int64_t m = m0 + 16 * mb + 4 * kq + reg;
          if (m < d.M) out[m * d.r + rr] = d.scale * acc[mb][u][reg];
        }
    }
  }
}

template <int UNITS, bool DROP>
__global__ __launch_bounds__(LD_WAVES * 64) void lora_down_bwd_kernel(const Dev d, int u0, int64_t slab_len, float* __restrict__ ws) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j16 = lane & 15, kq = lane >> 4;
  const bool vec = d.vec != 0;
  const int64_t slab = blockIdx.x;
  const int64_t mb0 = slab * slab_len, me = min(d.M, mb0 + slab_len);
  const f32x4 zero = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int cb = 64 * wave; cb < d.C; cb += 64 * LD_WAVES) {
    const int c = cb + 4 * j16;                   // this lane's four channels: one Philox block
    f32x4 accA[UNITS][4], bA[UNITS][4];
#pragma unroll
    for (int u = 0; u < UNITS; ++u) {
      const int unit = u0 + u;
      const int j = unit / d.RT, rt = unit - j * d.RT;
#pragma unroll
      for (int st = 0; st < 4; ++st) {
        const int rr = 16 * rt + 4 * st + kq;      // k index of the dx product
        bA[u][st] = rr < d.r ? ld4(d.A[j] + (int64_t)rr * d.C, c, d.C, vec) : zero;
        accA[u][st] = zero;
      }
    }

    for (int64_t m0 = mb0; m0 < me; m0 += 16) {
      int64_t mr[4];
      bool ok[4];
      f32x4 xv[4], dxv[4], k4[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        mr[t] = m0 + 4 * kq + t;
        ok[t] = mr[t] < me;
        xv[t] = ok[t] ? ld4(d.x + mr[t] * d.ldx, c, d.C, vec) : zero;
        dxv[t] = ok[t] ? ld4(d.dx + mr[t] * d.ld_dx, c, d.C, vec) : zero;
        k4[t] = f32x4{1.f, 1.f, 1.f, 1.f};
      }
      const int64_t mrow = m0 + j16;               // the dx product's A operand row
      const bool rok = mrow < me;
      int jprev = -1;
#pragma unroll
      for (int u = 0; u < UNITS; ++u) {
        const int unit = u0 + u;
        const int j = unit / d.RT, rt = unit - j * d.RT;
        if (DROP && j != jprev) {
#pragma unroll
          for (int t = 0; t < 4; ++t)
            if (ok[t]) k4[t] = keep4(d, j, mr[t], (uint32_t)(c >> 2));
          jprev = j;
        }
        const float* dm = d.dmid[j];
        // dA tile (rank 16 rt + row, channel cb + 4 n + e): k = the four rows m0 + 4 kq + t of step t
        const int rra = 16 * rt + j16;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const float a = (ok[t] && rra < d.r) ? dm[mr[t] * d.r + rra] : 0.f;
          const f32x4 xm = DROP ? xv[t] * k4[t] : xv[t];
#pragma unroll
          for (int e = 0; e < 4; ++e) accA[u][e] = mfma16(a, xm[e], accA[u][e]);
        }
        // T = dmid_j[16 rows][16 ranks of rt] A_j[those ranks][64 channels]: tile e, register reg = row m0 + 4 kq + reg, channel c + e
        f32x4 T[4] = {zero, zero, zero, zero};
#pragma unroll
        for (int st = 0; st < 4; ++st) {
          const int rr = 16 * rt + 4 * st + kq;
          const float a2 = (rok && rr < d.r) ? dm[mrow * d.r + rr] : 0.f;
#pragma unroll
          for (int e = 0; e < 4; ++e) T[e] = mfma16(a2, bA[u][st][e], T[e]);
        }
#pragma unroll
        for (int reg = 0; reg < 4; ++reg)
#pragma unroll
          for (int e = 0; e < 4; ++e) dxv[reg][e] += DROP ? T[e][reg] * k4[reg][e] : T[e][reg];
      }
#pragma unroll
      for (int t = 0; t < 4; ++t)
        if (ok[t]) st4(d.dx + mr[t] * d.ld_dx, c, d.C, vec, dxv[t]);
    }

    // partial dA of this slab: ws[slab][unit][16][C]
#pragma unroll
    for (int u = 0; u < UNITS; ++u)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        float* row = ws + ((slab * d.total + (u0 + u)) * 16 + 4 * kq + reg) * (int64_t)d.C;
        st4(row, c, d.C, vec, f32x4{accA[u][0][reg], accA[u][1][reg], accA[u][2][reg], accA[u][3][reg]});
      }
  }
}

// dA_j[rr][c] = sum over slabs, in slab order
__global__ __launch_bounds__(256) void lora_da_reduce_kernel(const Dev d, const float* __restrict__ ws, int64_t n_slabs, float* dA0,
                                                             float* dA1, float* dA2, float* dA3) {
  const int64_t per = (int64_t)d.total * 16 * d.C;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= per) return;
  const int c = (int)(i % d.C);
  const int64_t row = i / d.C;
  const int unit = (int)(row / 16), j = unit / d.RT, rr = 16 * (unit - j * d.RT) + (int)(row % 16);
  if (rr >= d.r) return;
  float s = ws[i];
  for (int64_t k = 1; k < n_slabs; ++k) s += ws[k * per + i];
  float* out = j == 0 ? dA0 : j == 1 ? dA1 : j == 2 ? dA2 : dA3;
  out[(int64_t)rr * d.C + c] = s;
}

__global__ __launch_bounds__(256) void lora_merge_kernel(float* __restrict__ W, int64_t ldw, const float* __restrict__ B,
                                                         const float* __restrict__ A, int N, int K, int r, float alpha) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)N * K) return;
  const int64_t n = i / K;
  const int k = (int)(i - n * K);
  float acc = 0.f;
  for (int rr = 0; rr < r; ++rr) acc = fmaf(B[n * r + rr], A[(int64_t)rr * K + k], acc);
  W[n * ldw + k] = fmaf(alpha, acc, W[n * ldw + k]);
}

struct SlabPlan {
  int64_t slab_len, n_slabs;
};

// depends on M alone: the order in which a dA element's terms are added is the same for every launch of that M
SlabPlan slab_plan(int64_t M) {
  const int64_t blocks16 = gad_ceil_div(M, 16);
  const int64_t want = std::min<int64_t>(blocks16, LD_MAX_SLABS);
  SlabPlan pl;
  pl.slab_len = gad_ceil_div(blocks16, want) * 16;
  pl.n_slabs = gad_ceil_div(M, pl.slab_len);
  return pl;
}

int lora_validate(const gad_lora_dropout_args* a, const char* who) {
  GAD_CHECK(a != nullptr, "%s: null args", who);
  GAD_CHECK(a->p >= 0.0 && a->p < 1.0, "%s: dropout p=%g outside [0, 1)", who, a->p);
  GAD_CHECK(a->n_proj >= 1 && a->n_proj <= 4, "%s: n_proj=%d outside 1..4", who, a->n_proj);
  GAD_CHECK(a->M >= 1, "%s: M=%lld must be >= 1", who, (long long)a->M);
  GAD_CHECK(a->C >= 1, "%s: C=%d must be >= 1", who, a->C);
  GAD_CHECK(a->r >= 4 && a->r <= 64 && a->r % 4 == 0, "%s: rank r=%d must be a multiple of 4 in 4..64", who, a->r);
  GAD_CHECK(a->ldx >= a->C, "%s: ldx=%lld below C=%d", who, (long long)a->ldx, a->C);
  GAD_CHECK(a->layer < (1u << 30), "%s: layer=%u must be below 2^30", who, a->layer);
  return 0;
}

int64_t bwd_bytes(const gad_lora_dropout_args* a) {
  const SlabPlan pl = slab_plan(a->M);
  return pl.n_slabs * (int64_t)a->n_proj * gad_ceil_div(a->r, 16) * 16 * a->C * (int64_t)sizeof(float);
}

void plain_gemm_args(const gad_lora_dropout_args* a, int j, gad_gemm_args* g) {
  memset(g, 0, sizeof(*g));
  g->A = a->x;
  g->B = a->A[j];
  g->C = a->mid[j];
  g->a_mode = GAD_A_KC;
  g->b_mode = GAD_B_KC;
  g->M = (int32_t)a->M;
  g->N = a->r;
  g->K = a->C;
  g->lda = (int32_t)a->ldx;
  g->ldb = a->C;
  g->ldc = a->r;
  g->batch = 1;
  g->batch_inner = 1;
  g->alpha = a->scale;
  g->rows_per_group = 1;
  g->ws = a->workspace;
  g->ws_bytes = a->workspace_bytes;
}

Dev make_dev(const gad_lora_dropout_args* a, bool backward) {
  Dev d;
  memset(&d, 0, sizeof(d));
  d.x = a->x;
  d.ldx = a->ldx;
  d.M = a->M;
  d.C = a->C;
  d.r = a->r;
  d.RT = (int)gad_ceil_div(a->r, 16);
  d.total = a->n_proj * d.RT;
  bool vec = a->C % 4 == 0 && a->ldx % 4 == 0 && gad_aligned16(a->x);
  for (int j = 0; j < a->n_proj; ++j) {
    d.A[j] = a->A[j];
    d.mid[j] = a->mid[j];
    d.dmid[j] = a->dmid[j];
    vec = vec && gad_aligned16(a->A[j]);
  }
  if (backward) {
    d.dx = a->dx;
    d.ld_dx = a->ld_dx;
    vec = vec && a->ld_dx % 4 == 0 && gad_aligned16(a->dx) && gad_aligned16(a->workspace);
  }
  d.vec = vec ? 1 : 0;
  d.scale = a->scale;
  d.inv_keep = (float)(1.0 / (1.0 - a->p));
  d.thr = (uint32_t)(a->p * 4294967296.0);          // floor(p 2^32); p < 1
  d.seed = a->seed;
  d.offset = a->offset;
  d.layer = a->layer;
  return d;
}

}  // namespace

extern "C" int64_t gad_lora_down_dropout_workspace_bytes(const gad_lora_dropout_args* a) {
  if (lora_validate(a, "gad_lora_down_dropout_workspace_bytes") != 0) return -1;
  int64_t need = bwd_bytes(a);
  if (a->p == 0.0 && a->M <= INT32_MAX && a->ldx <= INT32_MAX) {      // the forward's plain launches may split K
    gad_lora_dropout_args b = *a;
    b.workspace = nullptr;
    b.workspace_bytes = 0;
    gad_gemm_args g;
    plain_gemm_args(&b, 0, &g);
    g.A = g.B = g.C = reinterpret_cast<float*>(uintptr_t(4096));     // the size query reads only alignments
    need = std::max<int64_t>(need, gad_gemm_workspace_bytes(&g));
  }
  return need;
}

extern "C" int gad_lora_down_dropout_fwd(const gad_lora_dropout_args* a, void* stream) {
  const char* who = "gad_lora_down_dropout_fwd";
  if (lora_validate(a, who) != 0) return 1;
  GAD_CHECK(a->x != nullptr, "%s: null pointer (x)", who);
  for (int j = 0; j < a->n_proj; ++j) GAD_CHECK(a->A[j] != nullptr && a->mid[j] != nullptr, "%s: null pointer (A[%d] or mid[%d])", who, j, j);
  if (a->p == 0.0) {
    GAD_CHECK(a->M <= INT32_MAX && a->ldx <= INT32_MAX, "%s: M=%lld beyond the plain down-projection's 32-bit rows", who, (long long)a->M);
    for (int j = 0; j < a->n_proj; ++j) {
      gad_gemm_args g;
      plain_gemm_args(a, j, &g);
      const int64_t need = gad_gemm_workspace_bytes(&g);
      GAD_CHECK(need <= 0 || (a->workspace != nullptr && a->workspace_bytes >= need), "%s: workspace_bytes=%lld < %lld (short workspace)", who,
                (long long)a->workspace_bytes, (long long)need);
      const int rc = gad_gemm(&g, stream);
      if (rc != 0) return rc;
    }
    return 0;
  }
  const Dev d = make_dev(a, false);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int cap = a->max_blocks > 0 ? a->max_blocks : LD_FWD_BLOCKS;
  const dim3 grid((unsigned)std::min<int64_t>(cap, gad_ceil_div(a->M, LD_WAVES * 16 * LD_MB)));
  for (int u0 = 0; u0 < d.total; u0 += LD_UNITS) {
    switch (std::min(LD_UNITS, d.total - u0)) {
      case 1: hipLaunchKernelGGL((lora_down_fwd_kernel<1>), grid, dim3(LD_WAVES * 64), 0, st, d, u0); break;
      case 2: hipLaunchKernelGGL((lora_down_fwd_kernel<2>), grid, dim3(LD_WAVES * 64), 0, st, d, u0); break;
      case 3: hipLaunchKernelGGL((lora_down_fwd_kernel<3>), grid, dim3(LD_WAVES * 64), 0, st, d, u0); break;
      default: hipLaunchKernelGGL((lora_down_fwd_kernel<4>), grid, dim3(LD_WAVES * 64), 0, st, d, u0); break;
    }
    GAD_LAUNCH_CHECK("lora_down_fwd_kernel");
  }
  return 0;
}

extern "C" int gad_lora_down_dropout_bwd(const gad_lora_dropout_args* a, void* stream) {
  const char* who = "gad_lora_down_dropout_bwd";
  if (lora_validate(a, who) != 0) return 1;
  GAD_CHECK(a->x != nullptr && a->dx != nullptr && a->workspace != nullptr, "%s: null pointer (x, dx or workspace)", who);
  for (int j = 0; j < a->n_proj; ++j)
    GAD_CHECK(a->A[j] != nullptr && a->dmid[j] != nullptr && a->dA[j] != nullptr, "%s: null pointer (A[%d], dmid[%d] or dA[%d])", who, j, j, j);
  GAD_CHECK(a->ld_dx >= a->C, "%s: ld_dx=%lld below C=%d", who, (long long)a->ld_dx, a->C);
  const int64_t need = bwd_bytes(a);
  GAD_CHECK(a->workspace_bytes >= need, "%s: workspace_bytes=%lld < %lld (short workspace)", who, (long long)a->workspace_bytes,
            (long long)need);
  const Dev d = make_dev(a, true);
  const SlabPlan pl = slab_plan(a->M);
  hipStream_t st = static_cast<hipStream_t>(stream);
  float* ws = static_cast<float*>(a->workspace);
  const dim3 grid((unsigned)pl.n_slabs), block(LD_WAVES * 64);
  const bool drop = a->p != 0.0;
#define LD_BWD(U)                                                                                              \
  do {                                                                                                         \
    if (drop) hipLaunchKernelGGL((lora_down_bwd_kernel<U, true>), grid, block, 0, st, d, u0, pl.slab_len, ws); \
    else hipLaunchKernelGGL((lora_down_bwd_kernel<U, false>), grid, block, 0, st, d, u0, pl.slab_len, ws);     \
  } while (0)
  for (int u0 = 0; u0 < d.total; u0 += LD_UNITS) {
    switch (std::min(LD_UNITS, d.total - u0)) {
      case 1: LD_BWD(1); break;
      case 2: LD_BWD(2); break;
      case 3: LD_BWD(3); break;
      default: LD_BWD(4); break;
    }
    GAD_LAUNCH_CHECK("lora_down_bwd_kernel");
  }
#undef LD_BWD
  const int64_t per = (int64_t)d.total * 16 * d.C;
  hipLaunchKernelGGL(lora_da_reduce_kernel, dim3((unsigned)gad_ceil_div(per, 256)), dim3(256), 0, st, d, ws, pl.n_slabs, a->dA[0],
                     a->dA[1], a->dA[2], a->dA[3]);
  GAD_LAUNCH_CHECK("lora_da_reduce_kernel");
  return 0;
}

extern "C" int gad_lora_merge(float* W, int64_t ldw, const float* B, const float* A, int32_t N, int32_t K, int32_t r, float alpha,
                              void* stream) {
  GAD_CHECK(W != nullptr && B != nullptr && A != nullptr, "gad_lora_merge: null pointer (W, B or A)");
  GAD_CHECK(N >= 1 && K >= 1 && r >= 1, "gad_lora_merge: N=%d, K=%d, r=%d must be >= 1", N, K, r);
  GAD_CHECK(ldw >= K, "gad_lora_merge: ldw=%lld below K=%d", (long long)ldw, K);
  hipLaunchKernelGGL(lora_merge_kernel, dim3((unsigned)gad_ceil_div((int64_t)N * K, 256)), dim3(256), 0, static_cast<hipStream_t>(stream), W,
                     ldw, B, A, N, K, r, alpha);
  GAD_LAUNCH_CHECK("lora_merge_kernel");
  return 0;
}
