// Johnson-Lindenstrauss projection out = A R with R generated on the fly (TRAK / D-TRAK gradient features).
//
// R(row, j) comes from Philox-4x32-10 (key = (seed, model_id), counter = (column block, row lo, row hi, type)); see
// include/gad.h for the two entry maps.  One wave owns a 64-column tile of R and a slab of P; per 16 rows of its slab
// every lane makes four Philox calls (its four rows) and feeds 4 x MB v_mfma_f32_16x16x4_f32 per call.  The generator is
// VALU work (integer multiplies, Box-Muller), the products are MFMA work: the four calls of a 16-row step are unrolled
// next to the MFMAs that consume them, and 2-4 resident waves per SIMD fill each other's gaps.
//
// Lane l (kq = l >> 4, j = l & 15) of a wave, M block m, step s in 0..3 of a 16-row chunk at p:
//   A operand  A[g0 + 16m + j][p + 4kq + s]         (one float4 load per lane per chunk per M block)
//   B operand  R(p0 + p + 4kq + s, column(t, j))     t = 0..3: the wave's four 16-column MFMA tiles
//   normal:     column(t, j) = 64 ct + 4j + t         (Philox column block 16 ct + j, word t)
//   rademacher: column(t, j) = 64 ct + 16t + j        (Philox column block ct / 2, word 2 (ct & 1) + t / 2, bit 16 (t & 1) + j)
// so the k index of the MFMA is the slab row p + 4kq + s on both operands.  Each wave writes its slab's partial
// [G][d] product into the workspace; a second kernel adds the slabs in slab order (no atomics).
#include "gad_dev.h"

namespace {

constexpr int JL_COLS = 64;          // columns of R per wave
constexpr int JL_CHUNK = 16;         // P rows per step of a wave
constexpr int JL_WAVES = 4;          // waves per workgroup (consecutive slabs of one column tile)
constexpr int JL_GROWS = 64;         // rows of A per launch z index (4 M blocks of 16)
constexpr int64_t JL_TARGET_WAVES = 4096;   // 4 per SIMD on 256 CUs
constexpr int64_t JL_MIN_SLAB = 256;        // rows: below this the per-slab partials cost more than they split

struct Plan {
  int64_t slab_len;   // rows of P per slab (multiple of JL_CHUNK)
  int64_t n_slabs;
};

// depends on (P, d) only: the reduction order of a row is the same for every G
Plan jl_plan(int64_t P, int32_t d) {
  const int64_t n_ct = d / JL_COLS;
  int64_t want = gad_ceil_div(JL_TARGET_WAVES, n_ct);
  want = std::max<int64_t>(1, std::min<int64_t>(want, gad_ceil_div(P, JL_MIN_SLAB)));
  Plan pl;
  pl.slab_len = gad_ceil_div(gad_ceil_div(P, JL_CHUNK), want) * JL_CHUNK;
  pl.n_slabs = gad_ceil_div(P, pl.slab_len);
  return pl;
}

// the uniform map and the four normals of a Philox block: jl_uniform / jl_normal4 in gad_dev.h
template <int TYPE>
__device__ __forceinline__ void jl_entries(uint64_t row, uint32_t ct, int j, uint32_t k0, uint32_t k1, float b[4]) {
  if constexpr (TYPE == GAD_JL_NORMAL) {
    jl_normal4(philox4x32_10(make_uint4(ct * 16u + (uint32_t)j, (uint32_t)row, (uint32_t)(row >> 32), 0u), k0, k1), b);
  } else {
    const uint4 x = philox4x32_10(make_uint4(ct >> 1, (uint32_t)row, (uint32_t)(row >> 32), 1u), k0, k1);
    const uint32_t lo = (ct & 1) ? x.z : x.x, hi = (ct & 1) ? x.w : x.y;
    // bit b of the word -> sign bit of +-1.0f
    b[0] = __uint_as_float(0x3f800000u | ((lo << (31 - j)) & 0x80000000u));
    b[1] = __uint_as_float(0x3f800000u | ((lo << (15 - j)) & 0x80000000u));
    b[2] = __uint_as_float(0x3f800000u | ((hi << (31 - j)) & 0x80000000u));
    b[3] = __uint_as_float(0x3f800000u | ((hi << (15 - j)) & 0x80000000u));
  }
}

template <int MB, int TYPE>
__global__ __launch_bounds__(JL_WAVES * 64) void jl_project_kernel(const float* __restrict__ A, int64_t lda, int G, int64_t P,
                                                                   uint64_t p0, int d, uint32_t seed, uint32_t model_id,
                                                                   int64_t slab_len, int64_t n_slabs, float* __restrict__ ws) {
  const int lane = threadIdx.x & 63;
  const int64_t slab = (int64_t)blockIdx.y * JL_WAVES + (threadIdx.x >> 6);
  if (slab >= n_slabs) return;
  const uint32_t ct = blockIdx.x;
  const int g0 = blockIdx.z * JL_GROWS;
  const int j = lane & 15, kq = lane >> 4;
  const int64_t pb = slab * slab_len, pe = min(P, pb + slab_len);

  const float* arow[MB];
  bool gok[MB];
#pragma unroll
  for (int m = 0; m < MB; ++m) {
    const int g = g0 + 16 * m + j;
    gok[m] = g < G;
    arow[m] = A + (int64_t)(gok[m] ? g : 0) * lda;
  }
  f32x4 acc[MB][4];
#pragma unroll
  for (int m = 0; m < MB; ++m)
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[m][t] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int64_t p = pb; p < pe; p += JL_CHUNK) {
    const int64_t pr = p + 4 * kq;         // this lane's rows pr .. pr+3 (pr is a multiple of 4, lda too: one float4)
    f32x4 a[MB];
#pragma unroll
    for (int m = 0; m < MB; ++m) {
      a[m] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (gok[m] && pr < P) {
        a[m] = *reinterpret_cast<const f32x4*>(arow[m] + pr);
        if (pr + 4 > P) {                  // the row's tail: entries at or past P are not part of A
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (pr + e >= P) a[m][e] = 0.f;
        }
      }
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      float b[4];
      jl_entries<TYPE>(p0 + (uint64_t)(pr + s), ct, j, seed, model_id, b);
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int m = 0; m < MB; ++m) acc[m][t] = mfma16(a[m][s], b[t], acc[m][t]);
    }
  }

  // C/D of 16x16x4: column lane & 15, row 4 (lane >> 4) + r
  float* wsl = ws + slab * (int64_t)G * d;
#pragma unroll
  for (int m = 0; m < MB; ++m)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int g = g0 + 16 * m + 4 * kq + r;
      if (g >= G) continue;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int col = JL_COLS * ct + (TYPE == GAD_JL_NORMAL ? 4 * j + t : 16 * t + j);
        wsl[(int64_t)g * d + col] = acc[m][t][r];
      }
    }
}

// out[i] (+)= sum over slabs in slab order
__global__ __launch_bounds__(256) void jl_reduce_kernel(const float* __restrict__ ws, int64_t n_slabs, int64_t n4,
                                                        float* __restrict__ out, int accumulate) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  const f32x4* w = reinterpret_cast<const f32x4*>(ws);
  f32x4 s = w[i];
  for (int64_t k = 1; k < n_slabs; ++k) s += w[k * n4 + i];
  f32x4* o = reinterpret_cast<f32x4*>(out);
  o[i] = accumulate ? o[i] + s : s;
}

int jl_validate(const gad_jl_args* a) {
  GAD_CHECK(a != nullptr, "gad_jl_project: null args");
  GAD_CHECK(a->G >= 1, "gad_jl_project: G=%d must be >= 1", a->G);
  GAD_CHECK(a->P >= 1, "gad_jl_project: P=%lld must be >= 1", (long long)a->P);
  GAD_CHECK(a->d >= JL_COLS && a->d % JL_COLS == 0, "gad_jl_project: d=%d must be a positive multiple of %d", a->d, JL_COLS);
  GAD_CHECK(a->lda >= a->P, "gad_jl_project: lda=%lld below P=%lld", (long long)a->lda, (long long)a->P);
  GAD_CHECK(a->lda % 4 == 0, "gad_jl_project: lda=%lld must be a multiple of 4 (float4 row loads)", (long long)a->lda);
  GAD_CHECK(a->p0 >= 0, "gad_jl_project: p0=%lld must be >= 0", (long long)a->p0);
  GAD_CHECK(a->type == GAD_JL_NORMAL || a->type == GAD_JL_RADEMACHER, "gad_jl_project: unknown projection type %d", a->type);
  return 0;
}

}  // namespace

extern "C" int64_t gad_jl_project_workspace_bytes(const gad_jl_args* a) {
  if (jl_validate(a) != 0) return -1;
  const Plan pl = jl_plan(a->P, a->d);
  return pl.n_slabs * (int64_t)a->G * a->d * (int64_t)sizeof(float);
}

extern "C" int gad_jl_project(const gad_jl_args* a, void* stream) {
  if (jl_validate(a) != 0) return 1;
  GAD_CHECK(a->A != nullptr && a->out != nullptr && a->workspace != nullptr, "gad_jl_project: null pointer (A, out or workspace)");
  GAD_CHECK(gad_aligned16(a->A) && gad_aligned16(a->out) && gad_aligned16(a->workspace),
            "gad_jl_project: A, out and workspace must be 16-B aligned (misaligned pointer)");
  const Plan pl = jl_plan(a->P, a->d);
  const int64_t need = pl.n_slabs * (int64_t)a->G * a->d * (int64_t)sizeof(float);
  GAD_CHECK(a->workspace_bytes >= need, "gad_jl_project: workspace_bytes=%lld < %lld", (long long)a->workspace_bytes,
            (long long)need);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid(a->d / JL_COLS, (unsigned)gad_ceil_div(pl.n_slabs, JL_WAVES), (unsigned)gad_ceil_div(a->G, JL_GROWS));
  const int gz = std::min(a->G, JL_GROWS);
  float* ws = static_cast<float*>(a->workspace);
#define JL_LAUNCH(MB, T)                                                                                                   \
  hipLaunchKernelGGL((jl_project_kernel<MB, T>), grid, dim3(JL_WAVES * 64), 0, st, a->A, a->lda, a->G, a->P,              \
                     (uint64_t)a->p0, a->d, a->seed, a->model_id, pl.slab_len, pl.n_slabs, ws)
  if (a->type == GAD_JL_NORMAL) {
    if (gz <= 16) JL_LAUNCH(1, GAD_JL_NORMAL);
    else if (gz <= 32) JL_LAUNCH(2, GAD_JL_NORMAL);
    else JL_LAUNCH(4, GAD_JL_NORMAL);
  } else {
    if (gz <= 16) JL_LAUNCH(1, GAD_JL_RADEMACHER);
    else if (gz <= 32) JL_LAUNCH(2, GAD_JL_RADEMACHER);
    else JL_LAUNCH(4, GAD_JL_RADEMACHER);
  }
#undef JL_LAUNCH
  GAD_LAUNCH_CHECK("jl_project_kernel");
  const int64_t n4 = (int64_t)a->G * a->d / 4;
  hipLaunchKernelGGL(jl_reduce_kernel, dim3((unsigned)gad_ceil_div(n4, 256)), dim3(256), 0, st, ws, pl.n_slabs, n4, a->out,
                     a->accumulate);
  GAD_LAUNCH_CHECK("jl_reduce_kernel");
  return 0;
}
