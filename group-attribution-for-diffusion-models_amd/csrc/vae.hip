// Autoencoders (gad/vae.py: AutoencoderKL, VQModel).  Their convolutions, norms and attention run on gad_gemm,
// gad_groupnorm_silu_fwd and the attention kernels; the one operator of their own is VQModel's codebook lookup
// (diffusers VectorQuantizer.forward: argmin over torch.cdist(z, embedding), then z + (z_q - z).detach()).
//
//   gad_vq_lookup   per latent row z[D]: idx = argmin_k sum_c (z_c - e[k][c])^2, zq = z + (e[idx] - z)
//
// One thread per row, the row in registers; the codebook streams through LDS in chunks of at most CHUNK floats (the CelebA
// codebook, 8192 x 3 floats = 96 KB, is two: a single 96 KB chunk would leave a CU one two-wave workgroup) and every lane
// of a wave reads the same code at the same time - a broadcast read, no bank conflicts.  The distance is the exact-difference form summed in channel order, multiply and add
// unfused (contraction is off), so it is the same fp32 number torch gives for ((z - e) ** 2).sum(-1) on these rows.  Codes
// are scanned in increasing k with a strict <: ties go to the lowest index, and a row holding a NaN (no distance compares
// below anything) keeps index 0.  No atomics, no cross-thread reduction: the result does not depend on the launch shape.
#include <math.h>

#include "gad_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int NT = 128;
constexpr int CHUNK = 12288;      // floats of codebook per LDS chunk: 48 KB - three workgroups per CU, under the 64 KB default limit

template <int D>
__global__ __launch_bounds__(NT) void vq_lookup_kernel(const float* __restrict__ z, int64_t ldz, const float* __restrict__ e,
                                                       int64_t n, int K, int codes_per_chunk, int* __restrict__ idx,
                                                       float* __restrict__ zq, int64_t ldzq) {
  extern __shared__ __attribute__((aligned(16))) float cb[];
  const int64_t row = (int64_t)blockIdx.x * NT + threadIdx.x;
  const bool live = row < n;
  float zr[D];
#pragma unroll
  for (int c = 0; c < D; ++c) zr[c] = live ? z[row * ldz + c] : 0.f;
  float best = INFINITY;
  int arg = 0;
  for (int k0 = 0; k0 < K; k0 += codes_per_chunk) {
    const int nk = min(codes_per_chunk, K - k0);
    if (k0) __syncthreads();                                    // every lane is done with the previous chunk
    for (int i = threadIdx.x; i < nk * D; i += NT) cb[i] = e[(int64_t)k0 * D + i];
    __syncthreads();
    for (int k = 0; k < nk; ++k) {
      float dist = 0.f;
#pragma unroll
      for (int c = 0; c < D; ++c) {
        const float df = zr[c] - cb[k * D + c];
        dist += df * df;
      }
      if (dist < best) { best = dist; arg = k0 + k; }
    }
  }
  if (!live) return;
  idx[row] = arg;
#pragma unroll
  for (int c = 0; c < D; ++c) zq[row * ldzq + c] = zr[c] + (e[(int64_t)arg * D + c] - zr[c]);
}

template <int D>
int launch_vq(const float* z, int64_t ldz, const float* e, int64_t n, int K, int* idx, float* zq, int64_t ldzq, hipStream_t st) {
  const int cpc = CHUNK / D;
  const int bytes = (K < cpc ? K : cpc) * D * (int)sizeof(float);
  const dim3 grid((unsigned)gad_ceil_div(n, NT));
  hipLaunchKernelGGL((vq_lookup_kernel<D>), grid, dim3(NT), bytes, st, z, ldz, e, n, K, cpc, idx, zq, ldzq);
  return 0;
}

}  // namespace

#define GAD_VQ_DIMS(X) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13) X(14) X(15) X(16)

extern "C" int gad_vq_lookup(const float* z, int64_t ldz, const float* e, int64_t n, int32_t K, int32_t D, int32_t* idx,
                             float* zq, int64_t ldzq, void* stream) {
  const char* who = "gad_vq_lookup";
  GAD_CHECK(D >= 1 && D <= 16, "%s: code dim D=%d is outside 1..16", who, D);
  GAD_CHECK(K >= 1, "%s: codebook size K=%d must be at least 1", who, K);
  GAD_CHECK(n >= 0 && gad_ceil_div(n, NT) < (1L << 31), "%s: bad row count n=%lld", who, (long long)n);
  GAD_CHECK(ldz >= D && ldzq >= D, "%s: a row stride (ldz=%lld, ldzq=%lld) is smaller than D=%d", who, (long long)ldz, (long long)ldzq, D);
  if (n == 0) return 0;
  GAD_CHECK(z && e && idx && zq, "%s: null pointer", who);
  int rc = 1;
  switch (D) {
#define X(DIM) case DIM: rc = launch_vq<DIM>(z, ldz, e, n, K, idx, zq, ldzq, (hipStream_t)stream); break;
    GAD_VQ_DIMS(X)
#undef X
  }
  if (rc) return rc;
  GAD_LAUNCH_CHECK(who);
  return 0;
}
