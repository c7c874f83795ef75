// Ancestral DDPM update x_t -> x_{t-1} (diffusers DDPMScheduler.step, epsilon prediction, fixed_small / fixed_large variance)
// in one pass, with the variance noise generated in the kernel: the Journey-TRAK trajectory generator (gad/trak.py).
//
// x and eps are B rows of n contiguous floats.  Element e of row b:
//   x0     = (x - sqrt(1 - abar_t) eps) / sqrt(abar_t), clamped to +-clip when clip > 0
//   mean   = c0 x0 + c1 x        c0 = sqrt(abar_prev) (1 - cur_alpha) / (1 - abar_t),  cur_alpha = abar_t / abar_prev
//                                c1 = sqrt(cur_alpha) (1 - abar_prev) / (1 - abar_t)
//   x_prev = mean + sigma z      for t > 0;  x_prev = mean for t == 0 (Philox is not called)
// z is never stored: it is word e & 3 of Philox-4x32-10 with key (seeds[b] low word, high word) and counter (e >> 2, t, 0, 2)
// through the projector's uniform and Box-Muller maps (jl_normal4 in gad_dev.h).  A lane owns one float4, i.e. one Philox
// block, so a row's result depends on (its seed, t, its own elements) only - not on B, on its position or on the grid.
// The coefficients are formed in fp64 on the host and rounded once.  12 B of traffic per element, no workspace, no atomics.
#include "gad_dev.h"

namespace {

constexpr int NT = 256;
constexpr int MAX_BLOCKS = 2048;     // 8 workgroups per CU, as the other streaming kernels

// x / xp are NOT restrict-qualified: the trajectory generator may launch this in place (xp == x)
template <bool NOISE>
__global__ __launch_bounds__(NT) void ddpm_step_kernel(const float* x, const float* __restrict__ eps, float* xp, int B, long nv,
                                                       const int64_t* __restrict__ seeds, uint32_t t, float sa, float sb,
                                                       float c0, float c1, float sigma, float clip) {
  const long gs = (long)gridDim.x * NT;
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    const f32x4* xr = reinterpret_cast<const f32x4*>(x) + (long)b * nv;
    const f32x4* er = reinterpret_cast<const f32x4*>(eps) + (long)b * nv;
    f32x4* pr = reinterpret_cast<f32x4*>(xp) + (long)b * nv;
    uint32_t k0 = 0, k1 = 0;
    if constexpr (NOISE) {
      const uint64_t s = (uint64_t)seeds[b];
      k0 = (uint32_t)s;
      k1 = (uint32_t)(s >> 32);
    }
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < nv; i += gs) {
      const f32x4 v = xr[i], e4 = er[i];
      float z[4] = {0.f, 0.f, 0.f, 0.f};
      if constexpr (NOISE) jl_normal4(philox4x32_10(make_uint4((uint32_t)i, t, 0u, 2u), k0, k1), z);
      f32x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float x0 = (v[e] - sb * e4[e]) / sa;
        if (clip > 0.f) x0 = fminf(fmaxf(x0, -clip), clip);
        const float mean = c0 * x0 + c1 * v[e];
        o[e] = NOISE ? mean + sigma * z[e] : mean;
      }
      pr[i] = o;
    }
  }
}

}  // namespace

extern "C" int gad_ddpm_step(const float* x, const float* eps, float* x_prev, int32_t B, int64_t n, const int64_t* seeds,
                             int32_t t, float alpha_t, float alpha_prev, float clip, int32_t variance_type, void* stream) {
  GAD_CHECK(x != nullptr, "gad_ddpm_step: null pointer x");
  GAD_CHECK(eps != nullptr, "gad_ddpm_step: null pointer eps");
  GAD_CHECK(x_prev != nullptr, "gad_ddpm_step: null pointer x_prev");
  GAD_CHECK(seeds != nullptr, "gad_ddpm_step: null pointer seeds");
  GAD_CHECK(gad_aligned16(x), "gad_ddpm_step: x must be 16-B aligned (misaligned pointer)");
  GAD_CHECK(gad_aligned16(eps), "gad_ddpm_step: eps must be 16-B aligned (misaligned pointer)");
  GAD_CHECK(gad_aligned16(x_prev), "gad_ddpm_step: x_prev must be 16-B aligned (misaligned pointer)");
  GAD_CHECK((reinterpret_cast<uintptr_t>(seeds) & 7) == 0, "gad_ddpm_step: seeds must be 8-B aligned (misaligned pointer)");
  GAD_CHECK(B >= 1, "gad_ddpm_step: B=%d must be >= 1", B);
  GAD_CHECK(n >= 4 && n % 4 == 0, "gad_ddpm_step: n=%lld must be a positive multiple of 4 (one float4 per lane)", (long long)n);
  GAD_CHECK(n / 4 <= (int64_t)1 << 32, "gad_ddpm_step: n=%lld exceeds the 32-bit block counter (n / 4 <= 2^32)", (long long)n);
  GAD_CHECK(t >= 0, "gad_ddpm_step: t=%d must be >= 0", t);
  GAD_CHECK(alpha_t > 0.f && alpha_t <= 1.f, "gad_ddpm_step: alpha_t=%g out of (0,1]", (double)alpha_t);
  GAD_CHECK(alpha_prev > 0.f && alpha_prev <= 1.f, "gad_ddpm_step: alpha_prev=%g out of (0,1]", (double)alpha_prev);
  GAD_CHECK(alpha_prev >= alpha_t, "gad_ddpm_step: alpha_prev=%g below alpha_t=%g", (double)alpha_prev, (double)alpha_t);
  GAD_CHECK(variance_type == GAD_DDPM_FIXED_SMALL || variance_type == GAD_DDPM_FIXED_LARGE,
            "gad_ddpm_step: unknown variance_type %d", variance_type);
  GAD_CHECK(clip >= 0.f, "gad_ddpm_step: clip=%g must be >= 0 (0: no clipping)", (double)clip);

  const double a_t = alpha_t, a_p = alpha_prev;
  const double cur_alpha = a_t / a_p, cur_beta = 1.0 - cur_alpha;
  const double c0 = sqrt(a_p) * cur_beta / (1.0 - a_t), c1 = sqrt(cur_alpha) * (1.0 - a_p) / (1.0 - a_t);
  double var = cur_beta;
  if (variance_type == GAD_DDPM_FIXED_SMALL) var = fmax((1.0 - a_p) / (1.0 - a_t) * cur_beta, 1e-20);
  const float sa = (float)sqrt(a_t), sb = (float)sqrt(1.0 - a_t);

  const long nv = (long)(n / 4);
  const int64_t gx = std::min<int64_t>(gad_ceil_div(nv, NT), MAX_BLOCKS);
  const int64_t gy = std::min<int64_t>(B, std::max<int64_t>(1, MAX_BLOCKS / gx));
  const dim3 grid((unsigned)gx, (unsigned)gy);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (t > 0)
    hipLaunchKernelGGL(ddpm_step_kernel<true>, grid, dim3(NT), 0, st, x, eps, x_prev, B, nv, seeds, (uint32_t)t, sa, sb, (float)c0,
                       (float)c1, (float)sqrt(var), clip);
  else
    hipLaunchKernelGGL(ddpm_step_kernel<false>, grid, dim3(NT), 0, st, x, eps, x_prev, B, nv, seeds, 0u, sa, sb, (float)c0,
                       (float)c1, 0.f, clip);
  GAD_LAUNCH_CHECK("gad_ddpm_step");
  return 0;
}
