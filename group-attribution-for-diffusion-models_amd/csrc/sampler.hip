// The scheduler updates of the samplers, one streaming pass each over the latents (gfx950): DDIM (eta = 0) with and without
// classifier-free guidance, the ancestral DDPM step with in-kernel variance noise, and the PLMS step of PNDM.  They share the
// x0 prediction, the guidance combination, the float4 operand checks and the streaming grid rule; each keeps its own expression
// for x_prev (DDIM's  spa x0 + spb eps  and PLMS's  cs x - cm m  are the same function but not the same bits).
//
// gad_ddim_step / gad_cfg_ddim_step: n contiguous floats.  Element i:
//   eps    = eps_u + g (eps_c - eps_u)                 (guided; eps_c = eps_uc + n)
//   x0     = (x - sqrt(1 - abar_t) eps) / sqrt(abar_t), clamped to +-clip when clip > 0
//   x_prev = sqrt(abar_prev) x0 + sqrt(1 - abar_prev) eps
//
// gad_ddpm_step (diffusers DDPMScheduler.step, epsilon prediction, fixed_small / fixed_large variance; the Journey-TRAK
// trajectory generator, gad/trak.py): x and eps are B rows of n contiguous floats.  Element e of row b:
//   x0 as above
//   mean   = c0 x0 + c1 x        c0 = sqrt(abar_prev) (1 - cur_alpha) / (1 - abar_t),  cur_alpha = abar_t / abar_prev
//                                c1 = sqrt(cur_alpha) (1 - abar_prev) / (1 - abar_t)
//   x_prev = mean + sigma z      for t > 0;  x_prev = mean for t == 0 (Philox is not called)
// z is never stored: it is word e & 3 of Philox-4x32-10 with key (seeds[b] low word, high word) and counter (e >> 2, t, 0, 2)
// through the projector's uniform and Box-Muller maps (jl_normal4 in gad_dev.h).  A lane owns one float4, i.e. one Philox
// block, so a row's result depends on (its seed, t, its own elements) only - not on B, on its position or on the grid.
// The coefficients are formed in fp64 on the host and rounded once.  12 B of traffic per element, no workspace, no atomics.
//
// gad_plms_step (diffusers PNDMScheduler.step_plms, epsilon prediction, skip_prk_steps): guidance, the linear-multistep
// combination of the stored noise predictions, the transfer to the previous timestep, and the two pieces of scheduler state
// that live on the device (the prediction pushed into the history ring, the sample remembered by the first step).  All
// operands are n contiguous floats.  Element i:
//   e      = eps_u + g (eps_c - eps_u)                (eps_c == NULL: e = eps_u)
//   m      = w0 e + w1 h1 + w2 h2 + w3 h3             (h1 the newest stored prediction; a NULL h_i is not read)
//   x_prev = cs xs - cm m                             (xs = x, or x_saved under GAD_PLMS_USE_SAVED; x is then not read)
//   push[i]    = e                                    (push != NULL)
//   x_saved[i] = x                                    (GAD_PLMS_SAVE)
// A lane reads every operand of its float4 before it writes any, and no lane touches another lane's elements, so x_prev may be
// x (in place) and push may be any of the h_i (a three-slot ring: the oldest slot is read, then overwritten).  The six
// coefficients arrive as fp64 and are rounded once to fp32.  The kernel is instantiated on the number of history terms and on
// guidance, so an absent term costs no load: 12 B per element on the first step, 32 B (24 read, 8 written) on a guided
// four-term step.  No workspace, no atomics, no host sync.
#include <math.h>

#include "gad_dev.h"

namespace {

constexpr int NT = 256;

__device__ __forceinline__ float predict_x0(float x, float eps, float sa, float sb, float clip) {
  float x0 = (x - sb * eps) / sa;
  if (clip > 0.f) x0 = fminf(fmaxf(x0, -clip), clip);
  return x0;
}
__device__ __forceinline__ float guided_eps(float u, float c, float g) { return u + g * (c - u); }

__device__ __forceinline__ float ddim_update(float x, float eps, float sa, float sb, float spa, float spb, float clip) {
  return spa * predict_x0(x, eps, sa, sb, clip) + spb * eps;
}

// x / xp are NOT restrict-qualified: the samplers launch this in place (xp == x).  Unguided: eps = eu, and ec / gd are not read.
template <bool GUIDED>
__global__ void ddim_step_kernel(const float* x, const float* __restrict__ eu, const float* __restrict__ ec, float* xp, long n,
                                 float gd, float sa, float sb, float spa, float spb, float clip) {
  const long nv = n >> 2, gs = (long)gridDim.x * blockDim.x;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += gs) {
    const f32x4 v = reinterpret_cast<const f32x4*>(x)[i];
    f32x4 e4 = reinterpret_cast<const f32x4*>(eu)[i], o;
    if constexpr (GUIDED) {
      const f32x4 c = reinterpret_cast<const f32x4*>(ec)[i];
#pragma unroll
      for (int e = 0; e < 4; ++e) e4[e] = guided_eps(e4[e], c[e], gd);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = ddim_update(v[e], e4[e], sa, sb, spa, spb, clip);
    reinterpret_cast<f32x4*>(xp)[i] = o;
  }
  for (long i = (n & ~3L) + (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gs) {   // n % 4 tail
    float eps = eu[i];
    if constexpr (GUIDED) eps = guided_eps(eps, ec[i], gd);
    xp[i] = ddim_update(x[i], eps, sa, sb, spa, spb, clip);
  }
}

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
        const float mean = c0 * predict_x0(v[e], e4[e], sa, sb, clip) + c1 * v[e];
        o[e] = NOISE ? mean + sigma * z[e] : mean;
      }
      pr[i] = o;
    }
  }
}

// only eps_u / eps_c are restrict-qualified: x_prev may alias x, push may alias a history slot, x_saved is read or written
template <int NH, bool GUIDED>
__global__ __launch_bounds__(NT) void plms_step_kernel(const float* x, const float* __restrict__ eu, const float* __restrict__ ec,
                                                       const float* h1, const float* h2, const float* h3, float* push,
                                                       float* x_saved, int saved_mode, float* xp, long nv, float g, float cs,
                                                       float cm, float w0, float w1, float w2, float w3) {
  const long gs = (long)gridDim.x * NT;
  for (long i = (long)blockIdx.x * NT + threadIdx.x; i < nv; i += gs) {
    f32x4 e4 = reinterpret_cast<const f32x4*>(eu)[i];
    if constexpr (GUIDED) {
      const f32x4 c4 = reinterpret_cast<const f32x4*>(ec)[i];
#pragma unroll
      for (int k = 0; k < 4; ++k) e4[k] = guided_eps(e4[k], c4[k], g);
    }
    const f32x4 xs = saved_mode == GAD_PLMS_USE_SAVED ? reinterpret_cast<const f32x4*>(x_saved)[i]
                                                      : reinterpret_cast<const f32x4*>(x)[i];
    f32x4 m;
#pragma unroll
    for (int k = 0; k < 4; ++k) m[k] = w0 * e4[k];
    if constexpr (NH >= 1) {
      const f32x4 a = reinterpret_cast<const f32x4*>(h1)[i];
#pragma unroll
      for (int k = 0; k < 4; ++k) m[k] += w1 * a[k];
    }
    if constexpr (NH >= 2) {
      const f32x4 a = reinterpret_cast<const f32x4*>(h2)[i];
#pragma unroll
      for (int k = 0; k < 4; ++k) m[k] += w2 * a[k];
    }
    if constexpr (NH >= 3) {
      const f32x4 a = reinterpret_cast<const f32x4*>(h3)[i];
#pragma unroll
      for (int k = 0; k < 4; ++k) m[k] += w3 * a[k];
    }
    f32x4 o;
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = cs * xs[k] - cm * m[k];
    // every load of this lane is above, every store below
    if (push != nullptr) reinterpret_cast<f32x4*>(push)[i] = e4;
    if (saved_mode == GAD_PLMS_SAVE) reinterpret_cast<f32x4*>(x_saved)[i] = xs;
    reinterpret_cast<f32x4*>(xp)[i] = o;
  }
}

template <int NH>
void plms_launch(bool guided, dim3 grid, hipStream_t st, const float* x, const float* eu, const float* ec, const float* h1,
                 const float* h2, const float* h3, float* push, float* x_saved, int saved_mode, float* xp, long nv, float g,
                 float cs, float cm, float w0, float w1, float w2, float w3) {
  if (guided)
    hipLaunchKernelGGL((plms_step_kernel<NH, true>), grid, dim3(NT), 0, st, x, eu, ec, h1, h2, h3, push, x_saved, saved_mode, xp,
                       nv, g, cs, cm, w0, w1, w2, w3);
  else
    hipLaunchKernelGGL((plms_step_kernel<NH, false>), grid, dim3(NT), 0, st, x, eu, ec, h1, h2, h3, push, x_saved, saved_mode, xp,
                       nv, g, cs, cm, w0, w1, w2, w3);
}

// A float4 operand of entry point `fn`: read or written 16 B per lane.  An optional one may be NULL (NULL counts as aligned).
// The entry points refuse every NULL before any misalignment, so the two checks are two passes over the operand list.
struct F4Operand {
  const char* name;
  const void* p;
  bool required;
};
template <size_t N>
int f4_null(const char* fn, const F4Operand (&ops)[N]) {
  for (const F4Operand& o : ops) GAD_CHECK(o.p != nullptr || !o.required, "%s: null pointer %s", fn, o.name);
  return 0;
}
template <size_t N>
int f4_misaligned(const char* fn, const F4Operand (&ops)[N]) {
  for (const F4Operand& o : ops) GAD_CHECK(gad_aligned16(o.p), "%s: %s must be 16-B aligned (misaligned pointer)", fn, o.name);
  return 0;
}

}  // namespace

#define ST ((hipStream_t)stream)

extern "C" int gad_ddim_step(const float* x, const float* eps, float* x_prev, int64_t n, float alpha_t, float alpha_prev,
                             float clip, void* stream) {
  const F4Operand ops[] = {{"x", x, true}, {"eps", eps, true}, {"x_prev", x_prev, true}};
  if (f4_null("gad_ddim_step", ops) || f4_misaligned("gad_ddim_step", ops)) return 1;
  GAD_CHECK(alpha_t > 0.f && alpha_t <= 1.f && alpha_prev > 0.f && alpha_prev <= 1.f, "gad_ddim_step: alphas out of (0,1]");
  const int64_t nv = n / 4;
  hipLaunchKernelGGL(ddim_step_kernel<false>, dim3(gad_stream_grid(nv > 0 ? nv : 1)), dim3(NT), 0, ST, x, eps, nullptr, x_prev,
                     (long)n, 0.f, sqrtf(alpha_t), sqrtf(1.f - alpha_t), sqrtf(alpha_prev), sqrtf(1.f - alpha_prev), clip);
  GAD_LAUNCH_CHECK("gad_ddim_step");
  return 0;
}

extern "C" int gad_cfg_ddim_step(const float* x, const float* eps_uc, float* x_prev, int64_t n, float guidance, float alpha_t,
                                 float alpha_prev, float clip, void* stream) {
  const F4Operand ops[] = {{"x", x, true}, {"eps_uc", eps_uc, true}, {"x_prev", x_prev, true}};
  if (f4_null("gad_cfg_ddim_step", ops) || f4_misaligned("gad_cfg_ddim_step", ops)) return 1;
  GAD_CHECK(n > 0 && n % 4 == 0, "gad_cfg_ddim_step: bad args (n must be a multiple of 4)");
  GAD_CHECK(alpha_t > 0.f && alpha_t <= 1.f && alpha_prev > 0.f && alpha_prev <= 1.f, "gad_cfg_ddim_step: alphas out of (0,1]");
  hipLaunchKernelGGL(ddim_step_kernel<true>, dim3(gad_stream_grid(n / 4)), dim3(NT), 0, ST, x, eps_uc, eps_uc + n, x_prev, (long)n,
                     guidance, sqrtf(alpha_t), sqrtf(1.f - alpha_t), sqrtf(alpha_prev), sqrtf(1.f - alpha_prev), clip);
  GAD_LAUNCH_CHECK("gad_cfg_ddim_step");
  return 0;
}

extern "C" int gad_ddpm_step(const float* x, const float* eps, float* x_prev, int32_t B, int64_t n, const int64_t* seeds,
                             int32_t t, float alpha_t, float alpha_prev, float clip, int32_t variance_type, void* stream) {
  const F4Operand ops[] = {{"x", x, true}, {"eps", eps, true}, {"x_prev", x_prev, true}};
  if (f4_null("gad_ddpm_step", ops)) return 1;
  GAD_CHECK(seeds != nullptr, "gad_ddpm_step: null pointer seeds");
  if (f4_misaligned("gad_ddpm_step", ops)) return 1;
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
  const dim3 grid = gad_stream_grid_rows(B, nv);
  if (t > 0)
    hipLaunchKernelGGL(ddpm_step_kernel<true>, grid, dim3(NT), 0, ST, x, eps, x_prev, B, nv, seeds, (uint32_t)t, sa, sb, (float)c0,
                       (float)c1, (float)sqrt(var), clip);
  else
    hipLaunchKernelGGL(ddpm_step_kernel<false>, grid, dim3(NT), 0, ST, x, eps, x_prev, B, nv, seeds, 0u, sa, sb, (float)c0,
                       (float)c1, 0.f, clip);
  GAD_LAUNCH_CHECK("gad_ddpm_step");
  return 0;
}

extern "C" int gad_plms_step(const float* x, const float* eps_u, const float* eps_c, float guidance, const float* h1,
                             const float* h2, const float* h3, float* push, float* x_saved, int32_t saved_mode, float* x_prev,
                             int64_t n, double cs, double cm, double w0, double w1, double w2, double w3, void* stream) {
  // x_saved counts as an operand only under a mode that touches it; its NULL has a message of its own below
  const F4Operand ops[] = {{"x", x, true},       {"eps_u", eps_u, true}, {"eps_c", eps_c, false},
                           {"h1", h1, false},    {"h2", h2, false},      {"h3", h3, false},
                           {"push", push, false}, {"x_saved", saved_mode == GAD_PLMS_SAVED_NONE ? nullptr : x_saved, false},
                           {"x_prev", x_prev, true}};
  if (f4_null("gad_plms_step", ops)) return 1;
  GAD_CHECK(saved_mode == GAD_PLMS_SAVED_NONE || saved_mode == GAD_PLMS_SAVE || saved_mode == GAD_PLMS_USE_SAVED,
            "gad_plms_step: unknown saved_mode %d", saved_mode);
  GAD_CHECK(saved_mode == GAD_PLMS_SAVED_NONE || x_saved != nullptr, "gad_plms_step: null pointer x_saved with saved_mode %d",
            saved_mode);
  GAD_CHECK(h1 != nullptr || h2 == nullptr, "gad_plms_step: h2 without h1 (the history terms are a prefix)");
  GAD_CHECK(h2 != nullptr || h3 == nullptr, "gad_plms_step: h3 without h2 (the history terms are a prefix)");
  if (f4_misaligned("gad_plms_step", ops)) return 1;
  GAD_CHECK(n >= 4 && n % 4 == 0, "gad_plms_step: n=%lld must be a positive multiple of 4 (one float4 per lane)", (long long)n);
  // x_prev may be x and nothing else; the state written beside it must be its own memory
  GAD_CHECK(x_prev != eps_u && x_prev != eps_c && x_prev != h1 && x_prev != h2 && x_prev != h3,
            "gad_plms_step: x_prev aliases eps or a history slot (only x_prev == x is allowed)");
  GAD_CHECK(push == nullptr || (push != x_prev && push != x && push != eps_u && push != eps_c),
            "gad_plms_step: push aliases x, x_prev or eps");
  GAD_CHECK(saved_mode == GAD_PLMS_SAVED_NONE || (x_saved != x_prev && x_saved != push && x_saved != x),
            "gad_plms_step: x_saved aliases x, x_prev or push");
  const float csf = (float)cs, cmf = (float)cm, wf[4] = {(float)w0, (float)w1, (float)w2, (float)w3};
  GAD_CHECK(isfinite(cs) && isfinite(csf) && cs > 0.0, "gad_plms_step: cs=%g must be finite and > 0", cs);
  GAD_CHECK(isfinite(cm) && isfinite(cmf), "gad_plms_step: cm=%g must be finite", cm);
  GAD_CHECK(isfinite(w0) && isfinite(wf[0]), "gad_plms_step: w0=%g must be finite", w0);
  GAD_CHECK(isfinite(w1) && isfinite(wf[1]), "gad_plms_step: w1=%g must be finite", w1);
  GAD_CHECK(isfinite(w2) && isfinite(wf[2]), "gad_plms_step: w2=%g must be finite", w2);
  GAD_CHECK(isfinite(w3) && isfinite(wf[3]), "gad_plms_step: w3=%g must be finite", w3);
  GAD_CHECK(h1 != nullptr || w1 == 0.0, "gad_plms_step: w1=%g with a null h1 (an absent term has weight 0)", w1);
  GAD_CHECK(h2 != nullptr || w2 == 0.0, "gad_plms_step: w2=%g with a null h2 (an absent term has weight 0)", w2);
  GAD_CHECK(h3 != nullptr || w3 == 0.0, "gad_plms_step: w3=%g with a null h3 (an absent term has weight 0)", w3);
  GAD_CHECK(eps_c == nullptr || isfinite(guidance), "gad_plms_step: guidance=%g must be finite", (double)guidance);

  const long nv = (long)(n / 4);
  const dim3 grid(gad_stream_grid(nv));
  const bool guided = eps_c != nullptr;
  const int nh = h3 ? 3 : h2 ? 2 : h1 ? 1 : 0;
#define GAD_PLMS_ARGS guided, grid, ST, x, eps_u, eps_c, h1, h2, h3, push, x_saved, saved_mode, x_prev, nv, guidance, csf, cmf, wf[0], wf[1], wf[2], wf[3]
  switch (nh) {
    case 0: plms_launch<0>(GAD_PLMS_ARGS); break;
    case 1: plms_launch<1>(GAD_PLMS_ARGS); break;
    case 2: plms_launch<2>(GAD_PLMS_ARGS); break;
    default: plms_launch<3>(GAD_PLMS_ARGS); break;
  }
#undef GAD_PLMS_ARGS
  GAD_LAUNCH_CHECK("gad_plms_step");
  return 0;
}
