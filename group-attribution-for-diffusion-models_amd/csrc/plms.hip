// One PLMS step (diffusers PNDMScheduler.step_plms, epsilon prediction, skip_prk_steps) on the latents in one pass: guidance, the
// linear-multistep combination of the stored noise predictions, the transfer to the previous timestep, and the two pieces of
// scheduler state that live on the device (the prediction pushed into the history ring, the sample remembered by the first step).
//
// All operands are n contiguous floats.  Element i:
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

#include <algorithm>

#include "gad_dev.h"

namespace {

constexpr int NT = 256;
constexpr int MAX_BLOCKS = 2048;     // 8 workgroups per CU, as the other streaming kernels

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
      for (int k = 0; k < 4; ++k) e4[k] = e4[k] + g * (c4[k] - e4[k]);
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
void launch(bool guided, dim3 grid, hipStream_t st, const float* x, const float* eu, const float* ec, const float* h1,
            const float* h2, const float* h3, float* push, float* x_saved, int saved_mode, float* xp, long nv, float g, float cs,
            float cm, float w0, float w1, float w2, float w3) {
  if (guided)
    hipLaunchKernelGGL((plms_step_kernel<NH, true>), grid, dim3(NT), 0, st, x, eu, ec, h1, h2, h3, push, x_saved, saved_mode, xp,
                       nv, g, cs, cm, w0, w1, w2, w3);
  else
    hipLaunchKernelGGL((plms_step_kernel<NH, false>), grid, dim3(NT), 0, st, x, eu, ec, h1, h2, h3, push, x_saved, saved_mode, xp,
                       nv, g, cs, cm, w0, w1, w2, w3);
}

}  // namespace

extern "C" int gad_plms_step(const float* x, const float* eps_u, const float* eps_c, float guidance, const float* h1,
                             const float* h2, const float* h3, float* push, float* x_saved, int32_t saved_mode, float* x_prev,
                             int64_t n, double cs, double cm, double w0, double w1, double w2, double w3, void* stream) {
  GAD_CHECK(x != nullptr, "gad_plms_step: null pointer x");
  GAD_CHECK(eps_u != nullptr, "gad_plms_step: null pointer eps_u");
  GAD_CHECK(x_prev != nullptr, "gad_plms_step: null pointer x_prev");
  GAD_CHECK(saved_mode == GAD_PLMS_SAVED_NONE || saved_mode == GAD_PLMS_SAVE || saved_mode == GAD_PLMS_USE_SAVED,
            "gad_plms_step: unknown saved_mode %d", saved_mode);
  GAD_CHECK(saved_mode == GAD_PLMS_SAVED_NONE || x_saved != nullptr, "gad_plms_step: null pointer x_saved with saved_mode %d",
            saved_mode);
  GAD_CHECK(h1 != nullptr || h2 == nullptr, "gad_plms_step: h2 without h1 (the history terms are a prefix)");
  GAD_CHECK(h2 != nullptr || h3 == nullptr, "gad_plms_step: h3 without h2 (the history terms are a prefix)");
  GAD_CHECK(gad_aligned16(x), "gad_plms_step: x must be 16-B aligned (misaligned pointer)");
  GAD_CHECK(gad_aligned16(eps_u), "gad_plms_step: eps_u must be 16-B aligned (misaligned pointer)");
  GAD_CHECK(gad_aligned16(eps_c), "gad_plms_step: eps_c must be 16-B aligned (misaligned pointer)");
  GAD_CHECK(gad_aligned16(h1), "gad_plms_step: h1 must be 16-B aligned (misaligned pointer)");
  GAD_CHECK(gad_aligned16(h2), "gad_plms_step: h2 must be 16-B aligned (misaligned pointer)");
  GAD_CHECK(gad_aligned16(h3), "gad_plms_step: h3 must be 16-B aligned (misaligned pointer)");
  GAD_CHECK(gad_aligned16(push), "gad_plms_step: push must be 16-B aligned (misaligned pointer)");
  GAD_CHECK(saved_mode == GAD_PLMS_SAVED_NONE || gad_aligned16(x_saved),
            "gad_plms_step: x_saved must be 16-B aligned (misaligned pointer)");
  GAD_CHECK(gad_aligned16(x_prev), "gad_plms_step: x_prev must be 16-B aligned (misaligned pointer)");
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
  const dim3 grid((unsigned)std::min<int64_t>(gad_ceil_div(nv, NT), MAX_BLOCKS));
  hipStream_t st = static_cast<hipStream_t>(stream);
  const bool guided = eps_c != nullptr;
  const int nh = h3 ? 3 : h2 ? 2 : h1 ? 1 : 0;
#define GAD_PLMS_ARGS guided, grid, st, x, eps_u, eps_c, h1, h2, h3, push, x_saved, saved_mode, x_prev, nv, guidance, csf, cmf, wf[0], wf[1], wf[2], wf[3]
  switch (nh) {
    case 0: launch<0>(GAD_PLMS_ARGS); break;
    case 1: launch<1>(GAD_PLMS_ARGS); break;
    case 2: launch<2>(GAD_PLMS_ARGS); break;
    default: launch<3>(GAD_PLMS_ARGS); break;
  }
#undef GAD_PLMS_ARGS
  GAD_LAUNCH_CHECK("gad_plms_step");
  return 0;
}
