// The x0 rows of one Stable-Diffusion training step drawn from cached VAE posterior moments (gad/latents.py), and the
// uint8 -> fp32 NCHW pixel conversion that feeds the encoder when the cache is written (text_to_image/encode_dataset.py).
//
// gad_latent_draw: moments is [N][F][2][n] fp32 - per dataset row F slabs (the plain encode, then the encode of the mirrored
// image), per slab mean[n] then logvar[n].  Batch row b with r = rows[b] (clamped to [0, N)), element e:
//   coin = bit 0 of word 0 of Philox-4x32-10, key (seed low word, high word), counter (0xFFFFFFFF, r, step, 3)
//   f    = coin under GAD_LATENT_RANDOM_FLIP (F == 2), else 0;   m, lv = mean, logvar of slab (r, f) at e
//   x0   = scale * m                                              without GAD_LATENT_SAMPLE (the mode; Philox is not called for noise)
//   x0   = scale * (m + expf(0.5f * clamp(lv, -30, 20)) * z)      with it: z is word e & 3 of the block with counter (e >> 2, r, step, 3)
//          through the projector's uniform and Box-Muller maps (jl_normal4 in gad_dev.h)
// A lane owns one float4, i.e. one Philox block, and n / 4 < 2^32 - 1 keeps the coin's block index out of the noise's reach,
// so a row's result depends on (seed, r, step) only - not on B, on its position in the batch or on the grid.
// 12 B of traffic per element (mean and logvar read, x0 written; 8 B for the mode), no workspace, no atomics.
#include "gad_dev.h"

namespace {

constexpr int NT = 256;
constexpr uint32_t TAG = 3u;         // the projector uses 0 and 1, the DDPM step (sampler.hip) 2
constexpr uint32_t COIN_BLOCK = 0xFFFFFFFFu;

template <bool SAMPLE, bool FLIP>
__global__ __launch_bounds__(NT) void latent_draw_kernel(const float* __restrict__ moments, int64_t N, int F, long nv,
                                                         const int64_t* __restrict__ rows, int B, float* __restrict__ x0,
                                                         uint8_t* __restrict__ flipped, uint32_t k0, uint32_t k1, uint32_t step,
                                                         float scale) {
  const long gs = (long)gridDim.x * NT;
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    int64_t r = rows[b];
    r = r < 0 ? 0 : (r >= N ? N - 1 : r);
    const uint32_t r32 = (uint32_t)r;                                 // N < 2^32
    int f = 0;
    if constexpr (FLIP) f = (int)(philox4x32_10(make_uint4(COIN_BLOCK, r32, step, TAG), k0, k1).x & 1u);
    if (flipped != nullptr && blockIdx.x == 0 && threadIdx.x == 0) flipped[b] = (uint8_t)f;
    const f32x4* mr = reinterpret_cast<const f32x4*>(moments) + ((long)r * F + f) * 2 * nv;
    const f32x4* lr = mr + nv;
    f32x4* out = reinterpret_cast<f32x4*>(x0) + (long)b * nv;
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < nv; i += gs) {
      const f32x4 m = mr[i];
      f32x4 o;
      if constexpr (SAMPLE) {
        const f32x4 lv = lr[i];
        float z[4];
        jl_normal4(philox4x32_10(make_uint4((uint32_t)i, r32, step, TAG), k0, k1), z);
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = scale * (m[e] + expf(0.5f * fminf(fmaxf(lv[e], -30.f), 20.f)) * z[e]);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = scale * m[e];
      }
      out[i] = o;
    }
  }
}

// dst[b][c][h][w] = lut[src[b][h][flip ? W - 1 - w : w][c]]; VEC: one float4 of four consecutive w per lane (W % 4 == 0)
template <bool VEC>
__global__ __launch_bounds__(NT) void pixels_to_nchw_kernel(const uint8_t* __restrict__ src, float* __restrict__ dst, long total,
                                                            int H, int W, int Cn, const float* __restrict__ lut, int flip) {
  const long gs = (long)gridDim.x * NT;
  const int Wq = VEC ? W / 4 : W;                                      // lane items per output row
  for (long i = (long)blockIdx.x * NT + threadIdx.x; i < total; i += gs) {
    const int wq = (int)(i % Wq);
    long t = i / Wq;
    const int h = (int)(t % H);
    t /= H;
    const int c = (int)(t % Cn);
    const long b = t / Cn;
    const uint8_t* row = src + ((b * H + h) * (long)W) * Cn + c;
    if constexpr (VEC) {
      f32x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int w = wq * 4 + e;
        o[e] = lut[row[(long)(flip ? W - 1 - w : w) * Cn]];
      }
      reinterpret_cast<f32x4*>(dst)[i] = o;
    } else {
      dst[i] = lut[row[(long)(flip ? W - 1 - wq : wq) * Cn]];
    }
  }
}

}  // namespace

extern "C" int gad_latent_draw(const float* moments, int64_t N, int32_t F, int64_t n, const int64_t* rows, int32_t B, float* x0,
                               uint8_t* flipped, int64_t seed, uint32_t step, float scale, int32_t flags, void* stream) {
  GAD_CHECK(moments != nullptr, "gad_latent_draw: null pointer moments");
  GAD_CHECK(rows != nullptr, "gad_latent_draw: null pointer rows");
  GAD_CHECK(x0 != nullptr, "gad_latent_draw: null pointer x0");
  GAD_CHECK(gad_aligned16(moments), "gad_latent_draw: moments must be 16-B aligned (misaligned pointer)");
  GAD_CHECK(gad_aligned16(x0), "gad_latent_draw: x0 must be 16-B aligned (misaligned pointer)");
  GAD_CHECK((reinterpret_cast<uintptr_t>(rows) & 7) == 0, "gad_latent_draw: rows must be 8-B aligned (misaligned pointer)");
  GAD_CHECK(B >= 1, "gad_latent_draw: B=%d must be >= 1", B);
  GAD_CHECK(n >= 4 && n % 4 == 0, "gad_latent_draw: n=%lld must be a positive multiple of 4 (one float4 per lane)", (long long)n);
  GAD_CHECK(n / 4 < ((int64_t)1 << 32) - 1,
            "gad_latent_draw: n=%lld reaches the coin's block index (n / 4 < 2^32 - 1)", (long long)n);
  GAD_CHECK(N >= 1 && N < (int64_t)1 << 32, "gad_latent_draw: N=%lld must be in [1, 2^32) (the row is a 32-bit counter word)",
            (long long)N);
  GAD_CHECK(F == 1 || F == 2, "gad_latent_draw: F=%d must be 1 (plain) or 2 (plain | flipped)", F);
  GAD_CHECK((flags & ~(GAD_LATENT_SAMPLE | GAD_LATENT_RANDOM_FLIP)) == 0, "gad_latent_draw: unknown flag in flags=0x%x", flags);
  GAD_CHECK(!(flags & GAD_LATENT_RANDOM_FLIP) || F == 2,
            "gad_latent_draw: GAD_LATENT_RANDOM_FLIP needs the flipped slab (F=%d, expected 2)", F);

  const long nv = (long)(n / 4);
  const dim3 grid = gad_stream_grid_rows(B, nv);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const uint32_t k0 = (uint32_t)(uint64_t)seed, k1 = (uint32_t)((uint64_t)seed >> 32);
  const bool sample = flags & GAD_LATENT_SAMPLE, flip = flags & GAD_LATENT_RANDOM_FLIP;
#define GAD_LATENT_LAUNCH(S, FL) \
  hipLaunchKernelGGL((latent_draw_kernel<S, FL>), grid, dim3(NT), 0, st, moments, N, (int)F, nv, rows, (int)B, x0, flipped, k0, k1, step, scale)
  if (sample && flip) GAD_LATENT_LAUNCH(true, true);
  else if (sample) GAD_LATENT_LAUNCH(true, false);
  else if (flip) GAD_LATENT_LAUNCH(false, true);
  else GAD_LATENT_LAUNCH(false, false);
#undef GAD_LATENT_LAUNCH
  GAD_LAUNCH_CHECK("gad_latent_draw");
  return 0;
}

extern "C" int gad_pixels_to_nchw(const uint8_t* src, float* dst, int64_t B, int32_t H, int32_t W, int32_t C, const float* lut,
                                  int32_t flip, void* stream) {
  GAD_CHECK(src != nullptr, "gad_pixels_to_nchw: null pointer src");
  GAD_CHECK(dst != nullptr, "gad_pixels_to_nchw: null pointer dst");
  GAD_CHECK(lut != nullptr, "gad_pixels_to_nchw: null pointer lut");
  GAD_CHECK(gad_aligned16(dst), "gad_pixels_to_nchw: dst must be 16-B aligned (misaligned pointer)");
  GAD_CHECK((reinterpret_cast<uintptr_t>(lut) & 3) == 0, "gad_pixels_to_nchw: lut must be 4-B aligned (misaligned pointer)");
  GAD_CHECK(B >= 1 && H >= 1 && W >= 1 && C >= 1, "gad_pixels_to_nchw: B=%lld H=%d W=%d C=%d must all be >= 1", (long long)B, H, W,
            C);
  GAD_CHECK(flip == 0 || flip == 1, "gad_pixels_to_nchw: flip=%d must be 0 or 1", flip);
  GAD_CHECK(B <= (INT64_MAX / 4) / ((int64_t)H * W) / C, "gad_pixels_to_nchw: B=%lld x H=%d x W=%d x C=%d overflows", (long long)B,
            H, W, C);
  const bool vec = W % 4 == 0;
  const long total = (long)B * C * H * (vec ? W / 4 : W);
  const unsigned grid = gad_stream_grid(total);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (vec)
    hipLaunchKernelGGL(pixels_to_nchw_kernel<true>, dim3(grid), dim3(NT), 0, st, src, dst, total, (int)H, (int)W, (int)C, lut, (int)flip);
  else
    hipLaunchKernelGGL(pixels_to_nchw_kernel<false>, dim3(grid), dim3(NT), 0, st, src, dst, total, (int)H, (int)W, (int)C, lut, (int)flip);
  GAD_LAUNCH_CHECK("gad_pixels_to_nchw");
  return 0;
}
