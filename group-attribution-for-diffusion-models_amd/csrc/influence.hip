// WoodFisher recursion of influence unlearning over the flat parameter-sized vectors (gfx950).
// One iteration for a batch gradient g (reference src/unlearn/Wfisher.py:200-205, Singh & Alistarh eq. 2):
//   tmp = o.g   kg = k.g        k -= kg / (N + tmp) * o (old o)        o -= tmp / (N + tmp) * o
// gad_wf_dots reads o, k, g once (12 B/param) and leaves the two dot products on the device as fp64; gad_wf_update reads
// o, k and writes both (16 B/param) with coefficients every thread forms from those two doubles: 28 B/param per iteration,
// two + one launches, no host sync, hipGraph-capturable.
// The products and their sums are fp64: an fp32 x fp32 product is exact in fp64, so the only rounding is the fp64
// summation, and k.g is a sum of 3.6e7 (SD: 8.6e8) terms of both signs.  Order: each lane's four float4 components in
// their own chains, (c0 + c1) + (c2 + c3); the wave by xor butterflies; the four waves through LDS in wave order; one
// pair per workgroup in the workspace; a single-workgroup pass that sums the pairs in index order.  No atomics: the
// result is a function of (o, k, g, n) alone.
#include "gad_dev.h"

namespace {

constexpr int NT = 256;
constexpr int MAX_BLOCKS = GAD_STREAM_MAX_BLOCKS;     // the final pass stages a pair per workgroup in LDS

// the one sizing rule: the workspace query and the launch both read it (the streaming grid, a float4 per lane)
inline int wf_blocks(int64_t n) {
  const int64_t nv = n / 4;
  return (int)gad_stream_grid(nv > 0 ? nv : 1);
}

__global__ __launch_bounds__(NT) void wf_dots_part_kernel(const float* __restrict__ o, const float* __restrict__ k,
                                                          const float* __restrict__ g, long n, double* __restrict__ part) {
  __shared__ double red[2][NT / 64];
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;      // o.g, one chain per float4 component
  double b0 = 0.0, b1 = 0.0, b2 = 0.0, b3 = 0.0;      // k.g
  const long nv = n >> 2, gs = (long)gridDim.x * blockDim.x;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += gs) {
    const f32x4 vo = reinterpret_cast<const f32x4*>(o)[i];
    const f32x4 vk = reinterpret_cast<const f32x4*>(k)[i];
    const f32x4 vg = reinterpret_cast<const f32x4*>(g)[i];
    const double g0 = (double)vg[0], g1 = (double)vg[1], g2 = (double)vg[2], g3 = (double)vg[3];
    a0 = fma((double)vo[0], g0, a0); a1 = fma((double)vo[1], g1, a1);
    a2 = fma((double)vo[2], g2, a2); a3 = fma((double)vo[3], g3, a3);
    b0 = fma((double)vk[0], g0, b0); b1 = fma((double)vk[1], g1, b1);
    b2 = fma((double)vk[2], g2, b2); b3 = fma((double)vk[3], g3, b3);
  }
  for (long i = (n & ~3L) + (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gs) {   // n % 4 tail
    const double gi = (double)g[i];
    a0 = fma((double)o[i], gi, a0);
    b0 = fma((double)k[i], gi, b0);
  }
  const double a = wave_sum_f64((a0 + a1) + (a2 + a3));
  const double b = wave_sum_f64((b0 + b1) + (b2 + b3));
  if ((threadIdx.x & 63) == 0) {
    red[0][threadIdx.x >> 6] = a;
    red[1][threadIdx.x >> 6] = b;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    part[2 * (long)blockIdx.x + 0] = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
    part[2 * (long)blockIdx.x + 1] = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
  }
}

// one workgroup: the pairs are staged in LDS by all threads, then one lane per dot product (in two different waves)
// adds its column in index order
__global__ __launch_bounds__(NT) void wf_dots_final_kernel(const double* __restrict__ part, int nparts, double* __restrict__ dots) {
  __shared__ double sh[2 * MAX_BLOCKS];
  for (int i = threadIdx.x; i < 2 * nparts; i += NT) sh[i] = part[i];
  __syncthreads();
  if ((threadIdx.x & 63) == 0 && threadIdx.x < 128) {
    const int which = threadIdx.x >> 6;
    double s = 0.0;
    for (int i = 0; i < nparts; ++i) s += sh[2 * i + which];
    dots[which] = s;
  }
}

__device__ __forceinline__ void wf_one(float& o, float& k, float ck, float co) {
  const float old = o;
  k = __builtin_fmaf(-ck, old, k);
  o = __builtin_fmaf(-co, old, old);
}

__global__ __launch_bounds__(NT) void wf_update_kernel(float* __restrict__ o, float* __restrict__ k,
                                                       const double* __restrict__ dots, double N, long n) {
  const double tmp = dots[0], kg = dots[1], den = N + tmp;
  const float ck = (float)(kg / den), co = (float)(tmp / den);       // plain IEEE if den == 0, as in the reference
  const long nv = n >> 2, gs = (long)gridDim.x * blockDim.x;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += gs) {
    f32x4 vo = reinterpret_cast<f32x4*>(o)[i], vk = reinterpret_cast<f32x4*>(k)[i];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float oe = vo[e], ke = vk[e];
      wf_one(oe, ke, ck, co);
      vo[e] = oe; vk[e] = ke;
    }
    reinterpret_cast<f32x4*>(k)[i] = vk;
    reinterpret_cast<f32x4*>(o)[i] = vo;
  }
  for (long i = (n & ~3L) + (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gs) wf_one(o[i], k[i], ck, co);
}

inline bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; }

}  // namespace

extern "C" int64_t gad_wf_dots_workspace_bytes(int64_t n) {
  if (n <= 0) {
    gad_set_error("gad_wf_dots_workspace_bytes: n must be positive (n=%lld)", (long long)n);
    return -1;
  }
  return (int64_t)wf_blocks(n) * 2 * (int64_t)sizeof(double);
}

extern "C" int gad_wf_dots(const float* o, const float* k, const float* g, int64_t n, double* dots, void* ws, int64_t ws_bytes,
                           void* stream) {
  GAD_CHECK(o && k && g && dots && ws, "gad_wf_dots: null pointer");
  GAD_CHECK(n > 0, "gad_wf_dots: n must be positive (n=%lld)", (long long)n);
  GAD_CHECK(gad_aligned16(o) && gad_aligned16(k) && gad_aligned16(g), "gad_wf_dots: o, k and g must be 16-byte aligned");
  GAD_CHECK(aligned8(dots) && aligned8(ws), "gad_wf_dots: dots and the workspace must be 8-byte aligned");
  const int blocks = wf_blocks(n);
  const int64_t need = (int64_t)blocks * 2 * (int64_t)sizeof(double);
  GAD_CHECK(ws_bytes >= need, "gad_wf_dots: ws_bytes=%lld < gad_wf_dots_workspace_bytes()=%lld", (long long)ws_bytes, (long long)need);
  hipLaunchKernelGGL(wf_dots_part_kernel, dim3((unsigned)blocks), dim3(NT), 0, (hipStream_t)stream, o, k, g, (long)n, (double*)ws);
  GAD_LAUNCH_CHECK("gad_wf_dots(part)");
  hipLaunchKernelGGL(wf_dots_final_kernel, dim3(1), dim3(NT), 0, (hipStream_t)stream, (const double*)ws, blocks, dots);
  GAD_LAUNCH_CHECK("gad_wf_dots(final)");
  return 0;
}

extern "C" int gad_wf_update(float* o, float* k, const double* dots, double N, int64_t n, void* stream) {
  GAD_CHECK(o && k && dots, "gad_wf_update: null pointer");
  GAD_CHECK(n > 0, "gad_wf_update: n must be positive (n=%lld)", (long long)n);
  GAD_CHECK(gad_aligned16(o) && gad_aligned16(k), "gad_wf_update: o and k must be 16-byte aligned");
  GAD_CHECK(aligned8(dots), "gad_wf_update: dots must be 8-byte aligned");
  GAD_CHECK(o != k, "gad_wf_update: o and k must be different vectors");
  hipLaunchKernelGGL(wf_update_kernel, dim3((unsigned)wf_blocks(n)), dim3(NT), 0, (hipStream_t)stream, o, k, dots, N, (long)n);
  GAD_LAUNCH_CHECK("gad_wf_update");
  return 0;
}
