// Score tail (gad/inception.py: InceptionV3 pool3 / logits for FID and IS; reference src/attributions/global_scores/
// fid_score.py, inception_score.py through pytorch-fid's InceptionV3): the three bandwidth-bound kernels between the
// convolutions, which run through gad_gemm.
//
//   gad_pool2d           k x k max / average pooling of an NHWC map, reading and writing channel slices of wider buffers
//                        (pixel strides ldx / ldy), so a pool branch lands in its slice of a concatenated block output.
//   gad_resize_bilinear  F.interpolate(mode="bilinear", align_corners=False) from NCHW to NHWC with y = a v + b folded in.
//   gad_relu             in place on a [rows][C] slice of a [rows][ld] buffer.
//
// One thread per output element (float4 of channels on the vector path, else one float): consecutive lanes walk consecutive
// channels, then pixels, so every wave's loads and stores are contiguous runs.  Grid-stride over at most GAD_STREAM_MAX_BLOCKS
// workgroups; every element offset is 64-bit.  Contraction into fma is off: the resize weights its four taps in one stated
// order.
#include <math.h>

#include "gad_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int NT = 256;

template <int V> struct Vec;
template <> struct Vec<1> { typedef float T; };
template <> struct Vec<4> { typedef f32x4 T; };

template <int V> __device__ __forceinline__ typename Vec<V>::T splat(float v);
template <> __device__ __forceinline__ float splat<1>(float v) { return v; }
template <> __device__ __forceinline__ f32x4 splat<4>(float v) { return f32x4{v, v, v, v}; }

__device__ __forceinline__ float vmax(float a, float b) { return fmaxf(a, b); }
__device__ __forceinline__ f32x4 vmax(f32x4 a, f32x4 b) {
  return f32x4{fmaxf(a.x, b.x), fmaxf(a.y, b.y), fmaxf(a.z, b.z), fmaxf(a.w, b.w)};
}

struct PoolGeom {
  int H, W, Ho, Wo, k, stride, pad, mode, relu;
  int cv;                  // channels / V
  int64_t ldx, ldy;        // pixel strides in floats
  int64_t total;           // B * Ho * Wo * cv
};

template <int V>
__global__ __launch_bounds__(NT) void pool2d_kernel(const float* __restrict__ x, float* __restrict__ y, PoolGeom g) {
  typedef typename Vec<V>::T T;
  for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < g.total; i += (int64_t)gridDim.x * NT) {
    const int c = (int)(i % g.cv);
    int64_t p = i / g.cv;
    const int ow = (int)(p % g.Wo);
    p /= g.Wo;
    const int oh = (int)(p % g.Ho);
    const int64_t b = p / g.Ho;
    const int h0 = oh * g.stride - g.pad, w0 = ow * g.stride - g.pad;
    const int hs = max(h0, 0), he = min(h0 + g.k, g.H), ws = max(w0, 0), we = min(w0 + g.k, g.W);
    const float* xb = x + b * g.H * g.W * g.ldx + (int64_t)c * V;
    T acc;
    if (g.mode == GAD_POOL_MAX) {
      acc = splat<V>(-INFINITY);
      for (int h = hs; h < he; ++h)
        for (int w = ws; w < we; ++w) acc = vmax(acc, *reinterpret_cast<const T*>(xb + ((int64_t)h * g.W + w) * g.ldx));
      if (g.relu) acc = vmax(acc, splat<V>(0.f));       // max commutes with ReLU
    } else {
      // the taps are summed and divided in fp64 and rounded once: the average is the correctly rounded one whatever the taps'
      // signs (up to nine adds in fp32 lose ulps of the LARGEST tap, which a cancelling window magnifies); the kernel stays
      // bound by its loads
      double sum[V] = {};
      for (int h = hs; h < he; ++h)
        for (int w = ws; w < we; ++w) {
          T v = *reinterpret_cast<const T*>(xb + ((int64_t)h * g.W + w) * g.ldx);
          if (g.relu) v = vmax(v, splat<V>(0.f));
          const float* vf = reinterpret_cast<const float*>(&v);
#pragma unroll
          for (int j = 0; j < V; ++j) sum[j] += (double)vf[j];
        }
      const double n = (double)(g.mode == GAD_POOL_AVG ? g.k * g.k : (he - hs) * (we - ws));
      float* af = reinterpret_cast<float*>(&acc);
#pragma unroll
      for (int j = 0; j < V; ++j) af[j] = (float)(sum[j] / n);
    }
    *reinterpret_cast<T*>(y + ((b * g.Ho + oh) * g.Wo + ow) * g.ldy + (int64_t)c * V) = acc;
  }
}

struct ResizeGeom {
  int C, H, W, Ho, Wo;
  int cv;
  float a, b;
  double sh, sw;           // H / Ho, W / Wo
  int64_t total;           // B * Ho * Wo * cv
};

// source coordinate of output index o: (o + 0.5) * scale - 0.5, clamped below at 0; formed in fp64 so that the weight is the
// exact one rounded once (in fp32 the coordinate of a 32 -> 299 resize carries 2e-6 of its own)
__device__ __forceinline__ void src_of(int o, double scale, int n, int& i0, int& i1, float& l1) {
  double s = ((double)o + 0.5) * scale - 0.5;
  s = s < 0.0 ? 0.0 : s;
  i0 = min((int)s, n - 1);
  i1 = min(i0 + 1, n - 1);
  l1 = (float)(s - (double)i0);
}

template <int V>
__global__ __launch_bounds__(NT) void resize_bilinear_kernel(const float* __restrict__ x, float* __restrict__ y, ResizeGeom g) {
  const int64_t plane = (int64_t)g.H * g.W;
  for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < g.total; i += (int64_t)gridDim.x * NT) {
    const int c = (int)(i % g.cv) * V;
    int64_t p = i / g.cv;
    const int ow = (int)(p % g.Wo);
    p /= g.Wo;
    const int oh = (int)(p % g.Ho);
    const int64_t b = p / g.Ho;
    int h0, h1, w0, w1;
    float lh, lw;
    src_of(oh, g.sh, g.H, h0, h1, lh);
    src_of(ow, g.sw, g.W, w0, w1, lw);
    const float kh = 1.f - lh, kw = 1.f - lw;
    const float* xb = x + (b * g.C + c) * plane;
    float out[V];
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const float* xp = xb + j * plane;
      const float top = kw * xp[(int64_t)h0 * g.W + w0] + lw * xp[(int64_t)h0 * g.W + w1];
      const float bot = kw * xp[(int64_t)h1 * g.W + w0] + lw * xp[(int64_t)h1 * g.W + w1];
      out[j] = g.a * (kh * top + lh * bot) + g.b;
    }
    float* yo = y + ((b * g.Ho + oh) * g.Wo + ow) * g.C + c;
    if constexpr (V == 4) {
      *reinterpret_cast<f32x4*>(yo) = f32x4{out[0], out[1 % V], out[2 % V], out[3 % V]};
    } else {
      yo[0] = out[0];
    }
  }
}

template <int V>
__global__ __launch_bounds__(NT) void relu_kernel(float* __restrict__ x, int64_t total, int cv, int64_t ld) {
  typedef typename Vec<V>::T T;
  for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < total; i += (int64_t)gridDim.x * NT) {
    const int64_t r = i / cv;
    const int c = (int)(i - r * cv);
    T* p = reinterpret_cast<T*>(x + r * ld + (int64_t)c * V);
    *p = vmax(*p, splat<V>(0.f));
  }
}

const double TOO_LARGE = 4e18;            // element counts stay inside int64

}  // namespace

#define ST ((hipStream_t)stream)

extern "C" int gad_pool2d(const float* x, float* y, int32_t B, int32_t H, int32_t W, int32_t C, int32_t ldx, int32_t ldy,
                          int32_t Ho, int32_t Wo, int32_t k, int32_t stride, int32_t pad, int32_t mode, int32_t relu_in,
                          void* stream) {
  GAD_CHECK(x && y, "gad_pool2d: null pointer (x or y)");
  GAD_CHECK(B >= 1 && H >= 1 && W >= 1 && C >= 1, "gad_pool2d: B=%d, H=%d, W=%d, C=%d must all be >= 1", B, H, W, C);
  GAD_CHECK(k == 2 || k == 3, "gad_pool2d: window k=%d must be 2 or 3", k);
  GAD_CHECK(stride == 1 || stride == 2, "gad_pool2d: stride=%d must be 1 or 2", stride);
  GAD_CHECK(pad == 0 || pad == 1, "gad_pool2d: pad=%d must be 0 or 1", pad);
  GAD_CHECK(mode >= GAD_POOL_MAX && mode <= GAD_POOL_AVG_VALID, "gad_pool2d: mode=%d must be 0 (max), 1 (avg) or 2 (avg, padding excluded)", mode);
  GAD_CHECK(ldx >= C, "gad_pool2d: ldx=%d < C=%d", ldx, C);
  GAD_CHECK(ldy >= C, "gad_pool2d: ldy=%d < C=%d", ldy, C);
  GAD_CHECK(H + 2 * pad >= k && W + 2 * pad >= k, "gad_pool2d: map %d x %d (pad %d) is smaller than the %d x %d window", H, W, pad, k, k);
  const int ho = (H + 2 * pad - k) / stride + 1, wo = (W + 2 * pad - k) / stride + 1;
  GAD_CHECK(Ho == ho && Wo == wo, "gad_pool2d: Ho=%d, Wo=%d but a %d x %d map with k=%d, stride=%d, pad=%d pools to %d x %d", Ho, Wo, H,
            W, k, stride, pad, ho, wo);
  GAD_CHECK((double)B * H * W * ldx < TOO_LARGE && (double)B * Ho * Wo * ldy < TOO_LARGE, "gad_pool2d: tensor too large");
  const bool v4 = C % 4 == 0 && ldx % 4 == 0 && ldy % 4 == 0 && gad_aligned16(x) && gad_aligned16(y);
  PoolGeom g;
  g.H = H, g.W = W, g.Ho = Ho, g.Wo = Wo, g.k = k, g.stride = stride, g.pad = pad, g.mode = mode, g.relu = relu_in != 0;
  g.cv = v4 ? C / 4 : C;
  g.ldx = ldx, g.ldy = ldy;
  g.total = (int64_t)B * Ho * Wo * g.cv;
  if (v4) hipLaunchKernelGGL(pool2d_kernel<4>, dim3(gad_stream_grid(g.total)), dim3(NT), 0, ST, x, y, g);
  else hipLaunchKernelGGL(pool2d_kernel<1>, dim3(gad_stream_grid(g.total)), dim3(NT), 0, ST, x, y, g);
  GAD_LAUNCH_CHECK("gad_pool2d");
  return 0;
}

extern "C" int gad_resize_bilinear(const float* x, float* y, int32_t B, int32_t C, int32_t H, int32_t W, int32_t Ho, int32_t Wo,
                                   float a, float b, void* stream) {
  GAD_CHECK(x && y, "gad_resize_bilinear: null pointer (x or y)");
  GAD_CHECK(B >= 1 && C >= 1 && H >= 1 && W >= 1 && Ho >= 1 && Wo >= 1,
            "gad_resize_bilinear: B=%d, C=%d, H=%d, W=%d, Ho=%d, Wo=%d must all be >= 1", B, C, H, W, Ho, Wo);
  GAD_CHECK((double)B * C * H * W < TOO_LARGE && (double)B * C * Ho * Wo < TOO_LARGE, "gad_resize_bilinear: tensor too large");
  const bool v4 = C % 4 == 0 && gad_aligned16(y);
  ResizeGeom g;
  g.C = C, g.H = H, g.W = W, g.Ho = Ho, g.Wo = Wo, g.a = a, g.b = b;
  g.cv = v4 ? C / 4 : C;
  g.sh = (double)H / (double)Ho, g.sw = (double)W / (double)Wo;
  g.total = (int64_t)B * Ho * Wo * g.cv;
  if (v4) hipLaunchKernelGGL(resize_bilinear_kernel<4>, dim3(gad_stream_grid(g.total)), dim3(NT), 0, ST, x, y, g);
  else hipLaunchKernelGGL(resize_bilinear_kernel<1>, dim3(gad_stream_grid(g.total)), dim3(NT), 0, ST, x, y, g);
  GAD_LAUNCH_CHECK("gad_resize_bilinear");
  return 0;
}

extern "C" int gad_relu(float* x, int64_t rows, int32_t C, int32_t ld, void* stream) {
  GAD_CHECK(x, "gad_relu: null pointer (x)");
  GAD_CHECK(rows >= 1 && C >= 1, "gad_relu: rows=%lld and C=%d must be >= 1", (long long)rows, C);
  GAD_CHECK(ld >= C, "gad_relu: ld=%d < C=%d", ld, C);
  GAD_CHECK((double)rows * ld < TOO_LARGE, "gad_relu: tensor too large");
  const bool v4 = C % 4 == 0 && ld % 4 == 0 && gad_aligned16(x);
  const int cv = v4 ? C / 4 : C;
  const int64_t total = rows * cv;
  if (v4) hipLaunchKernelGGL(relu_kernel<4>, dim3(gad_stream_grid(total)), dim3(NT), 0, ST, x, total, cv, (int64_t)ld);
  else hipLaunchKernelGGL(relu_kernel<1>, dim3(gad_stream_grid(total)), dim3(NT), 0, ST, x, total, cv, (int64_t)ld);
  GAD_LAUNCH_CHECK("gad_relu");
  return 0;
}
