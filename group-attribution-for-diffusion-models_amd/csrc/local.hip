// Local model behaviours of the unconditional models (reference unconditional_generation/unlearn.py:871-948): the three
// bandwidth- / latency-bound kernels around the wide U-Net launches of gad/local.py.
//
//   gad_image_metrics    N image pairs -> (mse, nrmse, ssim) in fp64.  One workgroup per 16 x 32 tile of window origins of one
//                        image-channel plane: the tile and its (win-1)-pixel halo sit in LDS as the fp32 pixels they are, every
//                        pixel is converted to fp64 BEFORE it is multiplied or subtracted (products and differences of fp32 values
//                        are exact in fp64), the five window sums (x, y, xx, yy, xy) are formed separably - rows, then columns -
//                        and the SSIM map, its mean and the squared-error sums stay in fp64.  Per-tile partials go to the
//                        workspace; a second kernel adds them per image in a fixed order.
//   gad_add_noise_bcast  xt[r] = sqrt(ac[t]) x0[image(r)] + sqrt(1 - ac[t]) eps[r], NCHW in, NHWC out, one pass.
//   gad_mse_segments     out[s] = mean over segment s of (pred - eps)^2, pred NHWC, eps NCHW: fp64 row sums, then one fixed-order
//                        sum per segment and a single fp32 rounding.
//
// No atomics: every sum has one order that depends on the image / row geometry only, never on the batch size or the position in
// the batch.  Contraction into fma is off for the whole file: SSIM of an image with itself is exactly 1 only while
// ux*ux + uy*uy and 2*ux*uy round alike.
#include <math.h>

#include "gad_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int NT = 256;
constexpr int TH = 16, TW = 32;        // window origins per workgroup: TH rows x TW columns
constexpr int MAX_WIN = 11;            // LDS is sized for windows up to 11 x 11 (scikit-image's Gaussian default; uniform: 7)
constexpr int IH = TH + MAX_WIN - 1, IW = TW + MAX_WIN - 1;

// sum over the 256 threads of a workgroup, in a fixed order; the total is valid in thread 0
__device__ __forceinline__ double block_sum(double v, double* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();                                     // red may still be read from the previous call
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

// grid (tiles_x * tiles_y, C, N).  part[((n * C + c) * ntiles + tile) * 3 + {0, 1, 2}] = sum (a-b)^2 and sum a^2 over the
// tile's own TH x TW pixels, sum of the SSIM map over the tile's window origins.
__global__ __launch_bounds__(NT) void image_metrics_part(const float* __restrict__ a, const float* __restrict__ b,
                                                         double* __restrict__ part, int H, int W, int C, int win, double C1,
                                                         double C2, int tiles_x) {
  __shared__ float sa[IH][IW], sb[IH][IW];
  __shared__ double hs[5][IH][TW];
  __shared__ double red[NT / 64];
  const int tile = blockIdx.x, c = blockIdx.y, n = blockIdx.z;
  const int y0 = (tile / tiles_x) * TH, x0 = (tile % tiles_x) * TW;
  const int ih = min(TH + win - 1, H - y0), iw = min(TW + win - 1, W - x0);     // rows / columns of the image this tile reads
  const int64_t base = (int64_t)n * H * W * C + c;
  for (int i = threadIdx.x; i < ih * iw; i += NT) {
    const int y = i / iw, x = i - y * iw;
    const int64_t at = base + ((int64_t)(y0 + y) * W + (x0 + x)) * C;
    sa[y][x] = a[at];
    sb[y][x] = b[at];
  }
  __syncthreads();

  // squared error and reference energy over the tile's own pixels
  double se = 0.0, aa = 0.0;
  const int oh = min(TH, H - y0), ow = min(TW, W - x0);
  for (int i = threadIdx.x; i < oh * ow; i += NT) {
    const int y = i / ow, x = i - y * ow;
    const double pa = (double)sa[y][x], pb = (double)sb[y][x];
    const double d = pa - pb;
    se += d * d;
    aa += pa * pa;
  }

  // window origins of this tile: rows y0 .. y0 + nh, columns x0 .. x0 + nw (a window must lie inside the image)
  const int nh = max(0, min(TH, H - win + 1 - y0)), nw = max(0, min(TW, W - win + 1 - x0));
  const int rows = nh > 0 ? nh + win - 1 : 0;
  for (int i = threadIdx.x; i < rows * nw; i += NT) {   // horizontal pass: win pixels to the right of (y, x)
    const int y = i / nw, x = i - y * nw;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0, s4 = 0.0;
    for (int k = 0; k < win; ++k) {
      const double pa = (double)sa[y][x + k], pb = (double)sb[y][x + k];
      s0 += pa;
      s1 += pb;
      s2 += pa * pa;
      s3 += pb * pb;
      s4 += pa * pb;
    }
    hs[0][y][x] = s0;
    hs[1][y][x] = s1;
    hs[2][y][x] = s2;
    hs[3][y][x] = s3;
    hs[4][y][x] = s4;
  }
  __syncthreads();
  double ss = 0.0;
  const double np = (double)(win * win), cov_norm = np / (np - 1.0);
  for (int i = threadIdx.x; i < nh * nw; i += NT) {     // vertical pass and the SSIM value of the window at (y, x)
    const int y = i / nw, x = i - y * nw;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0, s4 = 0.0;
    for (int k = 0; k < win; ++k) {
      s0 += hs[0][y + k][x];
      s1 += hs[1][y + k][x];
      s2 += hs[2][y + k][x];
      s3 += hs[3][y + k][x];
      s4 += hs[4][y + k][x];
    }
    const double ux = s0 / np, uy = s1 / np;
    const double vx = cov_norm * (s2 / np - ux * ux), vy = cov_norm * (s3 / np - uy * uy), vxy = cov_norm * (s4 / np - ux * uy);
    ss += ((2.0 * ux * uy + C1) * (2.0 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2));
  }
  se = block_sum(se, red);
  aa = block_sum(aa, red);
  ss = block_sum(ss, red);
  if (threadIdx.x == 0) {
    double* p = part + (((int64_t)n * C + c) * gridDim.x + tile) * 3;
    p[0] = se;
    p[1] = aa;
    p[2] = ss;
  }
}

// one wave per image: lane l adds partials l, l + 64, ... in order, then the fixed butterfly
__global__ __launch_bounds__(64) void image_metrics_final(const double* __restrict__ part, double* __restrict__ out, int nparts,
                                                          double n_elem, double n_win) {
  const double* p = part + (int64_t)blockIdx.x * nparts * 3;
  double se = 0.0, aa = 0.0, ss = 0.0;
  for (int i = threadIdx.x; i < nparts; i += 64) {
    se += p[i * 3];
    aa += p[i * 3 + 1];
    ss += p[i * 3 + 2];
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    se += __shfl_xor(se, o, 64);
    aa += __shfl_xor(aa, o, 64);
    ss += __shfl_xor(ss, o, 64);
  }
  if (threadIdx.x == 0) {
    const double mse = se / n_elem;
    double* o3 = out + (int64_t)blockIdx.x * 3;
    o3[0] = mse;
    o3[1] = sqrt(mse) / sqrt(aa / n_elem);
    o3[2] = ss / n_win;
  }
}

// grid: R * ceil(HW / NT) workgroups; a thread owns one pixel of one row and walks its channels
__global__ __launch_bounds__(NT) void add_noise_bcast_kernel(const float* __restrict__ x0, const float* __restrict__ eps,
                                                             const int64_t* __restrict__ t, const float* __restrict__ ac,
                                                             float* __restrict__ xt, int rows_per_image, int T, int C, int HW,
                                                             int n_train, int chunks) {
  const int r = blockIdx.x / chunks, p = (blockIdx.x - r * chunks) * NT + threadIdx.x;
  if (p >= HW) return;
  const int64_t ts = t[r % T];
  float sa, sb;
  if (ts >= 0 && ts < n_train) {
    const float al = ac[ts];
    sa = sqrtf(al);
    sb = sqrtf(1.f - al);
  } else {                                              // a timestep outside the table: no read, and a result nobody can use
    sa = sb = NAN;
  }
  const float* xi = x0 + (int64_t)(r / rows_per_image) * C * HW + p;
  const float* er = eps + (int64_t)r * C * HW + p;
  float* o = xt + ((int64_t)r * HW + p) * C;
  for (int c = 0; c < C; ++c) o[c] = sa * xi[(int64_t)c * HW] + sb * er[(int64_t)c * HW];
}

// one workgroup per row: rowsum[r] = sum over (pixel, channel) of (pred - eps)^2 in fp64
__global__ __launch_bounds__(NT) void mse_rows_kernel(const float* __restrict__ pred, const float* __restrict__ eps,
                                                      double* __restrict__ rowsum, int C, int HW) {
  __shared__ double red[NT / 64];
  const int64_t r = blockIdx.x;
  const float* pr = pred + r * HW * C;
  const float* er = eps + r * C * HW;
  double s = 0.0;
  for (int p = threadIdx.x; p < HW; p += NT)
    for (int c = 0; c < C; ++c) {
      const double d = (double)pr[(int64_t)p * C + c] - (double)er[(int64_t)c * HW + p];
      s += d * d;
    }
  s = block_sum(s, red);
  if (threadIdx.x == 0) rowsum[r] = s;
}

// one wave per segment: rows l, l + 64, ... per lane, the butterfly, one rounding to fp32
__global__ __launch_bounds__(64) void mse_segments_final(const double* __restrict__ rowsum, float* __restrict__ out, int rows_per,
                                                         double n_elem) {
  const double* p = rowsum + (int64_t)blockIdx.x * rows_per;
  double s = 0.0;
  for (int i = threadIdx.x; i < rows_per; i += 64) s += p[i];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if (threadIdx.x == 0) out[blockIdx.x] = (float)(s / n_elem);
}

struct Tiles {
  int tx, ty;
  int64_t n() const { return (int64_t)tx * ty; }
};
Tiles metric_tiles(int H, int W) { return Tiles{(int)gad_ceil_div(W, TW), (int)gad_ceil_div(H, TH)}; }

int metrics_validate(int32_t N, int32_t H, int32_t W, int32_t C, int32_t win) {
  GAD_CHECK(N >= 1 && N < 65536 && C >= 1 && C < 65536, "gad_image_metrics: N=%d and C=%d must be in 1..65535", N, C);
  GAD_CHECK(win >= 3 && win <= MAX_WIN && (win & 1), "gad_image_metrics: win=%d must be odd and in 3..%d", win, MAX_WIN);
  GAD_CHECK(H >= win && W >= win, "gad_image_metrics: image %d x %d is smaller than the %d x %d window (H < win or W < win)", H, W,
            win, win);
  GAD_CHECK((int64_t)H * W * C < (int64_t)1 << 31, "gad_image_metrics: image of %d x %d x %d elements is too large", H, W, C);
  return 0;
}

int segments_validate(const char* who, int32_t R, int32_t rows_per, int32_t C, int32_t HW) {
  GAD_CHECK(R >= 1 && rows_per >= 1 && C >= 1 && HW >= 1, "%s: R=%d, rows per group=%d, C=%d, HW=%d must all be >= 1", who, R, rows_per,
            C, HW);
  GAD_CHECK((int64_t)C * HW < (int64_t)1 << 31, "%s: row of %d x %d elements is too large", who, C, HW);
  return 0;
}

}  // namespace

#define ST ((hipStream_t)stream)

extern "C" int64_t gad_image_metrics_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t C, int32_t win) {
  if (metrics_validate(N, H, W, C, win) != 0) return -1;
  return (int64_t)N * C * metric_tiles(H, W).n() * 3 * (int64_t)sizeof(double);
}

extern "C" int gad_image_metrics(const float* a, const float* b, double* out, int32_t N, int32_t H, int32_t W, int32_t C,
                                 int32_t win, double data_range, double K1, double K2, void* ws, int64_t ws_bytes, void* stream) {
  GAD_CHECK(a && b && out && ws, "gad_image_metrics: null pointer (a, b, out or workspace)");
  if (metrics_validate(N, H, W, C, win) != 0) return 1;
  GAD_CHECK(data_range > 0.0 && K1 > 0.0 && K2 > 0.0, "gad_image_metrics: data_range, K1 and K2 must be positive");
  GAD_CHECK((reinterpret_cast<uintptr_t>(out) & 7) == 0 && (reinterpret_cast<uintptr_t>(ws) & 7) == 0,
            "gad_image_metrics: out and workspace must be 8-B aligned (misaligned pointer)");
  const Tiles tl = metric_tiles(H, W);
  const int64_t need = (int64_t)N * C * tl.n() * 3 * (int64_t)sizeof(double);
  GAD_CHECK(ws_bytes >= need, "gad_image_metrics: workspace_bytes=%lld < %lld", (long long)ws_bytes, (long long)need);
  const double c1 = (K1 * data_range) * (K1 * data_range), c2 = (K2 * data_range) * (K2 * data_range);
  hipLaunchKernelGGL(image_metrics_part, dim3((unsigned)tl.n(), C, N), dim3(NT), 0, ST, a, b, (double*)ws, H, W, C, win, c1, c2,
                     tl.tx);
  GAD_LAUNCH_CHECK("gad_image_metrics(part)");
  hipLaunchKernelGGL(image_metrics_final, dim3(N), dim3(64), 0, ST, (const double*)ws, out, (int)(C * tl.n()),
                     (double)H * W * C, (double)(H - win + 1) * (W - win + 1) * C);
  GAD_LAUNCH_CHECK("gad_image_metrics(final)");
  return 0;
}

extern "C" int gad_add_noise_bcast(const float* x0, const float* eps, const int64_t* t, const float* alphas_cumprod, float* xt,
                                   int32_t R, int32_t rows_per_image, int32_t T, int32_t C, int32_t HW,
                                   int32_t num_train_timesteps, void* stream) {
  GAD_CHECK(x0 && eps && t && alphas_cumprod && xt, "gad_add_noise_bcast: null pointer (x0, eps, t, alphas_cumprod or xt)");
  if (segments_validate("gad_add_noise_bcast", R, rows_per_image, C, HW) != 0) return 1;
  GAD_CHECK(T >= 1 && num_train_timesteps >= 1, "gad_add_noise_bcast: T=%d and num_train_timesteps=%d must be >= 1", T,
            num_train_timesteps);
  GAD_CHECK(R % T == 0, "gad_add_noise_bcast: R=%d is not a multiple of T=%d (R %% T != 0)", R, T);
  GAD_CHECK(rows_per_image % T == 0 && R % rows_per_image == 0,
            "gad_add_noise_bcast: rows_per_image=%d must be a multiple of T=%d and divide R=%d", rows_per_image, T, R);
  const int64_t chunks = gad_ceil_div(HW, NT);
  GAD_CHECK(R * chunks < (int64_t)1 << 31, "gad_add_noise_bcast: launch of %d rows x %d pixels is too large", R, HW);
  hipLaunchKernelGGL(add_noise_bcast_kernel, dim3((unsigned)(R * chunks)), dim3(NT), 0, ST, x0, eps, t, alphas_cumprod, xt,
                     rows_per_image, T, C, HW, num_train_timesteps, (int)chunks);
  GAD_LAUNCH_CHECK("gad_add_noise_bcast");
  return 0;
}

extern "C" int64_t gad_mse_segments_workspace_bytes(int32_t R, int32_t rows_per_segment, int32_t C, int32_t HW) {
  if (segments_validate("gad_mse_segments", R, rows_per_segment, C, HW) != 0) return -1;
  return (int64_t)R * (int64_t)sizeof(double);
}

extern "C" int gad_mse_segments(const float* pred, const float* eps, float* out, int32_t R, int32_t rows_per_segment, int32_t C,
                                int32_t HW, void* ws, int64_t ws_bytes, void* stream) {
  GAD_CHECK(pred && eps && out && ws, "gad_mse_segments: null pointer (pred, eps, out or workspace)");
  if (segments_validate("gad_mse_segments", R, rows_per_segment, C, HW) != 0) return 1;
  GAD_CHECK(R % rows_per_segment == 0, "gad_mse_segments: R=%d is not a multiple of rows_per_segment=%d (R %% rows_per_segment != 0)",
            R, rows_per_segment);
  GAD_CHECK((reinterpret_cast<uintptr_t>(ws) & 7) == 0, "gad_mse_segments: workspace must be 8-B aligned (misaligned pointer)");
  const int64_t need = (int64_t)R * (int64_t)sizeof(double);
  GAD_CHECK(ws_bytes >= need, "gad_mse_segments: workspace_bytes=%lld < %lld", (long long)ws_bytes, (long long)need);
  hipLaunchKernelGGL(mse_rows_kernel, dim3(R), dim3(NT), 0, ST, pred, eps, (double*)ws, C, HW);
  GAD_LAUNCH_CHECK("gad_mse_segments(rows)");
  hipLaunchKernelGGL(mse_segments_final, dim3(R / rows_per_segment), dim3(64), 0, ST, (const double*)ws, out, rows_per_segment,
                     (double)rows_per_segment * C * HW);
  GAD_LAUNCH_CHECK("gad_mse_segments(final)");
  return 0;
}
