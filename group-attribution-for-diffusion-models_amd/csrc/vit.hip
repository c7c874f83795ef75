// Score tail (gad/vit.py: the CLIP ViT-B/32, open-CLIP ViT-L/14 and BLIP-VQA image towers; reference
// text_to_image/compute_model_behaviors.py:243-262,358-431 and src/attributions/global_scores/diversity_score.py:89-120): the
// four bandwidth-bound kernels between the contractions, LayerNorms and attention of a pre-LN Vision Transformer, which run
// through gad_gemm, gad_layernorm_fwd and gad_attention_fwd.
//
//   gad_resize_bicubic_patches  antialiased bicubic resize + centre crop + patchify from NCHW into the patch-major matrix
//                               the patch embedding contracts: no resized image reaches HBM.
//   gad_vit_tokens              out[b][t] = LN?((t == 0 ? cls : patches[b][t - 1]) + pos[t])     (CLIP's ln_pre)
//   gad_gelu                    exact erf GELU or QuickGELU, in place on a [rows][C] slice of a [rows][ld] buffer
//   gad_l2_normalize_rows       x[r] /= |x[r]|_2 in place
//
// The resize filter is PIL's / torch's antialias=True one (cubic a = -0.5 widened by max(in / out, 1), taps renormalised).
// `bicubic_axis` below is the one statement of it: a pre-kernel runs it in fp64 once per launch for the R output rows and R
// output columns and leaves (first tap, tap count, fp32 weights) in the caller's workspace; gad_bicubic_taps runs the same
// function on the host in fp64 (tests, references).  The main kernel copies the rows of the table its patch needs into LDS.
#include <math.h>

#include "gad_dev.h"

namespace {

constexpr int NT = 256, WPB = NT / 64;
constexpr int MAX_LDS = 64 * 1024;
const double TOO_LARGE = 4e18;            // element counts stay inside int64

// ---- the filter ----
__host__ __device__ inline double cubic_half(double x) {      // Keys' cubic convolution kernel, a = -0.5
  x = x < 0.0 ? -x : x;
  if (x < 1.0) return (1.5 * x - 2.5) * x * x + 1.0;
  if (x < 2.0) return ((-0.5 * x + 2.5) * x - 4.0) * x + 2.0;
  return 0.0;
}

// max taps of any output index of an axis resized in -> out: PIL's ksize = 2 ceil(support) + 1, support = 2 max(in / out, 1)
__host__ __device__ inline int bicubic_kmax(int in, int out) {
  const double scale = (double)in / (double)out, fs = scale > 1.0 ? scale : 1.0;
  return 2 * (int)ceil(2.0 * fs) + 1;
}

// output index o of an axis resized in -> out: first tap, tap count, and (w != nullptr) the count normalised weights
__host__ __device__ inline void bicubic_axis(int in, int out, int o, int& start, int& count, double* w) {
  const double scale = (double)in / (double)out, fs = scale > 1.0 ? scale : 1.0;
  const double c = ((double)o + 0.5) * scale, sup = 2.0 * fs;
  int x0 = (int)(c - sup + 0.5), x1 = (int)(c + sup + 0.5);
  x0 = x0 < 0 ? 0 : x0;
  x1 = x1 > in ? in : x1;
  start = x0, count = x1 - x0;
  if (w == nullptr) return;
  double sum = 0.0;
  for (int i = 0; i < count; ++i) {
    w[i] = cubic_half(((double)(x0 + i) - c + 0.5) / fs);
    sum += w[i];
  }
  for (int i = 0; i < count; ++i) w[i] /= sum;
}

// workspace: per axis (y then x) [R] int32 first tap | [R] int32 count | [R][kmax] float weights (zero past count)
struct ResizeGeom {
  int H, W, rh, rw, oy, ox, R, P, g;
  int kmy, kmx;
  float a, b;
};

__host__ __device__ inline int64_t axis_floats(int R, int kmax) { return (int64_t)R * (2 + kmax); }

constexpr int KMAX_CAP = 64;              // taps per axis a pre-kernel thread holds (in / out up to 15)

__global__ __launch_bounds__(NT) void bicubic_table_kernel(float* __restrict__ ws, ResizeGeom g) {
  const int i = blockIdx.x * NT + threadIdx.x;
  if (i >= 2 * g.R) return;
  const bool isx = i >= g.R;
  const int o = isx ? i - g.R : i;
  const int kmax = isx ? g.kmx : g.kmy;
  float* base = ws + (isx ? axis_floats(g.R, g.kmy) : 0);
  double w[KMAX_CAP];
  int start, count;
  bicubic_axis(isx ? g.W : g.H, isx ? g.rw : g.rh, (isx ? g.ox : g.oy) + o, start, count, w);
  reinterpret_cast<int32_t*>(base)[o] = start;
  reinterpret_cast<int32_t*>(base)[g.R + o] = count;
  float* wo = base + 2 * (int64_t)g.R + (int64_t)o * kmax;
  for (int k = 0; k < kmax; ++k) wo[k] = k < count ? (float)w[k] : 0.f;
}

// One workgroup per patch (b, gy, gx).  LDS: the patch's P rows of both tap tables, then the P x P x 3 output tile, which is
// computed with pw fastest across lanes (neighbouring lanes read neighbouring input columns) and stored as one contiguous
// run of the patch-major matrix.  Every output is sum_i wy[i] * (sum_j wx[j] * in[y0 + i][x0 + j]), accumulated in fp32.
__global__ __launch_bounds__(NT) void resize_bicubic_patches_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                                    const float* __restrict__ ws, ResizeGeom g) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int P = g.P, PP3 = P * P * 3;
  float* tile = lds;                                   // [P][P][3]
  float* wy = tile + ((PP3 + 3) & ~3);                 // [P][kmy]
  float* wx = wy + P * g.kmy;                          // [P][kmx]
  int32_t* sy = reinterpret_cast<int32_t*>(wx + P * g.kmx);      // [P] first tap, [P] count, then the same for x
  int32_t* cy = sy + P;
  int32_t* sx = cy + P;
  int32_t* cx = sx + P;
  const float* tyb = ws;
  const float* txb = ws + axis_floats(g.R, g.kmy);
  const int gx = blockIdx.x % g.g, gy = blockIdx.x / g.g;
  const int64_t b = blockIdx.y;
  for (int i = threadIdx.x; i < P; i += NT) {
    sy[i] = reinterpret_cast<const int32_t*>(tyb)[gy * P + i];
    cy[i] = reinterpret_cast<const int32_t*>(tyb)[g.R + gy * P + i];
    sx[i] = reinterpret_cast<const int32_t*>(txb)[gx * P + i];
    cx[i] = reinterpret_cast<const int32_t*>(txb)[g.R + gx * P + i];
  }
  for (int i = threadIdx.x; i < P * g.kmy; i += NT) wy[i] = tyb[2 * (int64_t)g.R + (int64_t)gy * P * g.kmy + i];
  for (int i = threadIdx.x; i < P * g.kmx; i += NT) wx[i] = txb[2 * (int64_t)g.R + (int64_t)gx * P * g.kmx + i];
  __syncthreads();
  const int64_t plane = (int64_t)g.H * g.W;
  const float* xb = x + b * 3 * plane;
  for (int e = threadIdx.x; e < PP3; e += NT) {
    const int pw = e % P, ph = (e / P) % P, c = e / (P * P);
    const float* xp = xb + c * plane + (int64_t)sy[ph] * g.W + sx[pw];
    const float* wr = wy + ph * g.kmy;
    const float* wc = wx + pw * g.kmx;
    const int ny = cy[ph], nx = cx[pw];
    float acc = 0.f;
    for (int i = 0; i < ny; ++i) {
      const float* row = xp + (int64_t)i * g.W;
      float r = 0.f;
      for (int j = 0; j < nx; ++j) r += wc[j] * row[j];
      acc += wr[i] * r;
    }
    tile[(ph * P + pw) * 3 + c] = g.a * acc + g.b;
  }
  __syncthreads();
  float* yo = y + (b * g.g * g.g + blockIdx.x) * PP3;
  if (PP3 % 4 == 0 && (reinterpret_cast<uintptr_t>(yo) & 15) == 0) {
    for (int e = threadIdx.x; e < PP3 / 4; e += NT) reinterpret_cast<f32x4*>(yo)[e] = reinterpret_cast<const f32x4*>(tile)[e];
  } else {
    for (int e = threadIdx.x; e < PP3; e += NT) yo[e] = tile[e];
  }
}

int resize_lds_bytes(int P, int kmy, int kmx) { return (((P * P * 3 + 3) & ~3) + P * (kmy + kmx) + 4 * P) * 4; }

// ---- tokens ----
template <int V> struct Vec;
template <> struct Vec<1> { typedef float T; };
template <> struct Vec<4> { typedef f32x4 T; };

__device__ __forceinline__ float hsum(float v) { return v; }
__device__ __forceinline__ float hsum(f32x4 v) { return (v.x + v.y) + (v.z + v.w); }

// One wave per token row.  The row is (source + pos), formed again in each of the three sweeps from lines that stay in the
// vector L1 (a row is at most a few KB): mean, then the centred sum of squares (two passes: the rows of a trained tower sit
// far from zero against their spread, where E[x^2] - E[x]^2 cancels), then the store.
template <int V>
__global__ __launch_bounds__(NT) void vit_tokens_kernel(const float* __restrict__ patches, const float* __restrict__ cls,
                                                        const float* __restrict__ pos, const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, float* __restrict__ out, int64_t rows,
                                                        int T, int C, float eps) {
  typedef typename Vec<V>::T VT;
  const int lane = threadIdx.x & 63, CV = C / V;
  for (int64_t row = (int64_t)blockIdx.x * WPB + (threadIdx.x >> 6); row < rows; row += (int64_t)gridDim.x * WPB) {
    const int64_t b = row / T;
    const int t = (int)(row - b * T);
    const VT* src = reinterpret_cast<const VT*>(t == 0 ? cls : patches + (b * (T - 1) + (t - 1)) * C);
    const VT* pr = reinterpret_cast<const VT*>(pos + (int64_t)t * C);
    VT* yr = reinterpret_cast<VT*>(out + row * C);
    if (gamma == nullptr) {
      for (int c = lane; c < CV; c += 64) yr[c] = src[c] + pr[c];
      continue;
    }
    float s = 0.f;
    for (int c = lane; c < CV; c += 64) s += hsum(src[c] + pr[c]);
    const float mu = wave_sum(s) / (float)C;
    float q = 0.f;
    for (int c = lane; c < CV; c += 64) {
      const VT d = src[c] + pr[c] - mu;
      q += hsum(d * d);
    }
    const float rs = 1.0f / sqrtf(wave_sum(q) / (float)C + eps);
    for (int c = lane; c < CV; c += 64)
      yr[c] = (src[c] + pr[c] - mu) * rs * reinterpret_cast<const VT*>(gamma)[c] + reinterpret_cast<const VT*>(beta)[c];
  }
}

// ---- GELU ----
__device__ __forceinline__ float gelu_quick(float v) { return v / (1.0f + expf(-1.702f * v)); }

template <int V, int KIND>
__global__ __launch_bounds__(NT) void gelu_kernel(float* __restrict__ x, int64_t total, int cv, int64_t ld) {
  for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < total; i += (int64_t)gridDim.x * NT) {
    const int64_t r = i / cv;
    const int c = (int)(i - r * cv);
    float* p = x + r * ld + (int64_t)c * V;
    if constexpr (V == 4) {
      f32x4 v = *reinterpret_cast<f32x4*>(p);
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = KIND == 0 ? gelu_f(v[j]) : gelu_quick(v[j]);
      *reinterpret_cast<f32x4*>(p) = v;
    } else {
      *p = KIND == 0 ? gelu_f(*p) : gelu_quick(*p);
    }
  }
}

// ---- L2 normalisation ----
// One wave per row.  The row is scaled by a power of two taken from its largest magnitude before it is squared (exact, and
// the squares of a row of norm 1e-20 or 1e+20 neither vanish nor overflow); an all-zero row divides 0 by 0 as the reference
// does (no eps).
template <int V>
__global__ __launch_bounds__(NT) void l2_normalize_kernel(float* __restrict__ x, int64_t rows, int C, int64_t ld) {
  typedef typename Vec<V>::T VT;
  const int lane = threadIdx.x & 63, CV = C / V;
  for (int64_t row = (int64_t)blockIdx.x * WPB + (threadIdx.x >> 6); row < rows; row += (int64_t)gridDim.x * WPB) {
    VT* xr = reinterpret_cast<VT*>(x + row * ld);
    float m = 0.f;
    for (int c = lane; c < CV; c += 64) {
      const VT v = xr[c];
      const float* vf = reinterpret_cast<const float*>(&v);
#pragma unroll
      for (int j = 0; j < V; ++j) m = fmaxf(m, fabsf(vf[j]));
    }
    m = wave_max(m);
    int e = 0;
    if (m > 0.f && m < INFINITY) frexpf(m, &e);
    // two exact steps: 2^-e alone is not an fp32 number at either end of the exponent range
    const int e1 = e / 2, e2 = e - e1;
    const float k1 = ldexpf(1.0f, -e1), k2 = ldexpf(1.0f, -e2);
    float q = 0.f;
    for (int c = lane; c < CV; c += 64) {
      const VT d = xr[c] * k1 * k2;
      q += hsum(d * d);
    }
    const float n = sqrtf(wave_sum(q));
    for (int c = lane; c < CV; c += 64) {
      VT v = xr[c] * k1 * k2;
      float* vf = reinterpret_cast<float*>(&v);
#pragma unroll
      for (int j = 0; j < V; ++j) vf[j] = vf[j] / n;
      xr[c] = v;
    }
  }
}

// the geometry checks shared by the workspace query and the launch -> nullptr or a message
const char* resize_refusal(int32_t H, int32_t W, int32_t rh, int32_t rw, int32_t oy, int32_t ox, int32_t R, int32_t P) {
  if (H < 1 || W < 1 || rh < 1 || rw < 1 || R < 1 || P < 1) return "H, W, rh, rw, R and P must all be >= 1";
  if (R % P != 0) return "R must be a multiple of the patch side P";
  if (oy < 0 || ox < 0 || oy + R > rh || ox + R > rw) return "the R x R crop at (oy, ox) must lie inside the rh x rw resized image";
  if (bicubic_kmax(H, rh) > KMAX_CAP || bicubic_kmax(W, rw) > KMAX_CAP) return "more than 64 taps per axis (a reduction beyond 15 x)";
  if (resize_lds_bytes(P, bicubic_kmax(H, rh), bicubic_kmax(W, rw)) > MAX_LDS) return "the patch tile and its tap tables exceed 64 KB of LDS";
  return nullptr;
}

}  // namespace

#define ST ((hipStream_t)stream)

extern "C" int32_t gad_bicubic_max_taps(int32_t in, int32_t out) {
  if (in < 1 || out < 1) {
    gad_set_error("gad_bicubic_max_taps: in=%d and out=%d must be >= 1", in, out);
    return -1;
  }
  return bicubic_kmax(in, out);
}

extern "C" int gad_bicubic_taps(int32_t in, int32_t out, int32_t origin, int32_t n, int32_t* start, int32_t* count, double* w) {
  GAD_CHECK(start && count && w, "gad_bicubic_taps: null pointer (start, count or w)");
  GAD_CHECK(in >= 1 && out >= 1 && n >= 1, "gad_bicubic_taps: in=%d, out=%d, n=%d must all be >= 1", in, out, n);
  GAD_CHECK(origin >= 0 && (int64_t)origin + n <= out, "gad_bicubic_taps: indices [%d, %d + %d) leave the %d resized ones", origin,
            origin, n, out);
  const int kmax = bicubic_kmax(in, out);
  for (int o = 0; o < n; ++o) {
    double* wo = w + (int64_t)o * kmax;
    for (int k = 0; k < kmax; ++k) wo[k] = 0.0;
    bicubic_axis(in, out, origin + o, start[o], count[o], wo);
  }
  return 0;
}

extern "C" int64_t gad_resize_bicubic_patches_workspace_bytes(int32_t H, int32_t W, int32_t rh, int32_t rw, int32_t oy, int32_t ox,
                                                              int32_t R, int32_t P) {
  const char* why = resize_refusal(H, W, rh, rw, oy, ox, R, P);
  if (why) {
    gad_set_error("gad_resize_bicubic_patches_workspace_bytes: %s (H=%d, W=%d, rh=%d, rw=%d, oy=%d, ox=%d, R=%d, P=%d)", why, H, W,
                  rh, rw, oy, ox, R, P);
    return -1;
  }
  return (axis_floats(R, bicubic_kmax(H, rh)) + axis_floats(R, bicubic_kmax(W, rw))) * 4;
}

extern "C" int gad_resize_bicubic_patches(const float* x, float* y, int32_t B, int32_t H, int32_t W, int32_t rh, int32_t rw,
                                          int32_t oy, int32_t ox, int32_t R, int32_t P, float a, float b, void* ws,
                                          int64_t ws_bytes, void* stream) {
  GAD_CHECK(x && y && ws, "gad_resize_bicubic_patches: null pointer (x, y or ws)");
  GAD_CHECK(B >= 1 && B <= 65535, "gad_resize_bicubic_patches: B=%d must be in [1, 65535]", B);
  const char* why = resize_refusal(H, W, rh, rw, oy, ox, R, P);
  GAD_CHECK(!why, "gad_resize_bicubic_patches: %s (H=%d, W=%d, rh=%d, rw=%d, oy=%d, ox=%d, R=%d, P=%d)", why ? why : "", H, W, rh, rw,
            oy, ox, R, P);
  GAD_CHECK((double)B * 3 * H * W < TOO_LARGE && (double)B * 3 * R * R < TOO_LARGE, "gad_resize_bicubic_patches: tensor too large");
  ResizeGeom g;
  g.H = H, g.W = W, g.rh = rh, g.rw = rw, g.oy = oy, g.ox = ox, g.R = R, g.P = P, g.g = R / P;
  g.kmy = bicubic_kmax(H, rh), g.kmx = bicubic_kmax(W, rw);
  g.a = a, g.b = b;
  const int64_t need = (axis_floats(R, g.kmy) + axis_floats(R, g.kmx)) * 4;
  GAD_CHECK(ws_bytes >= need, "gad_resize_bicubic_patches: workspace of %lld bytes, %lld needed", (long long)ws_bytes, (long long)need);
  GAD_CHECK((reinterpret_cast<uintptr_t>(ws) & 3) == 0, "gad_resize_bicubic_patches: workspace must be 4-byte aligned");
  GAD_CHECK((int64_t)g.g * g.g <= 0x7fffffff, "gad_resize_bicubic_patches: too many patches per image");
  hipLaunchKernelGGL(bicubic_table_kernel, dim3((unsigned)gad_ceil_div(2 * R, NT)), dim3(NT), 0, ST, (float*)ws, g);
  GAD_LAUNCH_CHECK("gad_resize_bicubic_patches (tap tables)");
  hipLaunchKernelGGL(resize_bicubic_patches_kernel, dim3((unsigned)(g.g * g.g), (unsigned)B), dim3(NT),
                     (size_t)resize_lds_bytes(P, g.kmy, g.kmx), ST, x, y, (const float*)ws, g);
  GAD_LAUNCH_CHECK("gad_resize_bicubic_patches");
  return 0;
}

extern "C" int gad_vit_tokens(const float* patches, const float* cls, const float* pos, const float* gamma, const float* beta,
                              float* out, int32_t B, int32_t T, int32_t C, float eps, void* stream) {
  GAD_CHECK(patches && cls && pos && out, "gad_vit_tokens: null pointer (patches, cls, pos or out)");
  GAD_CHECK((gamma == nullptr) == (beta == nullptr), "gad_vit_tokens: gamma and beta are given together or not at all");
  GAD_CHECK(B >= 1 && T >= 2 && C >= 1, "gad_vit_tokens: B=%d and C=%d must be >= 1, T=%d >= 2 (class token + patches)", B, C, T);
  GAD_CHECK(gamma == nullptr || eps >= 0.f, "gad_vit_tokens: eps=%g must be >= 0", (double)eps);
  GAD_CHECK((double)B * T * C < TOO_LARGE, "gad_vit_tokens: tensor too large");
  const bool v4 = C % 4 == 0 && gad_aligned16(patches) && gad_aligned16(cls) && gad_aligned16(pos) && gad_aligned16(out) &&
                  (gamma == nullptr || (gad_aligned16(gamma) && gad_aligned16(beta)));
  const int64_t rows = (int64_t)B * T;
  if (v4) hipLaunchKernelGGL(vit_tokens_kernel<4>, dim3(gad_stream_grid(rows, WPB)), dim3(NT), 0, ST, patches, cls, pos, gamma, beta, out, rows, T, C, eps);
  else hipLaunchKernelGGL(vit_tokens_kernel<1>, dim3(gad_stream_grid(rows, WPB)), dim3(NT), 0, ST, patches, cls, pos, gamma, beta, out, rows, T, C, eps);
  GAD_LAUNCH_CHECK("gad_vit_tokens");
  return 0;
}

extern "C" int gad_gelu(float* x, int64_t rows, int32_t C, int32_t ld, int32_t kind, void* stream) {
  GAD_CHECK(x, "gad_gelu: null pointer (x)");
  GAD_CHECK(rows >= 1 && C >= 1, "gad_gelu: rows=%lld and C=%d must be >= 1", (long long)rows, C);
  GAD_CHECK(ld >= C, "gad_gelu: ld=%d < C=%d", ld, C);
  GAD_CHECK(kind == GAD_GELU_ERF || kind == GAD_GELU_QUICK, "gad_gelu: kind=%d must be 0 (erf) or 1 (QuickGELU)", kind);
  GAD_CHECK((double)rows * ld < TOO_LARGE, "gad_gelu: tensor too large");
  const bool v4 = C % 4 == 0 && ld % 4 == 0 && gad_aligned16(x);
  const int cv = v4 ? C / 4 : C;
  const int64_t total = rows * cv;
  const dim3 grid(gad_stream_grid(total, NT));
  if (v4 && kind == GAD_GELU_ERF) hipLaunchKernelGGL((gelu_kernel<4, 0>), grid, dim3(NT), 0, ST, x, total, cv, (int64_t)ld);
  else if (v4) hipLaunchKernelGGL((gelu_kernel<4, 1>), grid, dim3(NT), 0, ST, x, total, cv, (int64_t)ld);
  else if (kind == GAD_GELU_ERF) hipLaunchKernelGGL((gelu_kernel<1, 0>), grid, dim3(NT), 0, ST, x, total, cv, (int64_t)ld);
  else hipLaunchKernelGGL((gelu_kernel<1, 1>), grid, dim3(NT), 0, ST, x, total, cv, (int64_t)ld);
  GAD_LAUNCH_CHECK("gad_gelu");
  return 0;
}

extern "C" int gad_l2_normalize_rows(float* x, int64_t rows, int32_t C, int32_t ld, void* stream) {
  GAD_CHECK(x, "gad_l2_normalize_rows: null pointer (x)");
  GAD_CHECK(rows >= 1 && C >= 1, "gad_l2_normalize_rows: rows=%lld and C=%d must be >= 1", (long long)rows, C);
  GAD_CHECK(ld >= C, "gad_l2_normalize_rows: ld=%d < C=%d", ld, C);
  GAD_CHECK((double)rows * ld < TOO_LARGE, "gad_l2_normalize_rows: tensor too large");
  const bool v4 = C % 4 == 0 && ld % 4 == 0 && gad_aligned16(x);
  if (v4) hipLaunchKernelGGL(l2_normalize_kernel<4>, dim3(gad_stream_grid(rows, WPB)), dim3(NT), 0, ST, x, rows, C, (int64_t)ld);
  else hipLaunchKernelGGL(l2_normalize_kernel<1>, dim3(gad_stream_grid(rows, WPB)), dim3(NT), 0, ST, x, rows, C, (int64_t)ld);
  GAD_LAUNCH_CHECK("gad_l2_normalize_rows");
  return 0;
}
