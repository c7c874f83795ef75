// Shared helpers for the gfx950 kernels (host + device).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "gad.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

void gad_set_error(const char* fmt, ...);

#define GAD_CHECK(cond, ...)        \
  do {                              \
    if (!(cond)) {                  \
      gad_set_error(__VA_ARGS__);   \
      return 1;                     \
    }                               \
  } while (0)

#define GAD_LAUNCH_CHECK(name)                                            \
  do {                                                                    \
    hipError_t e_ = hipGetLastError();                                    \
    if (e_ != hipSuccess) {                                               \
      gad_set_error("%s: launch failed: %s", name, hipGetErrorString(e_)); \
      return 2;                                                           \
    }                                                                     \
  } while (0)

static inline bool gad_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
static inline int64_t gad_ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// Grid of a streaming (grid-stride, HBM-bound) kernel: one workgroup per `per_block` items up to 2048 workgroups - 256 CUs x 8
// resident workgroups of 256 threads - and the loop strides over the rest.  n_items >= 1.
constexpr int GAD_STREAM_MAX_BLOCKS = 2048;
static inline unsigned gad_stream_grid(int64_t n_items, int per_block = 256) {
  const int64_t b = gad_ceil_div(n_items, per_block);
  return (unsigned)(b < GAD_STREAM_MAX_BLOCKS ? b : GAD_STREAM_MAX_BLOCKS);
}
// rows x chunks form: x covers one row's n_items as above, y as many of the rows as keep the whole grid inside the same bound
static inline dim3 gad_stream_grid_rows(int64_t rows, int64_t n_items) {
  const int64_t gx = gad_stream_grid(n_items), fit = GAD_STREAM_MAX_BLOCKS / gx;
  return dim3((unsigned)gx, (unsigned)(rows < fit ? rows : fit));
}

// wave64 sum reduction (all lanes get the total)
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// GroupNorm forward (norm.hip, half.hip): sum x^2 - (sum x)^2 / n cancels where a group's mean lies far from zero against its
// spread, and the result shows it: SS / m2 = 1 + (mean / std)^2 is the factor by which the sums' rounding is magnified.  Up to
// GN_COND (|mean| / std < 3.9: four bits, inside what another summation order costs) the one-sweep sums stand; beyond it the
// chunk is summed again, centred.
constexpr float GN_COND = 16.f;
