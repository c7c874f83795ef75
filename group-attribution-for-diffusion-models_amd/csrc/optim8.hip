// Fused gradient-clip + 8-bit blockwise Adam(W) + EMA over the flat parameter buffer (gfx950).
// Restates bitsandbytes 0.42 Adam8bit / AdamW8bit (blockwise, block 2048, min_8bit_size 4096, no percentile clipping) from
// its published description - the arithmetic pinned by this project is tests/adam8_ref.py.
// One pass: reads p, g, ema (12 B) + two codes (2 B), writes p, ema (8 B) + two codes (2 B) = 24 B/param against the fp32
// pass's 36, plus 8 B of absmax per 2048 parameters.  One launch, no atomics, no host sync; the clip coefficient comes from the
// gad_sumsq scalar on the device as in optim.hip, so the step stays hipGraph-capturable.
//
// One workgroup of 256 threads works through block descriptors (gad_adam8_block): thread t owns elements 4t..4t+3 and
// 1024+4t..1024+4t+3 of the block, so every 16-byte load of p / g / ema is fully coalesced and the codes go out as 4 B per lane.
// Dequantisation is an LDS lookup; the new absmax is a wave reduction followed by four LDS words (a max: order-independent, so
// the result is bit-reproducible); requantisation is an 8-step search over the maps' 255 lower values held in LDS in
// breadth-first (Eytzinger) order - the nodes of one level are neighbours, so the first six levels meet no bank conflict where a
// sorted array would put every level on one bank - and then one comparison of the two neighbours in the sorted copy.
#include <math.h>

#include "gad_common.h"

namespace {
constexpr int A8_BLOCK = 2048, A8_THREADS = 256;

struct Maps { float s[256]; float u[256]; };      // signed (first moment), unsigned (second moment); ascending

// midpoint k of linspace(0.1, 1, n + 1) in double; 2n is a power of two, so the only roundings are the product and the sum
constexpr double a8_mid(int k, int n) { return 0.1 + (0.9 * (double)(2 * k + 1)) / (double)(2 * n); }

constexpr Maps a8_make_maps() {
  constexpr double inv10[7] = {1e6, 1e5, 1e4, 1e3, 1e2, 1e1, 1e0};      // exact in double: the decade is applied by one division
  Maps m{};
  int j = 0;
  for (int i = 0; i < 7; ++i) {
    int n = 1 << i;
    for (int k = 0; k < n; ++k, ++j) {
      float v = (float)(a8_mid(k, n) / inv10[i]);
      m.s[128 + j] = v;
      m.s[126 - j] = -v;
    }
  }
  m.s[127] = 0.f;
  m.s[255] = 1.f;
  j = 0;
  for (int i = 0; i < 7; ++i) {
    int n = 2 << i;
    for (int k = 0; k < n; ++k, ++j) m.u[1 + j] = (float)(a8_mid(k, n) / inv10[i]);
  }
  m.u[0] = 0.f;
  m.u[255] = 1.f;
  return m;
}

constexpr Maps h_maps = a8_make_maps();           // what gad_adam8_qmap hands out
__constant__ Maps c_maps = a8_make_maps();        // what the kernel stages into LDS: the same constant expression

struct Adam8Dev {
  float* p; const float* g; float* ema;
  uint8_t* c1; uint8_t* c2;
  float* am1; float* am2; float* m32; float* v32;
  const gad_adam8_block* blocks;
  int nblocks, n_absmax;
  long n, n32;
  const float* sumsq;
  float max_norm, lr, b1, b2;
  float step_size, eps_c, ema_om;   // lr*sqrt(1-beta2^t)/(1-beta1^t), eps*sqrt(1-beta2^t), 1-ema_decay
};

// index of the map value nearest to x, the lower one on a tie.  e: the map's values 0..254 in breadth-first order (root at 1),
// a: the sorted map.  k never leaves [1, 511] whatever x is (NaN included), so no lookup can leave the tables.
__device__ __forceinline__ int a8_nearest(const float* e, const float* a, float x) {
  int k = 1;
#pragma unroll
  for (int s = 0; s < 8; ++s) k = 2 * k + (e[k] < x ? 1 : 0);
  int c = k - 256;                  // how many of a[0..254] lie below x
  if (c == 0) return 0;
  return (x - a[c - 1] <= a[c] - x) ? c - 1 : c;
}

__global__ __launch_bounds__(A8_THREADS) void adam8_kernel(const Adam8Dev a) {
  __shared__ float s_map1[256], s_map2[256], s_e1[256], s_e2[256];
  __shared__ float s_red[2][2][4];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  s_map1[t] = c_maps.s[t];
  s_map2[t] = c_maps.u[t];
  {
    int src = 0;
    if (t > 0) {
      int L = 31 - __clz(t), j = t - (1 << L);
      src = ((2 * j + 1) << (7 - L)) - 1;        // in-order position of breadth-first node t in a perfect tree of 255
    }
    s_e1[t] = c_maps.s[src];
    s_e2[t] = c_maps.u[src];
  }
  __syncthreads();
  float coef = 1.f;
  if (a.sumsq) {
    float c = a.max_norm / (sqrtf(a.sumsq[0]) + 1e-6f);
    coef = c < 1.f ? c : 1.f;
  }
  const float om1 = 1.f - a.b1, om2 = 1.f - a.b2;
  int par = 0;
  for (int b = blockIdx.x; b < a.nblocks; b += gridDim.x) {
    const gad_adam8_block d = a.blocks[b];
    const long off = d.offset;
    const int len = d.len, st = d.state, is32 = d.fp32;
    // a descriptor that points outside the buffers is skipped, never followed (workgroup-uniform)
    if (len < 1 || len > A8_BLOCK || off < 0 || (off & 7) || off + len > a.n) continue;
    if (is32 ? (st < 0 || (st & 3) || (long)st + len > a.n32) : (st < 0 || st >= a.n_absmax)) continue;
    const float decay = d.weight_decay > 0.f ? 1.f - a.lr * d.weight_decay : 1.f;
    float am1 = 0.f, am2 = 0.f;
    if (!is32) { am1 = a.am1[st]; am2 = a.am2[st]; }
    f32x4 m[2], v[2];
    int cnt[2];
    float mx1 = 0.f, mx2 = 0.f;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int e0 = 4 * (h * A8_THREADS + t);
      const int c = len - e0 < 0 ? 0 : (len - e0 > 4 ? 4 : len - e0);
      cnt[h] = c;
      const long i = off + e0;
      f32x4 p = {0, 0, 0, 0}, g = {0, 0, 0, 0}, e = {0, 0, 0, 0}, mm = {0, 0, 0, 0}, vv = {0, 0, 0, 0};
      if (c == 4) {
        p = *reinterpret_cast<const f32x4*>(a.p + i);
        g = *reinterpret_cast<const f32x4*>(a.g + i);
        if (a.ema) e = *reinterpret_cast<const f32x4*>(a.ema + i);
        if (is32) {
          mm = *reinterpret_cast<const f32x4*>(a.m32 + st + e0);
          vv = *reinterpret_cast<const f32x4*>(a.v32 + st + e0);
        } else {
          uint32_t q1 = *reinterpret_cast<const uint32_t*>(a.c1 + i), q2 = *reinterpret_cast<const uint32_t*>(a.c2 + i);
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            mm[k] = s_map1[(q1 >> (8 * k)) & 255] * am1;
            vv[k] = s_map2[(q2 >> (8 * k)) & 255] * am2;
          }
        }
      } else {
        for (int k = 0; k < c; ++k) {
          p[k] = a.p[i + k];
          g[k] = a.g[i + k];
          if (a.ema) e[k] = a.ema[i + k];
          if (is32) {
            mm[k] = a.m32[st + e0 + k];
            vv[k] = a.v32[st + e0 + k];
          } else {
            mm[k] = s_map1[a.c1[i + k]] * am1;
            vv[k] = s_map2[a.c2[i + k]] * am2;
          }
        }
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (k < c) {
          float gk = g[k] * coef;
          float mk = mm[k] * a.b1 + om1 * gk;
          float vk = vv[k] * a.b2 + om2 * gk * gk;
          float pk = p[k] - a.step_size * mk / (sqrtf(vk) + a.eps_c);
          pk *= decay;
          p[k] = pk;
          e[k] = e[k] - a.ema_om * (e[k] - pk);
          mm[k] = mk;
          vv[k] = vk;
          mx1 = fmaxf(mx1, fabsf(mk));
          mx2 = fmaxf(mx2, vk);
        }
      }
      if (c == 4) {
        *reinterpret_cast<f32x4*>(a.p + i) = p;
        if (a.ema) *reinterpret_cast<f32x4*>(a.ema + i) = e;
        if (is32) {
          *reinterpret_cast<f32x4*>(a.m32 + st + e0) = mm;
          *reinterpret_cast<f32x4*>(a.v32 + st + e0) = vv;
        }
      } else {
        for (int k = 0; k < c; ++k) {
          a.p[i + k] = p[k];
          if (a.ema) a.ema[i + k] = e[k];
          if (is32) {
            a.m32[st + e0 + k] = mm[k];
            a.v32[st + e0 + k] = vv[k];
          }
        }
      }
      m[h] = mm;
      v[h] = vv;
    }
    if (is32) continue;
    // new absmax of the block: wave reduction, then the four waves through LDS (double-buffered: one barrier per block)
    mx1 = wave_max(mx1);
    mx2 = wave_max(mx2);
    if (lane == 0) {
      s_red[par][0][wave] = mx1;
      s_red[par][1][wave] = mx2;
    }
    __syncthreads();
    const float n1 = fmaxf(fmaxf(s_red[par][0][0], s_red[par][0][1]), fmaxf(s_red[par][0][2], s_red[par][0][3]));
    const float n2 = fmaxf(fmaxf(s_red[par][1][0], s_red[par][1][1]), fmaxf(s_red[par][1][2], s_red[par][1][3]));
    par ^= 1;
    if (t == 0) {
      a.am1[st] = n1;
      a.am2[st] = n2;
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int c = cnt[h];
      const long i = off + 4 * (h * A8_THREADS + t);
      uint32_t q1 = 0, q2 = 0;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        int i1 = 127, i2 = 0;                          // the zero codes: what a block of absmax 0 holds, with no division
        if (k < c) {
          if (n1 > 0.f) {
            i1 = a8_nearest(s_e1, s_map1, m[h][k] / n1);
            if (i1 == 127 && m[h][k] < 0.f) i1 = 126;  // a negative moment keeps its sign
          }
          if (n2 > 0.f) i2 = a8_nearest(s_e2, s_map2, v[h][k] / n2);
        }
        q1 |= (uint32_t)i1 << (8 * k);
        q2 |= (uint32_t)i2 << (8 * k);
      }
      if (c == 4) {
        *reinterpret_cast<uint32_t*>(a.c1 + i) = q1;
        *reinterpret_cast<uint32_t*>(a.c2 + i) = q2;
      } else {
        for (int k = 0; k < c; ++k) {
          a.c1[i + k] = (uint8_t)(q1 >> (8 * k));
          a.c2[i + k] = (uint8_t)(q2 >> (8 * k));
        }
      }
    }
  }
}
}  // namespace

extern "C" int gad_adam8_qmap(int is_signed, float* out256) {
  GAD_CHECK(out256, "gad_adam8_qmap: null output");
  memcpy(out256, is_signed ? h_maps.s : h_maps.u, 256 * sizeof(float));
  return 0;
}

extern "C" int gad_clip_adam8_ema(const gad_adam8_args* a, void* stream) {
  GAD_CHECK(a && a->p && a->g && a->state1 && a->state2 && a->absmax1 && a->absmax2 && a->m32 && a->v32 && a->blocks,
            "gad_clip_adam8_ema: null pointer");
  GAD_CHECK(a->n > 0 && a->n32 >= 0 && a->n_absmax >= 0 && a->n_blocks > 0, "gad_clip_adam8_ema: empty buffer or descriptor table");
  GAD_CHECK(a->step >= 1, "gad_clip_adam8_ema: step must be >= 1");
  GAD_CHECK(gad_aligned16(a->p) && gad_aligned16(a->g) && gad_aligned16(a->ema) && gad_aligned16(a->state1) && gad_aligned16(a->state2) &&
                gad_aligned16(a->m32) && gad_aligned16(a->v32) && ((uintptr_t)a->absmax1 & 3) == 0 && ((uintptr_t)a->absmax2 & 3) == 0 &&
                ((uintptr_t)a->blocks & 7) == 0,
            "gad_clip_adam8_ema: buffers must be 16-byte aligned");
  Adam8Dev d;
  d.p = a->p; d.g = a->g; d.ema = a->ema;
  d.c1 = a->state1; d.c2 = a->state2;
  d.am1 = a->absmax1; d.am2 = a->absmax2; d.m32 = a->m32; d.v32 = a->v32;
  d.blocks = a->blocks; d.nblocks = a->n_blocks; d.n_absmax = a->n_absmax;
  d.n = a->n; d.n32 = a->n32;
  d.sumsq = a->sumsq; d.max_norm = a->max_norm;
  d.lr = a->lr; d.b1 = a->beta1; d.b2 = a->beta2;
  double bc1 = 1.0 - pow((double)a->beta1, (double)a->step), sbc2 = sqrt(1.0 - pow((double)a->beta2, (double)a->step));
  d.step_size = (float)((double)a->lr * sbc2 / bc1);
  d.eps_c = (float)((double)a->eps * sbc2);
  d.ema_om = 1.f - a->ema_decay;
  // 96 VGPRs: five workgroups fit a CU.  Four per CU on 256 CUs are all resident at once, so every workgroup stages the maps once
  // and the descriptors are dealt round-robin with no second, partly filled round of workgroups
  int blocks = a->n_blocks < 1024 ? a->n_blocks : 1024;
  hipLaunchKernelGGL(adam8_kernel, dim3((unsigned)blocks), dim3(A8_THREADS), 0, (hipStream_t)stream, d);
  GAD_LAUNCH_CHECK("gad_clip_adam8_ema");
  return 0;
}
