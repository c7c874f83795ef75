// Gathers of the CLIP text towers (gad/text.py; reference text_to_image/train_text_to_image_lora.py:723-731 CLIPTextModel,
// compute_model_behaviors.py:302-306 clip.encode_text) - everything else of a pre-LN text transformer is gad_gemm,
// gad_layernorm_fwd, gad_gelu and gad_attention_causal_fwd:
//   gad_text_tokens   out[b][t] = token_emb[ids[b][t]] + pos[t]      (the embedding lookup in front of the first block)
//   gad_gather_rows   out[b]    = x[b T + rows[b]]                   (the end-of-text row of every prompt, for ln_final + projection)
// One float4 per thread, HBM-bound; indices are clamped, so neither kernel can read outside its table.
#include "gad_common.h"

namespace {

constexpr int NT = 256;

__global__ __launch_bounds__(NT) void text_tokens_kernel(const int32_t* __restrict__ ids, const float* __restrict__ emb,
                                                         const float* __restrict__ pos, float* __restrict__ out, long n4, int T, int W4,
                                                         int V) {
  const long i = (long)blockIdx.x * NT + threadIdx.x;
  if (i >= n4) return;
  const long r = i / W4;
  const int c = (int)(i - r * W4), t = (int)(r % T);
  const int id = min(max(ids[r], 0), V - 1);
  const f32x4 e = reinterpret_cast<const f32x4*>(emb)[(long)id * W4 + c];
  const f32x4 p = reinterpret_cast<const f32x4*>(pos)[(long)t * W4 + c];
  reinterpret_cast<f32x4*>(out)[i] = e + p;
}

__global__ __launch_bounds__(NT) void gather_rows_kernel(const float* __restrict__ x, const int32_t* __restrict__ rows,
                                                         float* __restrict__ out, long n4, int T, int W4, long ldx) {
  const long i = (long)blockIdx.x * NT + threadIdx.x;
  if (i >= n4) return;
  const long b = i / W4;
  const int c = (int)(i - b * W4);
  const int r = min(max(rows[b], 0), T - 1);
  reinterpret_cast<f32x4*>(out)[i] = *reinterpret_cast<const f32x4*>(x + (b * T + r) * ldx + 4 * c);
}

}  // namespace

extern "C" int gad_text_tokens(const int32_t* ids, const float* token_emb, const float* pos, float* out, int32_t B, int32_t T,
                               int32_t W, int32_t V, void* stream) {
  GAD_CHECK(ids && token_emb && pos && out, "gad_text_tokens: null pointer (ids, token_emb, pos or out)");
  GAD_CHECK(B >= 1 && T >= 1 && W >= 1 && V >= 1, "gad_text_tokens: B=%d, T=%d, W=%d and V=%d must all be >= 1", B, T, W, V);
  GAD_CHECK(W % 4 == 0, "gad_text_tokens: W=%d must be a multiple of 4", W);
  GAD_CHECK(gad_aligned16(token_emb) && gad_aligned16(pos) && gad_aligned16(out), "gad_text_tokens: token_emb / pos / out must be 16-byte aligned");
  GAD_CHECK((reinterpret_cast<uintptr_t>(ids) & 3) == 0, "gad_text_tokens: ids must be 4-byte aligned");
  const long n4 = (long)B * T * (W / 4);
  GAD_CHECK(gad_ceil_div(n4, NT) < (1L << 31), "gad_text_tokens: tensor too large");
  hipLaunchKernelGGL(text_tokens_kernel, dim3((unsigned)gad_ceil_div(n4, NT)), dim3(NT), 0, (hipStream_t)stream, ids, token_emb, pos, out,
                     n4, T, W / 4, V);
  GAD_LAUNCH_CHECK("gad_text_tokens");
  return 0;
}

extern "C" int gad_gather_rows(const float* x, const int32_t* rows, float* out, int32_t B, int32_t T, int32_t W, int64_t ldx,
                               void* stream) {
  GAD_CHECK(x && rows && out, "gad_gather_rows: null pointer (x, rows or out)");
  GAD_CHECK(B >= 1 && T >= 1 && W >= 1, "gad_gather_rows: B=%d, T=%d and W=%d must all be >= 1", B, T, W);
  GAD_CHECK(W % 4 == 0 && ldx % 4 == 0 && ldx >= W, "gad_gather_rows: W=%d and ldx=%lld must be multiples of 4, ldx >= W", W, (long long)ldx);
  GAD_CHECK(gad_aligned16(x) && gad_aligned16(out), "gad_gather_rows: x / out must be 16-byte aligned");
  GAD_CHECK((reinterpret_cast<uintptr_t>(rows) & 3) == 0, "gad_gather_rows: rows must be 4-byte aligned");
  const long n4 = (long)B * (W / 4);
  GAD_CHECK(gad_ceil_div(n4, NT) < (1L << 31), "gad_gather_rows: tensor too large");
  hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)gad_ceil_div(n4, NT)), dim3(NT), 0, (hipStream_t)stream, x, rows, out, n4, T, W / 4,
                     (long)ldx);
  GAD_LAUNCH_CHECK("gad_gather_rows");
  return 0;
}
