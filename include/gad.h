/* gad.h - C ABI of the MI355X (gfx950) hot-path library `libgad_hip.so`.
 *
 * The reference (q8888620002/Group-Attribution-for-Diffusion-Models) has no FFI of
 * its own: its hot path is reached through the Python API of the third-party
 * diffusers==0.24.0 wheel, which dispatches to ATen/cuDNN/cuBLAS kernels.  Each entry
 * point below names the reference call site whose device work it replaces
 * (paths relative to the reference root).  The Python host layer
 * (group-attribution-for-diffusion-models_amd/gad) binds these with ctypes; the binding a
 * reference maintainer would add is shown in INTEGRATION.md.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer to caller-owned memory (PyTorch allocates);
 *     the library never allocates, frees or retains device memory;
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*), never
 *     synchronises the device and is re-entrant / hipGraph-capturable;
 *   - returns 0 on success, non-zero on error; gad_last_error() gives the
 *     thread-local message;
 *   - activations are fp32 NHWC ([B][H][W][C], "pixel-major"), conv weights are
 *     [Cout][KH][KW][Cin] (= torch channels_last storage of the diffusers
 *     [Cout][Cin][KH][KW] parameter), Linear weights [out][in].
 */
#ifndef GAD_H
#define GAD_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

int gad_version(void);
const char* gad_last_error(void);

/* ------------------------------------------------------------------------------
 * Contraction engine (f32-input MFMA v_mfma_f32_32x32x2_f32, exact fp32).
 * C[z][M][N] = epilogue( alpha * sum_k A[z](m,k) * B[z](k,n) )
 * Replaces cuDNN conv fwd/dgrad/wgrad and cuBLAS GEMMs under
 *   diffusers ResnetBlock2D / Downsample2D / Upsample2D / Attention
 *   (unconditional_generation/main.py:707,713; src/diffusion_utils.py:336-341;
 *    src/diffusers/models/attention_processor.py:1301-1329).
 * ---------------------------------------------------------------------------- */
enum gad_a_mode {
  GAD_A_KC = 0,     /* dense A[m][k], k contiguous, row stride lda                       */
  GAD_A_MC = 1,     /* dense A[k][m], m contiguous, row stride lda (i.e. A^T stored)    */
  GAD_A_CONV = 2,   /* im2col gather of NHWC x: m=(img,oh,ow), k=(r,s,c)   (conv fwd)   */
  GAD_A_CONVT = 3   /* transposed gather of NHWC dy: m=(img,ih,iw), k=(r,s,co) (dgrad)  */
};
enum gad_b_mode {
  GAD_B_KC = 0,     /* B[n][k], k contiguous, row stride ldb (torch Linear / conv weight)*/
  GAD_B_MC = 1,     /* B[k][n], n contiguous, row stride ldb                             */
  GAD_B_WDGRAD = 2, /* conv weight W[co][r][s][ci] read as B[k=(r,s,co)][n=ci]  (dgrad)  */
  GAD_B_CONV = 3    /* im2col gather of NHWC x as B[k=(img,oh,ow)][n=(r,s,c)]  (wgrad)   */
};

typedef struct gad_conv_geom {
  int32_t H, W, C;          /* gathered tensor: spatial size and channels (before upsample)   */
  int32_t ldx;              /* pixel stride of the gathered tensor in floats (>= C)          */
  int32_t Ho, Wo;           /* spatial size of the GEMM-row (A) / GEMM-k (B_CONV) pixel grid */
  int32_t KH, KW;
  int32_t stride;
  int32_t pad_t, pad_l;
  int32_t upsample;         /* 1: gathered tensor is nearest-2x upsampled on the fly         */
} gad_conv_geom;

typedef struct gad_gemm_args {
  const float* A;
  const float* B;
  float* C;
  int32_t a_mode, b_mode;
  int32_t M, N, K;
  int32_t lda, ldb, ldc;
  /* batch z = z0 * batch_inner + z1 ; pointer offset = z0*stride?0 + z1*stride?1 (floats) */
  int32_t batch, batch_inner;
  /* With batch > 1 the strides are part of the float4 decision (gad_gemm_plan's vec): an A or B stride that is not a
   * multiple of 4 floats puts the launch on the dword loaders (vec 1, fp32 products whatever operand_precision says), a C
   * stride that is not one puts it on the scalar epilogue.  With batch <= 1 they are ignored. */
  int64_t strideA0, strideA1, strideB0, strideB1, strideC0, strideC1;
  gad_conv_geom g;          /* used by the CONV / CONVT / WDGRAD / B_CONV modes              */
  /* epilogue: C = alpha*acc + bias[n] + rowadd[m / rows_per_group][n] + residual[m][n]      */
  float alpha;
  const float* bias;        /* [N] or NULL                                                   */
  const float* rowadd;      /* [M / rows_per_group][ld_rowadd] or NULL (time-embedding add)  */
  int32_t rows_per_group, ld_rowadd;
  const float* residual;    /* [M][ldr] or NULL (same batch strides as C)                    */
  int32_t ldr;
  /* split-K workspace (caller owned). ws_bytes >= gad_gemm_workspace_bytes(args)            */
  void* ws;
  int64_t ws_bytes;
  int32_t tile_hint;        /* 0 = auto, 1 = force 128x128, 2 = force 64x64, 3 = 128x64 (dense fp32 forms); 7 / 8 = a forward 3x3 convolution
                             * with B_wino / B_wino4 takes the F(2x2) / F(4x4) Winograd route whatever the planner models (tests, A/B tools); 3x3 weight gradient:
                             * 1 / 4 / 5 / 6 = 128 / 96 / 64 / 32 output channels per tile, 1000 + m1 = rows [0, m1) on 128-channel
                             * tiles and the rest planned, as a second launch (A/B tools) */
  int32_t splitk_hint;      /* 0 = auto, >0 = force                                          */
  /* 0: fp32 operands on v_mfma_f32_32x32x2_f32 (exact products; the reference's default precision).
   * 1: A and B may be rounded to bf16 (RNE) in flight and multiplied on v_mfma_f32_32x32x16_bf16 with fp32
   *    accumulation - the analogue of the reference's `--mixed_precision` autocast
   *    (text_to_image/train_text_to_image_lora.py:659-668) - whenever both operands can be read as 16-B aligned
   *    float4 (else the launch runs in fp32).  gad_gemm_uses_bf16() tells which. */
  int32_t operand_precision;
  /* A_CONV only: the gathered tensor is the channel concatenation of A ([..][ldx >= a_split], channels
   * [0, a_split)) and A2 ([..][ldx2], channels [a_split, g.C)) - UpBlock2D's torch.cat without the copy.
   * A2 == NULL: single source.  a_split must be a multiple of 32. */
  const float* A2;
  int32_t a_split, ldx2;
  /* optional bf16 copy of B (same [N][ldb] layout, k contiguous, RNE-rounded; 16-B aligned, ldb % 8 == 0): with
   * operand_precision = 1 the LDS-patch convolution streams it by LDS-DMA instead of converting the fp32 weights in every
   * workgroup.  Ignored by every other kernel. */
  const void* B_bf16;
  /* K-concatenated dense operands - the fused LoRA-compatible linear (diffusers LoRACompatibleLinear as injected at
   * text_to_image/train_text_to_image_lora.py:786-820): for k >= k_split the products read A_k2[m][k - k_split] and
   * B_k2 (laid out like B: [n][k - k_split] for B_KC, [k - k_split][n] for B_MC), so
   *   y = x W^T + mid (s B_up)^T            is ONE launch with A = x, A_k2 = mid, B = W, B_k2 = B_up   (forward)
   *   dx = dy W + dmid A_down               is ONE launch with A = dy, A_k2 = dmid, B = W, B_k2 = A_down (B_MC)
   * instead of a base GEMM plus a residual-accumulating side GEMM.  A_KC x B_KC|B_MC only; k_split % 32 == 0;
   * (K - k_split) % 4 == 0 (ragged LoRA ranks that are not multiples of 4 take the two-launch route). */
  const float* A_k2;
  const float* B_k2;
  int32_t lda_k2, ldb_k2, k_split;
  /* kernel-family switches for A/B tests and invariance checks (0 in production): GAD_GEMM_* bits below.  They
   * travel with the call - the library reads no environment variable and keeps no process-global switch. */
  int32_t flags;
  /* Winograd F(2x2, 3x3) route of the fp32 3x3 / stride 1 / pad 1 forward convolution (A_CONV x B_KC, even output maps,
   * Cin % 32 == 0, N % 4 == 0, N >= 64, single source, float4-addressable epilogue operands): B_wino = the transformed weights
   * U[16][Cout][Cin] = G w G^T made by gad_wino_weights from the [Cout][3][3][Cin] storage B points at; wino_ws = scratch
   * of gad_gemm_wino_bytes(args) bytes for the transformed input V[16][tiles][Cin].  B_wino == NULL (or a launch the
   * planner models no faster than the direct kernels: gad_gemm_wino_bytes returns 0): the direct kernels run and both are
   * ignored.  fp32 throughout; equal to the direct kernels up to fp32 reassociation / transform rounding, deterministic.
   * Replaces what cuDNN's own algorithm choice does for these convolutions in the reference (torch.nn.Conv2d of
   * diffusers' ResnetBlock2D.conv1 / conv2, Upsample2D.conv). */
  const float* B_wino;
  void* wino_ws;
  int64_t wino_ws_bytes;
  /* the F(4x4, 3x3) form of the same route (output maps that are multiples of 4): B_wino4 = U[36][Cout][Cin] made by
   * gad_wino4_weights.  With both forms given the planner takes whichever models fastest (or neither); wino_ws then holds the
   * transformed input AND the 36 product panels (gad_gemm_wino_bytes covers both), ws may be needed for a split of the batched
   * products (gad_gemm_workspace_bytes as usual).  4x fewer multiplies than the direct form; 15-20x the error of the
   * direct fp32 kernels on N(0, 1) data (measured 2.1e-5 .. 2.9e-5 at |y| <= 4.8, ~6e-6 of the output scale, against 1.4e-6; no
   * more than an fp32 run of the textbook transforms loses - profiles/conv_conditioning.txt).  Large launches run the one-launch form
   * (csrc/wino4_fused.hip: all 36 products and the output transform in one kernel, wino_ws holds V only); the planner decides,
   * tile_hint 9 / 10 force the one-launch / three-launch forms (tests, A/B tools). */
  const float* B_wino4;
} gad_gemm_args;
enum gad_gemm_flags {
  GAD_GEMM_NO_WINO = 16,      /* never take the Winograd route even when B_wino is given                              */
  GAD_GEMM_WINO_WGRAD = 32,   /* a 3x3 / stride 1 / pad 1 weight gradient (A_MC x B_CONV, output maps multiples of 4) may run in Winograd
                               * F(4x4, 3x3) form: dW = G^T [sum_tiles (A dy A^T) (.) (B^T x B)] G; wino_ws = gad_gemm_wino_bytes(args) bytes
                               * of scratch (transformed dy and x, the 36 product panels); the planner decides (tile_hint 8 forces).  With
                               * GAD_GEMM_WINO_SKIP_INPUT and B_wino4 = the V image [36][B Ho Wo / 16][Cin] the F(4x4) FORWARD launch of the same
                               * convolution left at the start of its wino_ws, the input is not transformed again (bit-identical result) */
  GAD_GEMM_NO_PATCH = 1,      /* never take the LDS-patch convolution kernels (generic im2col-gather engine instead) */
  GAD_GEMM_TAP_MAJOR_K = 2,   /* conv gathers walk K as (tap, channel chunk) instead of (channel chunk, tap)        */
  GAD_GEMM_SCALAR_EPILOGUE = 4, /* dword stores straight from the accumulators instead of the LDS-transposed float4 epilogue */
  GAD_GEMM_GENERAL_LOADERS = 8, /* dense operands with K % 32 == 0: the masking loaders instead of the lean (row-clamping) ones */
  /* Stages of a Winograd forward launch, so that a caller can put an event between them (bench.py's per-stage roofline) or
   * supply the transformed input itself: ONLY_INPUT runs the input transform x -> V into wino_ws and returns; SKIP_INPUT
   * takes wino_ws as already holding V (written by an ONLY_INPUT call with the same arguments) and runs the rest.  The two
   * calls back to back are the same kernels in the same order as one plain call: bit-identical.  Both are refused (gad_gemm
   * returns non-zero, nothing launched) off their route: ONLY_INPUT unless the launch takes the F(2x2) / F(4x4) forward route
   * (gad_gemm_kernel_id 5 / 6), SKIP_INPUT unless it takes one of those or the Winograd weight gradient (7). */
  GAD_GEMM_WINO_ONLY_INPUT = 64,
  GAD_GEMM_WINO_SKIP_INPUT = 128
};

int64_t gad_gemm_workspace_bytes(const gad_gemm_args* a);
/* which kernel instance gad_gemm would launch: tile, split-K factor, vector width (4 or 1).  tile by route: generic engine
 * 128 or 64 (128 also stands for its 128 x 64 form), split-K as planned; fp32 patch forward / data gradient the channel tile
 * 96 / 128 / 160, split-K over channel chunks; patch weight gradient the output-channel tile 128 / 96 / 64 / 32, split =
 * pixel splits; the two-launch N and M splits 224 (split: that of the single launch they replace); bf16 patch 128, split 1;
 * vector-ALU conv_out 256 pixels, split 1; Winograd F(2x2) the channel tile, F(4x4) 128 (one-launch form: its block's tile
 * extent 32 / 64 / 65), Winograd weight gradient 128 - split 1 for all three (the form's, not its sub-launch's) */
int gad_gemm_plan(const gad_gemm_args* a, int32_t* tile, int32_t* splitk, int32_t* vec);
int gad_gemm(const gad_gemm_args* a, void* stream);
int gad_gemm_uses_bf16(const gad_gemm_args* a);   /* 1 if gad_gemm(a) would multiply bf16-rounded operands */
/* which kernel family gad_gemm(a) launches: 0 gemm_kernel (fp32, im2col-gather / dense loaders), 1 gemm_bf16_kernel,
 * 2 conv3x3_patch_f32_kernel / wgrad3x3_patch_f32_kernel, 3 conv3x3_patch_bf16_kernel (3x3 / stride 1 / pad 1 convs whose
 * 128-pixel tiles are whole image rows: input patch resident in LDS), 4 conv3x3_fewout_kernel (<= 4 output channels:
 * vector ALUs, weights through the scalar cache) */
int gad_gemm_kernel_id(const gad_gemm_args* a);   /* ... 5 wino_input_kernel + wino_gemm_kernel (Winograd F(2x2, 3x3)), 6 wino4_input_kernel + wino4_gemm_kernel / batched gemm_kernel + wino4_output_kernel (F(4x4, 3x3)), 7 the F(4x4, 3x3) weight gradient
 * (wino4_dy_kernel + wino4_input_kernel + batched gemm_kernel + wino4_dw_kernel) */
/* bytes of wino_ws the Winograd route of gad_gemm(a) needs; 0 when gad_gemm(a) runs a direct kernel (set B_wino first) */
int64_t gad_gemm_wino_bytes(const gad_gemm_args* a);
/* Winograd weight transform U = G w G^T for the 3x3 weights listed in `table`: n_tiles rows of six int64
 * {src offset, dst offset, Cout, Cin, co0, ci0} (offsets in floats from src / dst; one 32 x 32 (co, ci) tile per row);
 * src storage [Cout][3][3][Cin] (diffusers Conv2d weight in channels_last: ResnetBlock2D.conv1/conv2, Up/Downsample2D.conv,
 * SURVEY Appendix A), dst storage [16][Cout][Cin].  One launch transforms every 3x3 weight of a flat parameter buffer. */
int gad_wino_weights(const float* src, float* dst, const int64_t* table, int64_t n_tiles, void* stream);
/* the same for F(4x4, 3x3): dst storage [36][Cout][Cin] */
int gad_wino4_weights(const float* src, float* dst, const int64_t* table, int64_t n_tiles, void* stream);

/* ------------------------------------------------------------------------------
 * GroupNorm (+ optional SiLU), NHWC.  Replaces ATen native_group_norm + SiLU in
 * ResnetBlock2D.norm1/norm2, Attention.group_norm, UNet2DModel.conv_norm_out
 * (diffusers; semantics SURVEY Appendix A.2/A.6; attention_processor.py:1297-1298).
 *   y = act( (x - mean_bg) * rstd_bg * gamma_c + beta_c ),  act = SiLU if silu != 0
 * mean/rstd [B][G] are written for the backward pass.
 * ws: gad_groupnorm_workspace_bytes() bytes of scratch.
 * ---------------------------------------------------------------------------- */
typedef struct gad_groupnorm_args {
  const float* x;           /* [B][HW][C]                                                    */
  float* y;                 /* fwd: output. bwd: dx                                          */
  const float* gamma;       /* [C]                                                           */
  const float* beta;        /* [C]                                                           */
  float* mean;              /* [B][G]  (fwd: out, bwd: in)                                   */
  float* rstd;              /* [B][G]                                                        */
  const float* dy;          /* bwd only: [B][HW][C]                                          */
  float* dgamma;            /* bwd only: [C] (overwritten); NULL together with dbeta: no affine gradients */
  float* dbeta;             /* bwd only: [C] (overwritten)                                   */
  int32_t B, HW, C, G;
  float eps;
  int32_t silu;
  void* ws;
  int64_t ws_bytes;
  /* forward only: channel-concatenated input without the concat (UpBlock2D's torch.cat([h, skip], 1),
   * SURVEY A.1): channels [0, C1) come from x ([B][HW][C1]) and [C1, C) from x2 ([B][HW][C-C1]).
   * x2 == NULL: single source.  C1 % 4 == 0 and (C - C1) % 4 == 0; both the one-pass and the two-pass plan read two sources. */
  const float* x2;
  int32_t C1;
  int32_t flags;            /* GAD_GN_TWO_PASS = 1: force the two-pass plan (A/B tests); 0 in production          */
  /* backward only: dx = (gradient through the norm) + dx_add ([B][HW][C], may alias nothing else): the gradient of a
   * second consumer of x - the residual branch of ResnetBlock2D / the attention block, whose input feeds both the norm
   * and the skip - summed in the store instead of by a separate elementwise launch.  NULL: none. */
  const float* dx_add;
} gad_groupnorm_args;
enum gad_groupnorm_flags { GAD_GN_TWO_PASS = 1 };

int64_t gad_groupnorm_workspace_bytes(const gad_groupnorm_args* a);
/* 1 if the forward of these shapes (incl. the x2/C1 split, if any) runs as the one-pass register-slab kernel */
int gad_groupnorm_one_pass(const gad_groupnorm_args* a);
int gad_groupnorm_silu_fwd(const gad_groupnorm_args* a, void* stream);
int gad_groupnorm_silu_bwd(const gad_groupnorm_args* a, void* stream);
/* Forward whose consumer is a 3x3 / stride-1 convolution on the Winograd F(4x4, 3x3) route of gad_gemm (ResnetBlock2D's
 * norm -> silu -> conv, reference diffusers ResnetBlock2D.forward): writes V[36][B * (H/4) * (W/4)][C] = B^T y_patch B - what
 * the route's own input transform would make of y - instead of y (a->y is ignored and may be NULL), plus mean / rstd.  The
 * convolution then runs with GAD_GEMM_WINO_SKIP_INPUT and wino_ws = V.  W = the map's width (HW = H * W, both multiples of 4),
 * C % 32 == 0, channels per group a multiple of 4; gad_groupnorm_wino4_ok tells whether a plan exists (the normalised
 * (image, channel slab) must fit 128 KB of LDS: up to 32 x 32 maps).  Same normalisation and transform arithmetic as the two
 * separate launches; the moments are reduced in the order of this kernel's channel slabs, so V equals theirs to fp32 rounding
 * (bit for bit where both cut the same slabs). */
int gad_groupnorm_wino4_ok(const gad_groupnorm_args* a, int32_t W);
int gad_groupnorm_silu_wino4(const gad_groupnorm_args* a, float* V, int32_t W, void* stream);

/* ------------------------------------------------------------------------------
 * Fused attention core: o = softmax(scale * q k^T) v per (batch, head), the score matrix never leaves the CU
 * (online softmax over streamed K/V tiles).  Replaces F.scaled_dot_product_attention of AttnProcessor2_0
 * (src/diffusers/models/attention_processor.py:1314-1325): UNet2DModel attention blocks (head dim 256 on CIFAR, 32 on
 * CelebA-HQ) and the self / cross attentions of the SD U-Net (head dims 40 / 80 / 160, Tk = Tq or 77;
 * text_to_image/train_text_to_image_lora.py:1268-1270).
 * Operands are [B][T][heads*d]-shaped views: row r of batch b, head h starts at base + b*stride + r*ld + h*d, so q, k, v
 * may be column blocks of one fused [B*T][3C] projection output (ld = 3C).  Any head dim 1 <= d <= 256
 * (gad_attention_supported).  Launches with d in {16, 24, 32, 40, 48, 64, 80, 96, 128, 160, 192, 224, 256}, every ld and
 * stride a multiple of 4 floats and every pointer 16-byte aligned stream their tiles by LDS-DMA; any other head dim or
 * alignment - the head-grouped-pruned CelebA-HQ model keeps its heads and shrinks the head dim 32 -> 23
 * (unconditional_generation/prune.py:337-342): rows of 322 floats - runs the next larger instance in its dword-staged
 * form (always exact fp32: gad_attention_uses_bf16 tells).
 * fwd writes o and, if lse != NULL, lse[b][h][q] = log2(sum_k exp2(scale*log2(e)*(q.k)))  (the statistics the backward
 * pass recomputes the probabilities from).  bwd needs q, k, v, o, lse, d_o and a caller-owned scratch `delta` of
 * B*heads*Tq floats; it writes dq, dk, dv (no atomics: every element is written once, bit-reproducibly).  Exact-fp32
 * launches up to d = 96 run ONE kernel per key block (S and dP computed once: the five products of the minimal scheme); key
 * blocks of one (b, h) leave dQ partials in `ws` and a fixed-order reduce sums them.  Wider heads and bf16-operand
 * launches run a dQ kernel + a dK/dV kernel that each recompute S and dP.
 * ---------------------------------------------------------------------------- */
typedef struct gad_attention_args {
  const float* q; const float* k; const float* v;
  float* o;                 /* fwd: out; bwd: in                                              */
  float* lse;               /* [B][heads][Tq]; fwd: out (may be NULL); bwd: in                */
  const float* d_o;         /* bwd: gradient w.r.t. o                                         */
  float* delta;             /* bwd scratch [B][heads][Tq]                                     */
  float* dq; float* dk; float* dv;
  int32_t B, heads, Tq, Tk, d;
  int32_t ldq, ldk, ldv, ldo, ld_do, ld_dq, ld_dk, ld_dv;           /* row strides (floats)  */
  int64_t stride_q, stride_k, stride_v, stride_o, stride_do, stride_dq, stride_dk, stride_dv;   /* batch strides */
  float scale;              /* 1/sqrt(d)                                                      */
  int32_t operand_precision;/* 0: exact fp32 products (v_mfma_f32_16x16x4_f32); 1: operands rounded to bf16 (RNE), fp32
                             * accumulation and softmax statistics (v_mfma_f32_16x16x32_bf16) - the autocast analogue */
  void* ws;                 /* bwd: caller-owned workspace of gad_attention_bwd_workspace_bytes(args) bytes (16-byte aligned)
                             * for the single-pass kernel's dQ partial slabs; NULL / too small: the dQ + dK/dV kernel pair runs */
  int64_t ws_bytes;
  int32_t flags;            /* GAD_ATTN_* */
} gad_attention_args;
#define GAD_ATTN_TWO_KERNEL_BWD 1   /* bwd: keep the recomputing dQ + dK/dV kernel pair (A/B tools, tests) */
#define GAD_ATTN_NARROW_FWD 2       /* fwd: keep the 4-wave kernel for d >= 160 instead of the 8-wave split-head-dim kernel (A/B) */
/* Bytes of `ws` the backward launch of these arguments uses if it is given them: the single-pass kernel's dQ slabs (key
 * blocks x B x Tq x heads x d floats; one key block writes dQ directly), 0 for every launch that runs the dQ + dK/dV pair -
 * d > 96, bf16 operands, few keys under many queries, GAD_ATTN_TWO_KERNEL_BWD - and for arguments gad_attention_bwd refuses.
 * Reads shapes, strides, flags and pointer alignment only (not ws / ws_bytes); the same route decision as the launch. */
int64_t gad_attention_bwd_workspace_bytes(const gad_attention_args* a);
int gad_attention_supported(int32_t d);      /* 1 if 1 <= d <= 256 */
int gad_attention_uses_bf16(const gad_attention_args* a, int32_t backward);   /* 1 if this launch multiplies bf16 operands */
int gad_attention_fwd(const gad_attention_args* a, void* stream);
int gad_attention_bwd(const gad_attention_args* a, void* stream);
/* Forward for one wide head, d = 512 (gad_attention_d512_supported): the mid-block attention of AutoencoderKL / VQModel
 * (gad/vae.py), one head over the whole channel count.  The contract of gad_attention_fwd's LDS-DMA launches - exact fp32,
 * online softmax, no score tensor in memory, any Tq and Tk >= 1, ld >= heads*d so q, k, v may be column blocks of one
 * [B*T][3C] projection, optional lse - with every ld and stride a multiple of 4 floats and every pointer 16-byte aligned;
 * anything else (another d, operand_precision != 0, a misaligned operand) is refused by name.  8 waves per workgroup of 64
 * queries, each with one half of the head dim; K and V stream in 16-key tiles (132 KB of LDS: one workgroup per CU). */
int gad_attention_d512_supported(int32_t d);   /* 1 if d == 512 */
int gad_attention_fwd_d512(const gad_attention_args* a, void* stream);
/* Causal self-attention forward for short sequences (gad_attention_causal_supported: 1 <= T <= 128, d in {16, 32, 64}): the
 * CLIP text towers (gad/text.py; T = 77, d = 64).  o = softmax(scale * q k^T + causal) v per (batch, head): query i sees keys
 * j <= i.  Tq == Tk == T; exact fp32 (v_mfma_f32_16x16x4_f32), every ld and stride a multiple of 4 floats and every pointer
 * 16-byte aligned, ld >= heads*d so q, k, v may be column blocks of one [B*T][3W] projection; lse optional, defined as for
 * gad_attention_fwd.  Anything else (Tq != Tk, T > 128, another d, operand_precision != 0, a misaligned operand) is refused by
 * name and launches nothing.  One workgroup per (b, h) stages K and V once in LDS (68 KB at most); key tiles above the
 * diagonal are skipped, the diagonal tile and the padded keys j >= T are masked before the row maximum, the softmax is one
 * pass.  A key's k and v rows never enter the arithmetic of an earlier query: a NaN at position t leaves rows < t as they were.
 * No score or mask tensor in memory, no atomics, bit-reproducible.  o must not overlap q, k or v. */
int gad_attention_causal_supported(int32_t T, int32_t d);
int gad_attention_causal_fwd(const gad_attention_args* a, void* stream);

/* ------------------------------------------------------------------------------
 * Row softmax (attention probabilities), in place allowed.
 *   fwd: p = softmax(scale * s) per row of length n
 *   bwd: ds = scale * p * (dp - sum(dp * p))
 * Replaces the softmax inside F.scaled_dot_product_attention
 * (src/diffusers/models/attention_processor.py:1321-1323).
 * ---------------------------------------------------------------------------- */
int gad_softmax_fwd(const float* s, float* p, int64_t rows, int32_t n, float scale, void* stream);
int gad_softmax_bwd(const float* p, const float* dp, float* ds, int64_t rows, int32_t n, float scale,
                    void* stream);

/* ------------------------------------------------------------------------------
 * Transformer-block pieces of UNet2DConditionModel (Stable Diffusion; BasicTransformerBlock in diffusers,
 * reached from text_to_image/train_text_to_image_lora.py:1268-1270): LayerNorm over the last dim and GEGLU
 * (out = h[:, :F] * gelu(h[:, F:]), exact erf GELU).  dgamma_dbeta is [2C]: dgamma then dbeta (NULL: not wanted).
 * ---------------------------------------------------------------------------- */
int64_t gad_layernorm_workspace_bytes(int64_t rows, int32_t C);
int gad_layernorm_fwd(const float* x, float* y, const float* gamma, const float* beta, float* mean, float* rstd,
                      int64_t rows, int32_t C, float eps, void* stream);
/* dx_add (may be NULL): [rows][C] added to dx in the store - the gradient of the residual branch that shares x with the
 * norm (BasicTransformerBlock: x = attn(norm(x)) + x), instead of a separate elementwise launch */
int gad_layernorm_bwd(const float* x, const float* dy, float* dx, const float* dx_add, const float* gamma, const float* mean,
                      const float* rstd, float* dgamma_dbeta, int64_t rows, int32_t C, void* ws, int64_t ws_bytes,
                      void* stream);
int gad_geglu_fwd(const float* h, float* out, int64_t M, int32_t F, void* stream);
int gad_geglu_bwd(const float* h, const float* dout, float* dh, int64_t M, int32_t F, void* stream);

/* ------------------------------------------------------------------------------
 * Elementwise / small kernels (HBM-bound)
 * ---------------------------------------------------------------------------- */
/* diffusers get_timestep_embedding: out[b][dim] fp32; t int64 [B] */
int gad_timestep_embedding(const int64_t* t, float* out, int32_t B, int32_t dim, int32_t flip_sin_to_cos,
                           float freq_shift, float max_period, void* stream);
/* y = x*sigmoid(x) ; dx = dy * s(1 + x(1-s)) */
int gad_silu_fwd(const float* x, float* y, int64_t n, void* stream);
int gad_silu_bwd(const float* x, const float* dy, float* dx, int64_t n, void* stream);
/* Rotated copies of the 3x3 conv weights that live in one flat parameter buffer, in ONE launch:
 *   dst[off + ((ci*3 + 2-r)*3 + 2-s)*Cout + co] = src[off + ((co*3 + r)*3 + s)*Cin + ci]
 * i.e. W'[ci][2-r][2-s][co] = W[co][r][s][ci]: with W' the data gradient of a 3x3 / stride-1 / pad-1 convolution IS the
 * forward convolution of dy (same kernels, same channel tiles).  table (device, int64[n_tiles][5]) = {off, Cout, Cin,
 * co0, ci0}, one row per 32 x 32 (co, ci) tile of every listed weight; src != dst.  Refreshed once per optimizer step. */
int gad_rotate_conv3x3(const float* src, float* dst, const int64_t* table, int32_t n_tiles, void* stream);
/* out[p][0:C1] = a[p][0:C1], out[p][C1:C1+C2] = b[p][0:C2]  (skip-connection concat, NHWC) */
int gad_concat_channels(const float* a, const float* b, float* out, int64_t pixels, int32_t C1, int32_t C2,
                        void* stream);
/* inverse of concat for the gradient: da = d[:, :C1], db = d[:, C1:] */
int gad_split_channels(const float* d, float* da, float* db, int64_t pixels, int32_t C1, int32_t C2,
                       void* stream);
/* NCHW <-> NHWC layout change */
int gad_nchw_to_nhwc(const float* x, float* y, int32_t B, int32_t C, int32_t HW, void* stream);
int gad_nhwc_to_nchw(const float* x, float* y, int32_t B, int32_t C, int32_t HW, void* stream);
/* dx[b][h][w][c] = sum of the 2x2 block of dy[b][2h..2h+1][2w..2w+1][c] (nearest-upsample backward) */
int gad_upsample2x_bwd(const float* dy, float* dx, int32_t B, int32_t H, int32_t W, int32_t C, void* stream);
/* out[s][n] = sum_m dy[s][m][n] for S segments of M rows (S=1: bias gradient; S=B, M=H*W: gradient of the
 * per-image time-embedding add) */
int gad_colsum(const float* dy, float* out, int32_t S, int64_t M, int32_t N, void* ws, int64_t ws_bytes,
               void* stream);

/* DDPMScheduler.add_noise (main.py:698): xt = sqrt(ac[t_b]) x0 + sqrt(1-ac[t_b]) eps ; per_sample = C*H*W */
int gad_add_noise(const float* x0, const float* eps, const int64_t* t, const float* alphas_cumprod,
                  float* xt, int32_t B, int64_t per_sample, void* stream);
/* DDIMScheduler.step, eta = 0 (src/diffusion_utils.py:336-341 via DDPMPipeline):
 *   x0 = (x - sqrt(1-a_t) e)/sqrt(a_t); clamp(+-clip) if clip>0; x' = sqrt(a_p) x0 + sqrt(1-a_p) e      */
int gad_ddim_step(const float* x, const float* eps, float* x_prev, int64_t n, float alpha_t,
                  float alpha_prev, float clip, void* stream);
/* classifier-free-guidance DDIM step (StableDiffusionPipeline loop driven at
 * text_to_image/compute_model_behaviors.py:311-326): eps = eps_u + guidance*(eps_c - eps_u), then the DDIM update.
 * eps_uc holds the U-Net output of the doubled batch: [uncond ; cond], each n floats. */
int gad_cfg_ddim_step(const float* x, const float* eps_uc, float* x_prev, int64_t n, float guidance, float alpha_t,
                      float alpha_prev, float clip, void* stream);
/* final pipeline post-processing: y = clamp(x/2 + 0.5, 0, 1) */
int gad_to_image01(const float* x, float* y, int64_t n, void* stream);
/* MSE loss and its gradient in one pass: loss[0] = mean((a-b)^2) ; d = 2 (a-b) * gscale / n */
int gad_mse_fwd_bwd(const float* a, const float* b, float* loss, float* d, int64_t n, float gscale,
                    void* ws, int64_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------
 * Fused optimizer over the flat parameter buffer
 * (clip_grad_norm_ main.py:718 + Adam/AdamW :557-561,719 + EMAModel.step :725).
 *   gad_sumsq: out[0] = sum(g^2)   (deterministic two-stage reduction)
 *   gad_clip_adam_ema: coef = min(1, max_norm/(sqrt(sumsq[0])+1e-6)); g*=coef;
 *     Adam(W) update with bias correction for `step`; ema -= (1-ema_decay)(ema-p) if ema != NULL
 * ---------------------------------------------------------------------------- */
int gad_sumsq(const float* g, float* out, int64_t n, void* ws, int64_t ws_bytes, void* stream);
typedef struct gad_adam_args {
  float* p; const float* g; float* m; float* v; float* ema;
  int64_t n;
  const float* sumsq;       /* device scalar from gad_sumsq, or NULL for no clipping          */
  float max_norm;
  float lr, beta1, beta2, eps, weight_decay;   /* weight_decay is decoupled (AdamW) if adamw  */
  int32_t adamw;
  int32_t step;             /* 1-based                                                        */
  float ema_decay;
} gad_adam_args;
int gad_clip_adam_ema(const gad_adam_args* a, void* stream);
/* standalone EMAModel.step (diffusers training_utils; main.py:725): ema -= (1-decay) * (ema - p) */
int gad_ema_update(float* ema, const float* p, int64_t n, float decay, void* stream);

/* ------------------------------------------------------------------------------
 * 8-bit blockwise Adam over the flat parameter buffer (csrc/optim8.hip): bitsandbytes' Adam8bit / AdamW8bit
 * (main.py:562-588, unlearn.py:429-477, train_text_to_image_lora.py:884-892) restated - blocks of 2048 elements, parameters
 * below 4096 elements keep fp32 moments, no percentile clipping - fused with the clip and the EMA like gad_clip_adam_ema.
 *   gad_adam8_qmap: the 256 ascending fp32 code values of the signed (first moment; zero at index 127) or unsigned (second
 *     moment; zero at index 0) dynamic map, into a HOST array; needs no GPU.  The kernel's tables are the same constants.
 *   gad_adam8_block: one run of at most 2048 elements of ONE parameter.  Blocks never cross a parameter and never cover the
 *     padding between parameters.  `state` is the block's index into absmax1 / absmax2, or with `fp32` set the offset of its
 *     moments in m32 / v32 (a multiple of 4).  `offset` is a multiple of 8.
 *   gad_clip_adam8_ema, per element, in fp32: g *= coef (as gad_clip_adam_ema) ; m = qmap1[c1]*absmax1[b], v = qmap2[c2]*absmax2[b] ;
 *     m = m*beta1 + (1-beta1) g ; v = v*beta2 + (1-beta2) g g ; p -= (lr sqrt(1-beta2^t)/(1-beta1^t)) m / (sqrt(v) + eps sqrt(1-beta2^t)) ;
 *     p *= 1 - lr*weight_decay if the block's weight_decay > 0 ; EMA as gad_clip_adam_ema ; absmax1[b] = max|m|, absmax2[b] = max v ;
 *     codes = nearest map value of m/absmax1, v/absmax2 (lower index on a tie; a negative m never takes the zero code: 126);
 *     a block whose absmax is 0 stores the zero code.  A descriptor that points outside n / n32 / n_absmax is skipped.
 * ---------------------------------------------------------------------------- */
int gad_adam8_qmap(int is_signed, float* out256);
typedef struct gad_adam8_block {
  int64_t offset;           /* first element in the flat buffer                                 */
  int32_t len;              /* 1..2048                                                          */
  int32_t state;            /* absmax index, or offset into m32 / v32 if fp32                   */
  float weight_decay;       /* decoupled, applied after the update; 0 = none                    */
  int32_t fp32;             /* 1: the parameter keeps fp32 moments (fewer than 4096 elements)   */
} gad_adam8_block;
typedef struct gad_adam8_args {
  float* p; const float* g; float* ema;       /* flat buffers of n floats; ema may be NULL      */
  uint8_t* state1; uint8_t* state2;           /* n code bytes each, laid out like p             */
  float* absmax1; float* absmax2;             /* n_absmax floats each                           */
  float* m32; float* v32;                     /* n32 floats each: moments of the small parameters */
  const gad_adam8_block* blocks;              /* DEVICE table of n_blocks descriptors           */
  int64_t n, n32;
  int32_t n_absmax, n_blocks;
  const float* sumsq;       /* device scalar from gad_sumsq, or NULL for no clipping            */
  float max_norm;
  float lr, beta1, beta2, eps;
  int32_t step;             /* 1-based                                                          */
  float ema_decay;
} gad_adam8_args;
int gad_clip_adam8_ema(const gad_adam8_args* a, void* stream);


/* ==============================================================================
 * Half-precision activation path ("--mixed_precision fp16|bf16" of the reference's Stable-Diffusion jobs:
 * text_to_image/experiments/setup_train_commands.py:127,142,165, setup_unlearn_commands.py:166; frozen weights cast to the
 * 16-bit type and autocast around the U-Net, text_to_image/train_text_to_image_lora.py:752-760,1268-1270).  bf16 is the
 * MI355X-native 16-bit type (fp32's exponent range: no loss scaling).  On this path ACTIVATIONS AND THEIR GRADIENTS LIVE IN
 * HBM AS bf16 (NHWC / [rows][C]); frozen weights are bf16 copies made once; LoRA A / B, their gradients and the optimizer
 * state stay fp32 (train_text_to_image_lora.py:777: "LoRA weights in fp32") with a bf16 shadow refreshed per step;
 * accumulation, normalisation statistics, softmax statistics and every epilogue are fp32.
 * All `void*` activation pointers below are bf16 (uint16 storage) unless a field says fp32.
 * ============================================================================== */
/* hgemm: C[m][n] = epilogue( alpha * sum_k A(m, k) * B[n][k] )   - v_mfma_f32_32x32x16_bf16, operands streamed by LDS-DMA.
 * B is always [n][k] with k contiguous (torch Linear / [Cout][KH][KW][Cin] conv storage; data gradients use transposed /
 * rotated bf16 copies of the frozen weights, made once).  A is
 *   conv == 0: dense A[m][k], row stride lda;
 *   conv == 1: the im2col gather of an NHWC tensor: m = (img, oy, ox), k = (r, s, c): pixel (oy*stride - pad_t + r,
 *              ox*stride - pad_l + s) of image img (>> 1 each if upsample: nearest-2x fused), zero outside;
 *   conv == 2: the gather of a stride-2 convolution's data gradient: m = (img, y, x) on the INPUT grid, k = (r, s, co) with
 *              the ROTATED weight: pixel ((y - pad_t + r) / 2, (x - pad_l + s) / 2) of dy where both are even, else zero.
 * The contraction axis may continue in a second operand pair: dense: k >= k_split reads A2[m][k - k_split] (row stride lda2)
 * and B2[n][k - k_split] (ldb2) - the fused LoRA linear (y = x W^T + mid up^T; dx = dy W + dmid down) -; conv: channels
 * c >= k_split of every tap come from A2 (pixel stride lda2) - UpBlock2D's torch.cat without the copy - while B stays one
 * [N][taps * C] matrix.  Every segment length and k_split must be a multiple of 8.
 * Epilogue (fp32): + bias[n] + rowadd[m / rows_per_group][n] (time-embedding add) + residual[m][n] (bf16), stored as bf16
 * (out_f32 == 0) or fp32 (out_f32 == 1; accumulate != 0 adds to what C holds: parameter-gradient slots).
 * ws: gad_hgemm_workspace_bytes(args) bytes for split-K partials (fp32 slabs reduced in a fixed order by a second launch).
 * Replaces cuDNN / cuBLAS half-precision kernels under the autocast U-Net (train_text_to_image_lora.py:1268-1270). */
typedef struct gad_hgemm_args {
  const void* A; const void* A2; const void* B; const void* B2;
  void* C;
  int32_t M, N, K;          /* K = total contraction length (conv: KH*KW*Cin)                                   */
  int32_t lda, lda2, ldb, ldb2, ldc;
  int32_t k_split;          /* dense: first segment's length (== K: single segment); conv: channels of source 1 */
  int32_t conv;             /* 0 / 1 / 2 as above                                                               */
  int32_t H, W, Cin;        /* gathered tensor (stored size), total channels                                    */
  int32_t Ho, Wo, KH, KW, stride, pad_t, pad_l, upsample;   /* Ho x Wo: the GEMM rows' pixel grid             */
  float alpha;
  const float* bias;        /* fp32 [N] or NULL                                                                 */
  const float* rowadd;      /* fp32 [M / rows_per_group][ld_rowadd] or NULL                                     */
  int32_t rows_per_group, ld_rowadd;
  const void* residual;     /* bf16 [M][ldr] or NULL                                                            */
  int32_t ldr;
  int32_t out_f32, accumulate;
  void* ws; int64_t ws_bytes;
  int32_t tile_hint;        /* 0 auto; 1 / 9 / 8: 128 x 128 (32x32x16 / 16x16x32 MFMAs / 32-deep steps); 2 / 7: 128 x 320; 5 / 6: 256 x 320, eight waves */
  int32_t splitk_hint;      /* 0 auto; > 0 force                                                                */
} gad_hgemm_args;
int64_t gad_hgemm_workspace_bytes(const gad_hgemm_args* a);
int gad_hgemm_plan(const gad_hgemm_args* a, int32_t* tile, int32_t* splitk);   /* tile: as tile_hint */
int gad_hgemm(const gad_hgemm_args* a, void* stream);
/* The token-axis contraction of the LoRA parameter gradients (dB = dy^T mid, dA = dmid^T x, G = dy^T x:
 * train_text_to_image_lora.py:1305 loss.backward() through LoRALinearLayer): C[m][n] = alpha * sum_k A[k][m] B[k][n], BOTH operands
 * stored with the contraction index k (the token) as their row - A: K rows of lda >= M, B: K rows of ldb >= N - so the activations
 * are read in place (transposing LDS reads), no transposed copies.  fp32 output only (out_f32 = 1; accumulate as in gad_hgemm);
 * lda, ldb multiples of 8 and >= M, N rounded up to 8 (rows are read in 16-byte chunks; columns >= M / N feed no output); of gad_hgemm_args only A, B, C, M, N, K, lda, ldb, ldc, alpha, accumulate, ws, splitk_hint are read. */
int64_t gad_hgemm_tn_workspace_bytes(const gad_hgemm_args* a);
int gad_hgemm_tn(const gad_hgemm_args* a, void* stream);
/* Segmented form of gad_hgemm_tn (per-sample LoRA gradients from one backward: the token axis of a batch is the concatenation of
 * the samples' tokens):  C_s[m][n] (+)= alpha * sum_{k = s L .. (s + 1) L - 1} A[k][m] B[k][n],  s = 0 .. S - 1,  C_s = C + s * c_seg_stride.
 * A, B bf16 [S * L][lda / ldb] read in place (alignment rules of gad_hgemm_tn); L is any positive length; C fp32, c_seg_stride in floats,
 * independent of ldc and >= (M - 1) * ldc + N.  One launch covers all segments (+ one reduce launch when a segment is split along its
 * rows).  The split depends on (M, N, L) only and the slabs are summed in slab order: a segment's result is bit-identical whatever S is
 * and wherever the segment sits, and equals gad_hgemm_tn with K = L and the same split.  Arguments are checked before any HIP call. */
typedef struct gad_hgemm_seg_args {
  const void* A;            /* bf16 [S * L][lda]: column m of row k is A[k][m]                 */
  const void* B;            /* bf16 [S * L][ldb]                                                */
  float* C;                 /* segment 0's [M][ldc] fp32 output                                 */
  void* ws;                 /* split workspace (caller owned)                                   */
  int64_t ws_bytes;
  int64_t c_seg_stride;     /* floats between the outputs of consecutive segments               */
  int32_t M, N;             /* output rows / columns                                            */
  int32_t L, S;             /* rows per segment, segments                                       */
  int32_t lda, ldb, ldc;    /* row strides in elements                                          */
  float alpha;
  int32_t accumulate;       /* 1: C_s += result, 0: C_s = result                                */
  int32_t splitk_hint;      /* 0 auto; > 0 force that many row slices per segment               */
} gad_hgemm_seg_args;
/* bytes of workspace gad_hgemm_tn_seg needs (-1 and gad_last_error() if the arguments are refused; ws / ws_bytes are not looked at) */
int64_t gad_hgemm_tn_seg_workspace_bytes(const gad_hgemm_seg_args* a);
int gad_hgemm_tn_seg(const gad_hgemm_seg_args* a, void* stream);
/* dst[c][r] = bf16(src[r][c]) for `batch` matrices (strides in elements); src fp32 (src_f32 != 0) or bf16; the operand
 * transposes of the LoRA parameter gradients (dUp = dy^T mid, dDown = dmid^T x) and of the per-step bf16 shadows of the
 * LoRA matrices' transposes */
int gad_h_transpose(const void* src, void* dst, int32_t rows, int32_t cols, int32_t ld_src, int32_t ld_dst, int32_t src_f32,
                    void* stream);
/* bf16 shadows of the 2-D matrices resident in a flat fp32 parameter buffer (the LoRA matrices of training.flatten_params), ONE launch
 * per optimizer step: dst[off + r*cols + c] = dst_t[off + c*rows + r] = bf16(src[off + r*cols + c]).  table (device, int64[n_tiles][5]) =
 * {off, rows, cols, r0, c0}: one 64 x 64 tile of one matrix per row.  The copies feed the forward products, the transposes the data
 * gradients (text_to_image/train_text_to_image_lora.py:1305 loss.backward() through LoRALinearLayer). */
int gad_h_shadow_pairs(const float* src, void* dst, void* dst_t, const int64_t* table, int32_t n_tiles, void* stream);
/* dst = bf16(src) (to_f32 == 0: src fp32) or dst = fp32(src) (to_f32 != 0: src bf16) */
int gad_h_cast(const void* src, void* dst, int64_t n, int32_t to_f32, void* stream);
/* GroupNorm (+ SiLU) with bf16 x / y / dy / dx, fp32 gamma / beta / mean / rstd: the fields of gad_groupnorm_args read as
 * bf16 where they are activations.  Forward reads two sources (x2 / C1) in place; backward computes dx only (frozen norm:
 * dgamma / dbeta must be NULL) and adds dx_add (bf16) in its store.  ws: gad_h_groupnorm_workspace_bytes(). */
int64_t gad_h_groupnorm_workspace_bytes(const gad_groupnorm_args* a);
int gad_h_groupnorm_silu_fwd(const gad_groupnorm_args* a, void* stream);
int gad_h_groupnorm_silu_bwd(const gad_groupnorm_args* a, void* stream);
/* LayerNorm over the last dim, bf16 x / y / dy / dx / dx_add, fp32 gamma / beta / mean / rstd; backward: dx only */
int gad_h_layernorm_fwd(const void* x, void* y, const float* gamma, const float* beta, float* mean, float* rstd, int64_t rows,
                        int32_t C, float eps, void* stream);
int gad_h_layernorm_bwd(const void* x, const void* dy, void* dx, const void* dx_add, const float* gamma, const float* mean,
                        const float* rstd, int64_t rows, int32_t C, void* stream);
/* GEGLU on bf16: out = h[:, :F] * gelu(h[:, F:]) and its backward */
int gad_h_geglu_fwd(const void* h, void* out, int64_t M, int32_t F, void* stream);
int gad_h_geglu_bwd(const void* h, const void* dout, void* dh, int64_t M, int32_t F, void* stream);
/* dx[b][h][w][c] = sum of the 2 x 2 block of dy (bf16 in / out, fp32 sum) */
int gad_h_upsample2x_bwd(const void* dy, void* dx, int32_t B, int32_t H, int32_t W, int32_t C, void* stream);
/* out = a + b (bf16, fp32 sum): skip-connection gradient sums the autograd engine would otherwise run as at::add */
int gad_h_add(const void* a, const void* b, void* out, int64_t n, void* stream);
/* Fused attention with bf16 q / k / v / o / d_o / dq / dk / dv (fp32 lse / delta): the fields of gad_attention_args read as
 * bf16, strides in elements; head dims that are multiples of 8 up to 160.  Same kernels as operand_precision = 1 of
 * gad_attention_fwd / _bwd with 16-bit tile loads and stores. */
int gad_h_attention_fwd(const gad_attention_args* a, void* stream);
int gad_h_attention_bwd(const gad_attention_args* a, void* stream);

/* ------------------------------------------------------------------------------
 * Johnson-Lindenstrauss random projection of gradients (TRAK / D-TRAK features).
 * Replaces trak.projectors.CudaProjector (fast_jl, CUDA only) under
 *   src/attributions/methods/d_trak_grad.py:411-418,654.
 *   out[g][j] = (accumulate ? out[g][j] : 0) + sum_{p<P} A[g*lda + p] * R(p0 + p, j)   g < G, j < d
 * R is never stored: R(row, j) is a pure function of (seed, model_id, row, j, type) through
 * Philox-4x32-10 (Random123 constants) with key (seed, model_id) and counter
 * (column block, row low 32 bits, row high 32 bits, type):
 *   GAD_JL_NORMAL      one call -> columns 4c..4c+3 of a row; words x -> u = fl32(fl32(x) * 2^-32 + 2^-33),
 *                      Box-Muller on (u0,u1), (u2,u3): r = sqrt(-2 ln u_even), z_even = r cos(2 pi u_odd), z_odd = r sin(..)
 *   GAD_JL_RADEMACHER  one call -> columns 128c..128c+127; entry j is +1 / -1 for bit (j mod 32) of word
 *                      (j mod 128) / 32 clear / set
 * Unit-variance entries, no 1/sqrt(d) scale.  Contraction on v_mfma_f32_16x16x4_f32 (exact fp32), split along P over a
 * plan that depends on (P, d) only and reduced slab by slab in a fixed order: bit-reproducible, and a row's output does
 * not depend on G or on the other rows.  A 16-B aligned with lda a multiple of 4 and >= P; d a multiple of 64; out and
 * workspace 16-B aligned, workspace_bytes >= gad_jl_project_workspace_bytes(args).
 * ---------------------------------------------------------------------------- */
enum gad_jl_type { GAD_JL_NORMAL = 0, GAD_JL_RADEMACHER = 1 };

typedef struct gad_jl_args {
  const float* A;           /* [G][lda] fp32 rows to project                                  */
  int64_t lda;              /* row stride of A in floats                                      */
  int32_t G;                /* rows of A / out                                                */
  int64_t P;                /* contracted length                                              */
  int64_t p0;               /* R row of A's column 0 (projection of a chunk of a longer row) */
  int32_t d;                /* projected dimension (columns of R and out)                     */
  uint32_t seed, model_id;  /* Philox key                                                     */
  int32_t type;             /* enum gad_jl_type                                               */
  int32_t accumulate;       /* 1: out += A R, 0: out = A R                                     */
  float* out;               /* [G][d] fp32                                                    */
  void* workspace;          /* per-slab partials (caller owned)                               */
  int64_t workspace_bytes;
} gad_jl_args;

/* bytes of workspace gad_jl_project needs for these arguments (-1 and gad_last_error() if they are refused) */
int64_t gad_jl_project_workspace_bytes(const gad_jl_args* a);
int gad_jl_project(const gad_jl_args* a, void* stream);

/* ------------------------------------------------------------------------------
 * Ancestral DDPM update with in-kernel variance noise (csrc/sampler.hip): the scheduler.step of the Journey-TRAK
 * trajectory generator (reference src/attributions/methods/d_trak_grad.py:472-479, diffusers DDPMScheduler.step with
 * epsilon prediction).  x, eps, x_prev: B rows of n contiguous floats.  Per element, with cur_alpha = alpha_t / alpha_prev:
 *   x0     = (x - sqrt(1 - alpha_t) eps) / sqrt(alpha_t), clamped to +-clip when clip > 0
 *   mean   = sqrt(alpha_prev) (1 - cur_alpha) / (1 - alpha_t) x0 + sqrt(cur_alpha) (1 - alpha_prev) / (1 - alpha_t) x
 *   x_prev = mean + sqrt(var) z   for t > 0      GAD_DDPM_FIXED_SMALL  var = max((1 - alpha_prev) / (1 - alpha_t) (1 - cur_alpha), 1e-20)
 *                                                GAD_DDPM_FIXED_LARGE  var = 1 - cur_alpha
 *   x_prev = mean                 for t == 0     (Philox is not called, seeds is not read)
 * The coefficients are formed in fp64 on the host from the two fp32 alphas and rounded once to fp32.
 * z is never stored: element e of row b takes word e & 3 of one Philox-4x32-10 call (Random123 constants) with
 *   key     (seeds[b] low 32 bits, seeds[b] high 32 bits)
 *   counter (e >> 2, t, 0, 2)
 * through the projector's maps: words x -> u = fl32(fl32(x) * 2^-32 + 2^-33), Box-Muller on (u0,u1), (u2,u3) in the order
 * r01 cos, r01 sin, r23 cos, r23 sin with r = sqrt(-2 ln u_even) and angle 2 pi u_odd.  A row's result is a function of
 * (seeds[b], t, the row's own x and eps) alone: it does not depend on B, on the row's position or on the launch grid, and a
 * repeated launch gives equal bits.  x and eps are read once and x_prev written once (12 B per element); no workspace, no
 * atomics; x_prev == x (in place) is allowed.  Refused with a named error before any HIP call: a null pointer, a base that
 * is not 16-byte aligned (seeds: 8-byte), n % 4 != 0, n / 4 > 2^32, B <= 0, t < 0, an alpha outside (0, 1],
 * alpha_prev < alpha_t, clip < 0, an unknown variance_type.
 * ---------------------------------------------------------------------------- */
enum gad_ddpm_variance { GAD_DDPM_FIXED_SMALL = 0, GAD_DDPM_FIXED_LARGE = 1 };
int gad_ddpm_step(const float* x, const float* eps, float* x_prev, int32_t B, int64_t n, const int64_t* seeds, int32_t t,
                  float alpha_t, float alpha_prev, float clip, int32_t variance_type, void* stream);

/* ------------------------------------------------------------------------------
 * One PLMS step of the PNDM sampler (csrc/sampler.hip; diffusers PNDMScheduler.step_plms with skip_prk_steps, epsilon
 * prediction - what the reference's StableDiffusionPipeline runs, text_to_image/compute_model_behaviors.py:311-326).
 * Every operand is n contiguous floats.  Per element:
 *   e      = eps_u + guidance (eps_c - eps_u)     (eps_c == NULL: e = eps_u, guidance is not read)
 *   m      = w0 e + w1 h1 + w2 h2 + w3 h3         (h1 the newest stored prediction; a NULL h_i is not read)
 *   x_prev = cs xs - cm m                         (xs = x; GAD_PLMS_USE_SAVED: xs = x_saved and x is not read)
 *   push[i]    = e                                (push != NULL: the history slot that receives this prediction)
 *   x_saved[i] = x                                (GAD_PLMS_SAVE: the first step remembers its sample for the second)
 * with, for abar_t = alphas_cumprod[t_from] and abar_p = alphas_cumprod[t_to] (gad.schedulers.plms_coefficients),
 *   cs = sqrt(abar_p / abar_t),  cm = (abar_p - abar_t) / (abar_t sqrt(1 - abar_p) + sqrt(abar_t (1 - abar_t) abar_p)).
 * The caller forms cs, cm and the weights in fp64; each is rounded once to fp32 here.  With weights (1, 0, 0, 0) the update
 * is the DDIM eta = 0 step of gad_ddim_step without clipping.  A lane reads all operands of its float4 before it writes, so
 * x_prev == x (in place) is allowed and push may be one of h1..h3 (a three-slot ring overwrites the slot it read as h3); the
 * history terms are a prefix (h2 needs h1, h3 needs h2) and the kernel is instantiated on their number and on guidance, so
 * an absent operand costs no load: at most 24 B read and 8 B written per element.  No workspace, no atomics, a repeated
 * launch gives equal bits.  Refused with a named error before any HIP call: a null x, eps_u or x_prev; a null x_saved under
 * GAD_PLMS_SAVE / GAD_PLMS_USE_SAVED; an unknown saved_mode; a base that is not 16-byte aligned; n < 4 or n % 4 != 0; a gap in
 * the history terms; a non-zero weight for a null h_i; a coefficient that is not finite (in fp64 or after rounding) or
 * cs <= 0; a guidance that is not finite; x_prev equal to eps or a history slot; push or x_saved equal to x, x_prev, eps or
 * each other.
 * ---------------------------------------------------------------------------- */
enum gad_plms_saved { GAD_PLMS_SAVED_NONE = 0, GAD_PLMS_SAVE = 1, GAD_PLMS_USE_SAVED = 2 };
int gad_plms_step(const float* x, const float* eps_u, const float* eps_c, float guidance, const float* h1, const float* h2,
                  const float* h3, float* push, float* x_saved, int32_t saved_mode, float* x_prev, int64_t n, double cs,
                  double cm, double w0, double w1, double w2, double w3, void* stream);

/* ------------------------------------------------------------------------------
 * The x0 rows of one Stable-Diffusion training step drawn from cached VAE posterior moments (csrc/latent.hip; reference
 * text_to_image/train_text_to_image_lora.py:1065-1077 RandomHorizontalFlip, :1220-1223
 * vae.encode(x).latent_dist.sample() * scaling_factor).  The posterior of an image is a function of (image, mirrored or
 * not), so both are encoded once and kept:
 *   moments : fp32 [N][F][2][n]   F = 1 (plain encode) or 2 (plain | encode of the mirrored image); per slab mean[n], logvar[n]
 *   rows    : int64 [B], device   the dataset row of every batch row, clamped to [0, N) in the kernel
 *   x0      : fp32 [B][n]         flipped : uint8 [B] or NULL - which slab row b was read from
 * For batch row b with r = rows[b] and element e, with Philox-4x32-10 (Random123 constants), key (seed low 32 bits, high 32 bits):
 *   coin = bit 0 of word 0 of the block with counter (0xFFFFFFFF, r, step, 3)
 *   f    = coin if GAD_LATENT_RANDOM_FLIP is set (needs F == 2), else 0;   m, lv = mean, logvar of slab (r, f) at e
 *   x0   = scale * m                                             flags without GAD_LATENT_SAMPLE: latent_dist.mode(); Philox is
 *                                                                not called for noise and logvar is not read
 *   x0   = scale * (m + expf(0.5f * clamp(lv, -30, 20)) * z)     GAD_LATENT_SAMPLE: z is word e & 3 of the block with
 *                                                                counter (e >> 2, r, step, 3)
 * through the projector's maps: words x -> u = fl32(fl32(x) * 2^-32 + 2^-33), Box-Muller on (u0,u1), (u2,u3) in the order
 * r01 cos, r01 sin, r23 cos, r23 sin.  Counter word 3 is this kernel's tag (gad_jl_project uses 0 and 1, gad_ddpm_step 2).
 * A row's result is a function of (seed, r, step) and the moments alone: it does not depend on B, on the row's position or on
 * the launch grid, a row repeated in `rows` gives equal rows, and a repeated launch gives equal bits.  12 B of traffic per
 * element, no workspace, no atomics.  Refused with a named error before any HIP call: a null moments, rows or x0; a base that
 * is not 16-byte aligned (rows: 8-byte); n % 4 != 0; n / 4 >= 2^32 - 1 (the coin's block index must not be reachable);
 * N < 1 or N >= 2^32; F outside {1, 2}; GAD_LATENT_RANDOM_FLIP with F == 1; an unknown flag; B < 1.
 * ---------------------------------------------------------------------------- */
enum gad_latent_flags { GAD_LATENT_SAMPLE = 1, GAD_LATENT_RANDOM_FLIP = 2 };
int gad_latent_draw(const float* moments, int64_t N, int32_t F, int64_t n, const int64_t* rows, int32_t B, float* x0,
                    uint8_t* flipped, int64_t seed, uint32_t step, float scale, int32_t flags, void* stream);

/* uint8 [B][H][W][C] -> fp32 [B][C][H][W] through a 256-entry device table: dst[b][c][h][w] = lut[src[b][h][w'][c]] with
 * w' = W - 1 - w when flip == 1, else w.  The caller fills the table as gad_cosine_rows' callers fill theirs, in the two fp32
 * steps u / 255 and (x - 0.5) / 0.5 (ToTensor + Normalize([0.5], [0.5])): the images stay on the device as bytes and the
 * encoder is fed both orientations without a host round trip.  Any B, H, W, C >= 1; a lane writes one float4 of four
 * consecutive w when W % 4 == 0 and one float otherwise.  dst 16-byte aligned, lut 4-byte; null pointers, flip outside
 * {0, 1} and sizes whose product overflows are refused by name before any HIP call. */
int gad_pixels_to_nchw(const uint8_t* src, float* dst, int64_t B, int32_t H, int32_t W, int32_t C, const float* lut,
                       int32_t flip, void* stream);

/* ------------------------------------------------------------------------------
 * Local model behaviours of the unconditional models (csrc/local.hip; reference
 * unconditional_generation/unlearn.py:871-948, calculate_local_scores.py:303-374).
 * All three are order-deterministic (no atomics): a result depends on its own image / segment and on the
 * geometry only, not on the batch size or the position in the batch.
 *
 * gad_image_metrics: N image pairs -> out[N][3] = (mse, nrmse, ssim) as fp64, with scikit-image's definitions for
 *   mean_squared_error(a, b), normalized_root_mse(image_true = a, image_test = b) (euclidean normalisation) and
 *   structural_similarity(a, b, channel_axis = -1, data_range): uniform win x win window, sample covariance, the map
 *   cropped by (win - 1) / 2 on every side, mean over pixels and channels.  a, b: [N][H][W][C] fp32; win odd, 3..11;
 *   H, W >= win.  Pixels are converted to fp64 before any product or difference; sums, the SSIM map and the means are fp64.
 *   out and workspace 8-B aligned, workspace_bytes >= gad_image_metrics_workspace_bytes(...) (-1: arguments refused).
 * gad_add_noise_bcast: row r of R belongs to image r / rows_per_image and timestep t[r % T]:
 *   xt[r] = sqrt(ac[t]) x0[image] + sqrt(1 - ac[t]) eps[r];  x0 [R / rows_per_image][C][HW] and eps [R][C][HW] are NCHW,
 *   xt [R][HW][C] is NHWC (the U-Net's input layout).  T divides rows_per_image, rows_per_image divides R;
 *   alphas_cumprod has num_train_timesteps entries (a t outside the table yields NaN rows, no read).
 * gad_mse_segments: out[s] = mean over rows s * rows_per_segment .. of (pred - eps)^2, pred [R][HW][C] NHWC, eps [R][C][HW]
 *   NCHW; fp64 row sums, one fixed-order sum per segment, one rounding to fp32.  workspace 8-B aligned,
 *   workspace_bytes >= gad_mse_segments_workspace_bytes(...).
 * ---------------------------------------------------------------------------- */
int64_t gad_image_metrics_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t C, int32_t win);
int gad_image_metrics(const float* a, const float* b, double* out, int32_t N, int32_t H, int32_t W, int32_t C,
                      int32_t win, double data_range, double K1, double K2, void* workspace, int64_t workspace_bytes,
                      void* stream);
int gad_add_noise_bcast(const float* x0, const float* eps, const int64_t* t, const float* alphas_cumprod, float* xt,
                        int32_t R, int32_t rows_per_image, int32_t T, int32_t C, int32_t HW, int32_t num_train_timesteps,
                        void* stream);
int64_t gad_mse_segments_workspace_bytes(int32_t R, int32_t rows_per_segment, int32_t C, int32_t HW);
int gad_mse_segments(const float* pred, const float* eps, float* out, int32_t R, int32_t rows_per_segment, int32_t C,
                     int32_t HW, void* workspace, int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------
 * WoodFisher recursion of influence unlearning (csrc/influence.hip; reference src/unlearn/Wfisher.py:200-205,
 * Singh & Alistarh eq. 2) over three parameter-sized fp32 vectors.  One iteration for a batch gradient g:
 *   tmp = o.g   kg = k.g      k -= kg / (N + tmp) * o  (the OLD o)      o -= tmp / (N + tmp) * o
 * Both calls are asynchronous on `stream`, allocate nothing and can be captured into a hipGraph; the coefficients never
 * visit the host.  28 B per parameter per iteration (3 + 2 reads, 2 writes).
 * gad_wf_dots: dots[0] = o.g, dots[1] = k.g.  Every product is formed and accumulated in fp64 (an fp32 x fp32 product is
 *   exact there, so the only rounding is the fp64 summation).  One sweep, a float4 per lane, grid-stride over at most 2048
 *   workgroups of 256, scalar tail for n % 4; wave, then LDS, then one fp64 pair per workgroup in ws; a single-workgroup
 *   pass sums the pairs in index order.  No atomics: bit-reproducible, a function of (o, k, g, n) alone.
 *   ws_bytes >= gad_wf_dots_workspace_bytes(n) (-1 and gad_last_error() if n <= 0), the function the launch sizes its grid by.
 * gad_wf_update: every thread forms c_k = dots[1] / (N + dots[0]) and c_o = dots[0] / (N + dots[0]) in fp64, rounds each once
 *   to fp32, then per element k = fmaf(-c_k, o, k) and o = fmaf(-c_o, o, o), both with the old o.  N + dots[0] == 0 follows
 *   IEEE arithmetic, as in the reference.
 * o, k, g 16-byte aligned; dots (two doubles) and ws 8-byte aligned; n > 0.  Arguments are checked before any HIP call.
 * ---------------------------------------------------------------------------- */
int64_t gad_wf_dots_workspace_bytes(int64_t n);
int gad_wf_dots(const float* o, const float* k, const float* g, int64_t n, double* dots, void* ws, int64_t ws_bytes, void* stream);
int gad_wf_update(float* o, float* k, const double* dots, double N, int64_t n, void* stream);

/* ------------------------------------------------------------------------------
 * LoRA unlearning of the unconditional U-Nets (csrc/lora.hip; reference unconditional_generation/unlearn.py:404-424 through
 * peft's LoRA layer, y = base(x) + B(A(dropout(x))) * alpha / r).  Up to four projections share the tokens x (an attention
 * block's to_q / to_k / to_v, each with its own dropout mask):
 *   gad_lora_down_dropout_fwd   mid_j [M][r] = scale * ( x o m_j / (1 - p) ) A_j^T                j < n_proj
 *   gad_lora_down_dropout_bwd   dA_j  [r][C] = dmid_j^T ( x o m_j / (1 - p) )                      (overwritten)
 *                               dx    [M][ld_dx] += sum_j ( dmid_j A_j ) o m_j / (1 - p)           (accumulated in place)
 * mid_j feed the K-concatenated gad_gemm launch (A_k2 = mid_j, B_k2 = B_j); dmid_j = scale * dy_j B_j comes from gad_gemm.
 * The keep mask m_j is never stored: m_j(m, c) is Philox-4x32-10 (Random123 constants) with key (seed, offset) and counter
 * (c >> 2, m low 32 bits, m high 32 bits, (layer << 2) | j); channel c takes word c & 3 of the result and is kept when
 * word >= floor(p * 2^32).  `offset` is the caller's step counter, `layer` (< 2^30) tells the attention blocks apart.  The
 * result does not depend on the grid (max_blocks caps the forward's, 0 = default) or on which access path runs.
 * p == 0 never calls Philox: the forward is then n_proj plain gad_gemm launches (alpha = scale), bit-equal to the plain
 * down-projection.  No atomics: the dA partials of the row slabs (a plan that depends on M alone) are written to the
 * workspace and added in slab order, so two launches give equal bits.  r a multiple of 4 in 4..64 (zero-padded to the
 * MFMA's 16 in registers); A_j and dA_j contiguous [r][C], mid_j and dmid_j contiguous [M][r]; C % 4 == 0, strides that are
 * multiples of 4 and 16-byte aligned pointers take float4 accesses, anything else guarded scalar ones.  Refused with a
 * named error before any HIP call: p outside [0, 1), n_proj outside 1..4, a short workspace, a null pointer.
 * workspace_bytes >= gad_lora_down_dropout_workspace_bytes(args) (-1 and gad_last_error() if the arguments are refused)
 * serves both directions.
 * gad_lora_merge: W[n][k] += alpha * sum_r B[n][r] A[r][k] in place (W row stride ldw; B [N][r], A [r][K] contiguous):
 * merge_and_unload with alpha = lora_alpha / r, the inverse with -alpha.
 * ---------------------------------------------------------------------------- */
typedef struct gad_lora_dropout_args {
  const float* x;           /* [M][ldx] tokens                                                */
  int64_t ldx;
  int64_t M;
  int32_t C;                /* channels of x (the projections' in_features)                   */
  int32_t r;                /* LoRA rank                                                      */
  int32_t n_proj;           /* 1..4 projections sharing x                                     */
  uint32_t layer;           /* mask stream of this attention block                            */
  const float* A[4];        /* down matrices [r][C]                                           */
  float* mid[4];            /* forward output [M][r]                                          */
  const float* dmid[4];     /* backward input [M][r]                                          */
  float* dA[4];             /* backward output [r][C]                                         */
  float* dx;                /* backward: [M][ld_dx], accumulated onto                         */
  int64_t ld_dx;
  double p;                 /* dropout probability in [0, 1)                                  */
  float scale;              /* forward: lora_alpha / r                                        */
  uint32_t seed, offset;    /* Philox key                                                     */
  int32_t max_blocks;       /* forward grid cap (0 = default)                                 */
  void* workspace;
  int64_t workspace_bytes;
} gad_lora_dropout_args;

int64_t gad_lora_down_dropout_workspace_bytes(const gad_lora_dropout_args* a);
int gad_lora_down_dropout_fwd(const gad_lora_dropout_args* a, void* stream);
int gad_lora_down_dropout_bwd(const gad_lora_dropout_args* a, void* stream);
int gad_lora_merge(float* W, int64_t ldw, const float* B, const float* A, int32_t N, int32_t K, int32_t r, float alpha, void* stream);

/* ------------------------------------------------------------------------------
 * Score tail: the kernels between the convolutions of InceptionV3 (csrc/scorenet.hip, gad/inception.py; reference
 * src/attributions/global_scores/fid_score.py:23-107 and inception_score.py through pytorch-fid's InceptionV3, whose
 * F.max_pool2d / F.avg_pool2d / F.interpolate / F.relu these replace).  fp32 NHWC, bandwidth-bound, 64-bit element
 * offsets; a float4 path along channels where C % 4 == 0, the strides are multiples of 4 and the pointers 16-byte
 * aligned, a scalar path otherwise.  Arguments are checked before any HIP call.
 *
 * gad_pool2d: y[b][oh][ow][c] = pool over the k x k window at (oh * stride - pad, ow * stride - pad) of x[b][..][..][c];
 *   k in {2, 3}, stride in {1, 2}, symmetric pad in {0, 1}, Ho = (H + 2 pad - k) / stride + 1 (floor; Wo alike).
 *   mode GAD_POOL_MAX: padding never wins; GAD_POOL_AVG: sum / k^2 (torch's avg_pool2d default, padding counted);
 *   GAD_POOL_AVG_VALID: sum / taps inside the map (count_include_pad=False).  x has pixel stride ldx >= C and y pixel stride
 *   ldy >= C floats: either may be a channel slice of a wider buffer, only channels [0, C) of a pixel are touched.
 *   relu_in != 0 pools relu(x).
 * gad_resize_bilinear: F.interpolate(x, (Ho, Wo), mode="bilinear", align_corners=False) without antialiasing - source
 *   coordinate (o + 0.5) in / out - 0.5 clamped below at 0, upper neighbour clamped to the last row / column - reading
 *   NCHW x [B][C][H][W], writing NHWC y [B][Ho][Wo][C] = a * v + b.
 * gad_relu: x[r][c] = max(x[r][c], 0) in place for r < rows, c < C, row stride ld >= C.
 * ---------------------------------------------------------------------------- */
enum gad_pool_mode { GAD_POOL_MAX = 0, GAD_POOL_AVG = 1, GAD_POOL_AVG_VALID = 2 };
int gad_pool2d(const float* x, float* y, int32_t B, int32_t H, int32_t W, int32_t C, int32_t ldx, int32_t ldy, int32_t Ho,
               int32_t Wo, int32_t k, int32_t stride, int32_t pad, int32_t mode, int32_t relu_in, void* stream);
int gad_resize_bilinear(const float* x, float* y, int32_t B, int32_t C, int32_t H, int32_t W, int32_t Ho, int32_t Wo, float a,
                        float b, void* stream);
int gad_relu(float* x, int64_t rows, int32_t C, int32_t ld, void* stream);

/* ------------------------------------------------------------------------------
 * Improved precision / recall manifolds on fp16 features (csrc/manifold.hip; reference
 * src/attributions/global_scores/precision_recall.py compute_kth / calc_pr, Kynkaanniemi et al.) without a distance matrix.
 * Features are row-major fp16 matrices [rows][D] with a row stride ld >= D in halves; D and every ld are multiples of 8 and
 * the matrices 16-byte aligned (rows are read as 16-byte chunks; columns [D, ld) are never read).  The distance is defined as
 *   d2(a, b) = max(0, (|a|^2 + |b|^2) - 2 a.b)   norms and dot product accumulated in fp32 from the exact fp16 values
 *   d16(a, b) = (half) sqrtf(d2)                  correctly rounded sqrt, round to nearest even
 * gad_manifold_radii: kth_out[i] (fp16) = the (k+1)-th smallest d16(F_i, F_j) over all j, i included - kthvalue(nhood_size + 1),
 *   selected on d2 and rounded once.  1 <= k <= 7, N >= k + 1.
 * gad_manifold_cover: covered_out[i] (0 / 1) = any_j d16(P_i, T_j) <= kth_T[j] (fp16 radii of the targets), compared in the
 *   fp16-rounded domain.
 * 128 x 128 tiles of dot products on v_mfma_f32_32x32x16_f16; the target axis is split over workgroups, every split keeps
 * its 8 smallest d2 (radii) or one flag (cover) per probe row and column half on chip and writes it to the workspace
 * [2 splits][rows][8 floats | 1 byte] behind the squared norms; a second kernel merges the partials in index order.  No atomics:
 * bit-reproducible.  Workspace 16-byte aligned, ws_bytes >= the matching *_workspace_bytes(...) (-1 and gad_last_error() if the
 * arguments are refused), the function the launch sizes itself by.  Arguments are checked before any HIP call.
 * ---------------------------------------------------------------------------- */
int64_t gad_manifold_radii_workspace_bytes(int32_t N, int32_t D, int32_t ld, int32_t k);
int gad_manifold_radii(const void* F, int32_t N, int32_t D, int32_t ld, int32_t k, void* kth_out, void* ws, int64_t ws_bytes,
                       void* stream);
int64_t gad_manifold_cover_workspace_bytes(int32_t Np, int32_t ldp, int32_t Nt, int32_t ldt, int32_t D);
int gad_manifold_cover(const void* P, int32_t Np, int32_t ldp, const void* T, int32_t Nt, int32_t ldt, int32_t D,
                       const void* kth_T, uint8_t* covered_out, void* ws, int64_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------
 * Score tail: the kernels between the contractions of a pre-LN Vision Transformer image tower (csrc/vit.hip, gad/vit.py:
 * OpenAI CLIP ViT-B/32, open-CLIP ViT-L/14 and the BLIP-VQA vision tower; reference text_to_image/compute_model_behaviors.py:
 * 243-262,358-431 and src/attributions/global_scores/diversity_score.py:89-120).  fp32, bandwidth-bound, 64-bit element
 * offsets, a float4 path where widths, strides and pointers allow it and a scalar path otherwise.  Arguments are checked
 * before any HIP call.
 *
 * gad_resize_bicubic_patches: F.interpolate(x, (rh, rw), mode="bicubic", antialias=True, align_corners=False) of NCHW
 *   x [B][3][H][W], cropped to the R x R window at (oy, ox) and cut into (R / P)^2 patches of P x P, written as the matrix
 *   y [B (R/P)^2][P P 3] = a v + b with (ph, pw, c) fastest - the K-contiguous A operand of the patch embedding.  The
 *   (rh, rw) image is virtual: it is never stored.  CLIP's Resize(n_px) + CenterCrop(n_px) is rh, rw = the shorter side
 *   scaled to R with the crop centred; BLIP's plain resize is rh = rw = R, oy = ox = 0.  The filter is PIL's: cubic
 *   (a = -0.5) widened by fs = max(in / out, 1); output index o has centre c = (o + 0.5) in / out and taps
 *   [max(0, int(c - 2 fs + 0.5)), min(in, int(c + 2 fs + 0.5))) weighted cubic((x - c + 0.5) / fs) / their sum.  PIL's uint8
 *   rounding between and after the two passes is NOT reproduced.  The two per-axis tap tables are built in fp64 by a
 *   pre-kernel into ws (4-byte aligned, ws_bytes >= gad_resize_bicubic_patches_workspace_bytes(...), which returns -1 and sets
 *   gad_last_error() if the geometry is refused: R % P != 0, a crop outside the resized image, a reduction beyond 15 x, or a
 *   patch tile that does not fit 64 KB of LDS) and each workgroup keeps its patch's rows of them in LDS.
 * gad_bicubic_max_taps / gad_bicubic_taps: the same tap function on the HOST in fp64 (no HIP call): for resized indices
 *   [origin, origin + n) of an axis in -> out, start[o], count[o] and w[o][kmax] (zero past count), kmax = gad_bicubic_max_taps.
 * gad_vit_tokens: out[b][t][:] = LN((t == 0 ? cls : patches[b][t - 1]) + pos[t]) for patches [B][T - 1][C], cls [C],
 *   pos [T][C], out [B][T][C]; LN is LayerNorm over C with gamma, beta, eps (two-pass statistics), or the identity when
 *   gamma == beta == NULL.
 * gad_gelu: in place on x[r][c], r < rows, c < C, row stride ld >= C; GAD_GELU_ERF: x (1 + erf(x / sqrt 2)) / 2,
 *   GAD_GELU_QUICK: x sigmoid(1.702 x).
 * gad_l2_normalize_rows: x[r][:] /= |x[r]|_2 in place (row stride ld >= C), fp32 accumulation of a power-of-two scaled row;
 *   no eps: a zero row becomes NaN.
 * ---------------------------------------------------------------------------- */
enum gad_gelu_kind { GAD_GELU_ERF = 0, GAD_GELU_QUICK = 1 };
int64_t gad_resize_bicubic_patches_workspace_bytes(int32_t H, int32_t W, int32_t rh, int32_t rw, int32_t oy, int32_t ox, int32_t R,
                                                   int32_t P);
int gad_resize_bicubic_patches(const float* x, float* y, int32_t B, int32_t H, int32_t W, int32_t rh, int32_t rw, int32_t oy,
                               int32_t ox, int32_t R, int32_t P, float a, float b, void* ws, int64_t ws_bytes, void* stream);
int32_t gad_bicubic_max_taps(int32_t in, int32_t out);
int gad_bicubic_taps(int32_t in, int32_t out, int32_t origin, int32_t n, int32_t* start, int32_t* count, double* w);
int gad_vit_tokens(const float* patches, const float* cls, const float* pos, const float* gamma, const float* beta, float* out,
                   int32_t B, int32_t T, int32_t C, float eps, void* stream);
int gad_gelu(float* x, int64_t rows, int32_t C, int32_t ld, int32_t kind, void* stream);
int gad_l2_normalize_rows(float* x, int64_t rows, int32_t C, int32_t ld, void* stream);

/* ------------------------------------------------------------------------------
 * Text-tower gathers (csrc/text.hip; gad/text.py: CLIP's text transformers).  float4 rows: W % 4 == 0, every pointer 16-byte
 * aligned, ldx % 4 == 0.
 * gad_text_tokens: out[b][t][:] = token_emb[ids[b][t]][:] + pos[t][:] for ids int32 [B][T], token_emb [V][W], pos [T][W],
 *   out [B*T][W].  The caller checks the ids (they come from the host); the kernel clamps them to [0, V) so that it never
 *   reads outside the table.
 * gad_gather_rows: out[b][:] = x[b*T + rows[b]][:] for x [B*T] rows of stride ldx >= W, rows int32 [B] clamped to [0, T),
 *   out [B][W] dense (the end-of-text pooling).
 * ---------------------------------------------------------------------------- */
int gad_text_tokens(const int32_t* ids, const float* token_emb, const float* pos, float* out, int32_t B, int32_t T, int32_t W,
                    int32_t V, void* stream);
int gad_gather_rows(const float* x, const int32_t* rows, float* out, int32_t B, int32_t T, int32_t W, int64_t ldx, void* stream);

/* ------------------------------------------------------------------------------
 * Similarity baselines: every cosine between training rows and generated rows in one pass (csrc/similarity.hip; reference
 * text_to_image/pixel_similarity.py, clip_similarity.py, baselines.py: x /= x.norm(); q /= q.norm(); x @ q).
 *   sim[n][m] = (x_n . q_m) / (|x_n| |q_m|)      X [N][D] training rows, Q [M][D] generated rows (fp32), sim [N][M] fp32, dense
 * x_kind = GAD_SIM_X_F32: X is fp32, ldx in elements, D and ldx multiples of 4; lut is not looked at.
 * x_kind = GAD_SIM_X_U8:  X is uint8, ldx in bytes, D and ldx multiples of 16; the value of byte u is lut[u], a device table of
 *   256 floats the caller fills on the host with ((float)u / 255.0f - 0.5f) / 0.5f (ToTensor + Normalize([0.5], [0.5])).
 * ldq in elements, a multiple of 4; ldx, ldq >= D; X and Q 16-byte aligned; columns [D, ld) are never read.  Any M >= 1: the
 * columns go in blocks of 64 per pass over X, further blocks read X again.
 * The contraction runs on v_mfma_f32_32x32x2_f32 from the exact fp32 values (no bf16 / fp16 rounding); |x_n|^2 is accumulated
 * from the same staged data in the same pass, |q_m|^2 by the first row tile's workgroups alone.  D is split over workgroups
 * in 64-wide steps: every split writes partial dots [splits][N][M] and partial squared norms [splits][N], [splits][M] to the
 * workspace and a second kernel adds them in split order and forms dot / (sqrtf(nx) sqrtf(nq)).  No atomics: bit-reproducible,
 * and at equal `splits` the uint8 path equals the fp32 path on the decoded matrix bit for bit.  splits = 0 lets the launch
 * choose (from N and D alone), a positive value (<= 4096) forces that many; trailing splits may be ragged or empty.  Rows past
 * N, columns past M and k past D are zeros, never read from the matrices.  No eps: a zero row gives NaN.  Workspace 16-byte
 * aligned, ws_bytes >= gad_cosine_rows_workspace_bytes(...) (-1 and gad_last_error() if the arguments are refused), the
 * function the launch sizes itself by.  Arguments are checked before any HIP call.
 * ---------------------------------------------------------------------------- */
enum gad_sim_x_kind { GAD_SIM_X_F32 = 0, GAD_SIM_X_U8 = 1 };
int64_t gad_cosine_rows_workspace_bytes(int64_t N, int64_t M, int64_t D, int32_t x_kind, int32_t splits);
int gad_cosine_rows(const void* X, int32_t x_kind, int64_t ldx, const float* lut, const float* Q, int64_t ldq, float* sim,
                    int64_t N, int64_t M, int64_t D, int32_t splits, void* ws, int64_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------
 * VQModel's codebook lookup (csrc/vae.hip; diffusers VectorQuantizer.forward).  z: n rows of D floats (NHWC latents, row stride
 * ldz), e: the codebook [K][D], dense.  Per row:
 *   idx[r] = argmin_k sum_c (z[r][c] - e[k][c])^2     fp32, exact-difference form, summed in channel order, unfused;
 *                                                     codes scanned in increasing k with a strict <: ties go to the lowest k
 *   zq[r][c] = z[r][c] + (e[idx[r]][c] - z[r][c])     the value of the straight-through z + (z_q - z).detach(), row stride ldzq
 * 1 <= D <= 16, K >= 1, ldz and ldzq >= D; zq must not overlap z.  A row holding a NaN gets index 0 and NaN outputs and
 * disturbs no other row.  One thread per row, the codebook streamed through LDS in 48 KB chunks; no atomics.
 * ---------------------------------------------------------------------------- */
int gad_vq_lookup(const float* z, int64_t ldz, const float* e, int64_t n, int32_t K, int32_t D, int32_t* idx, float* zq,
                  int64_t ldzq, void* stream);

#ifdef __cplusplus
}
#endif
#endif
