// f32-input MFMA contraction engine for gfx950 (MI355X).
//
// One templated kernel covers every matmul-shaped op on the U-Net hot path:
//   conv2d forward   (A = im2col gather of NHWC x,  B = weight [Cout][KH*KW*Cin])
//   conv2d dgrad     (A = transposed gather of dy,   B = weight read as [(r,s,co)][ci])
//   conv2d wgrad     (A = dy^T,                      B = im2col gather as [pixel][(r,s,ci)])
//   Linear fwd/dgrad/wgrad, attention QK^T / PV and their gradients (dense, batched)
// v_mfma_f32_32x32x2_f32 is an exact-fp32 fmaf chain (64 FLOP/clk/SIMD = 157.3 TF/s
// chip peak), so the result matches a CPU fp32 reference to summation-order noise.
//
// Structure (per 256-thread workgroup = 4 waves in a 2x2 arrangement):
//   * block tile BMxBN (128x128 or 64x64), K step 32, two LDS buffers (64 KB at 128x128 -> 2 blocks/CU);
//   * staging is LDS-DMA (global_load_lds_dwordx4, 1 KiB per wave-instruction, no VGPR round trip, no
//     ds_write): each wave-instruction fills 8 tile rows (KC tiles, [row][32 floats]) or 2-4 k-rows (MC
//     tiles, [k][row]); the DMA of step t+1 is issued slot by slot between the MFMA groups of step t so
//     its address arithmetic runs in the shadow of the 64-cycle MFMAs; padding / out-of-range lanes read
//     a 64-byte zero block, so there is no masking and no branch in the K step;
//   * KC tiles are XOR-swizzled on the SOURCE side (16-B chunk q of row r lives at chunk q^((r>>1)&7)):
//     the LDS image stays lane-linear for the DMA and ds_read_b128 of 4 consecutive k is conflict-free;
//     MC tiles are read with ds_read_b32; the k -> (MFMA step, lane half) assignment is the same
//     permutation for both operands so any A/B layout pair composes;
//   * operands that cannot be read as aligned float4 (Cin = 3, Cout = 3, odd K) take a register-staged
//     scalar path (VEC = 1) into the same LDS image;
//   * 1-D grid with an XCD-aware bijective remap so that tiles sharing an A panel sit
//     on one XCD's L2; split-K through a caller-owned workspace + deterministic reduce.
//
// Kernel families in this file (gad_gemm picks one from the shapes; gad_gemm_kernel_id reports it):
//   gemm_kernel                 the generic engine described above (all six operand-layout pairs)
//   conv3x3_patch_f32_kernel    3x3 / stride 1 / pad 1 forward and data gradient with the input patch resident in LDS
//   wgrad3x3_patch_f32_kernel   the matching weight gradient (128 x 288 slab of dW per workgroup)
//   gemm_bf16_kernel            the generic engine with bf16 operands (v_mfma_f32_32x32x16_bf16, fp32 accumulate)
//   conv3x3_patch_bf16_kernel   the patch convolution with bf16 operands (optionally a bf16 weight copy by LDS-DMA)
//   splitk_reduce_kernel        deterministic reduction + fused epilogue of any split launch
// The Winograd routes are planned here (use_wino, use_wino_wgrad) and run by winograd.hip and wino4_fused.hip.
#include "gemm_dev.h"

using namespace gadk;

namespace {

// dense [row][k]
template <int ROWS, int VEC>
struct LoadKCDense : KCSlots<ROWS> {
  using S = KCSlots<ROWS>;
  const float* base;
  long roff[S::NS];
  unsigned rowmask;
  int kend, k;
  bool kok;
  __device__ void init(const float* b, int ld, int row0, int nrows, int kend_) {
    base = b;
    kend = kend_;
    rowmask = 0;
#pragma unroll
    for (int i = 0; i < S::NS; ++i) {
      int r = row0 + S::row(i);
      bool ok = r < nrows;
      roff[i] = ok ? (long)r * ld : 0;
      rowmask |= (unsigned)ok << i;
    }
  }
  __device__ __forceinline__ void prep(int k0, unsigned& mask) {
    k = k0 + S::kq4();
    kok = k < kend;
    mask = rowmask;
  }
  __device__ __forceinline__ const float* src(int i) const {
    bool ok = kok && ((rowmask >> i) & 1u);
    return sel_src(base, roff[i] + k, ok);
  }
  __device__ __forceinline__ void slot(int i, f32x4* v, unsigned& mask) const {
    f32x4 t = zero4();
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      bool ok = k + e < kend;
      float x = base[roff[i] + (ok ? k + e : 0)];
      t[e] = ok ? x : 0.f;
    }
    v[i] = t;
  }
};

// dense [row][k] whose K axis is the concatenation of two tensors: k < ksplit from (base, ld), the rest from (base2, ld2)
// at k - ksplit.  ksplit % 32 == 0, so a K step lies inside one segment; float4 path only.
template <int ROWS>
struct LoadKCDense2 : KCSlots<ROWS> {
  using S = KCSlots<ROWS>;
  const float* base;
  const float* base2;
  long roff[S::NS], roff2[S::NS];
  unsigned rowmask;
  int kend, ksplit, k;
  bool kok, second;
  __device__ void init(const float* b, int ld, const float* b2, int ld2, int ksplit_, int row0, int nrows, int kend_) {
    base = b;
    base2 = b2;
    kend = kend_;
    ksplit = ksplit_;
    rowmask = 0;
#pragma unroll
    for (int i = 0; i < S::NS; ++i) {
      int r = row0 + S::row(i);
      bool ok = r < nrows;
      roff[i] = ok ? (long)r * ld : 0;
      roff2[i] = ok ? (long)r * ld2 : 0;
      rowmask |= (unsigned)ok << i;
    }
  }
  __device__ __forceinline__ void prep(int k0, unsigned& mask) {
    second = k0 >= ksplit;
    k = k0 + S::kq4();
    kok = k < kend;
    mask = rowmask;
  }
  __device__ __forceinline__ const float* src(int i) const {
    bool ok = kok && ((rowmask >> i) & 1u);
    return second ? sel_src(base2, roff2[i] + (k - ksplit), ok) : sel_src(base, roff[i] + k, ok);
  }
  __device__ __forceinline__ void slot(int, f32x4*, unsigned&) const {}
};

// dense [k][row] with the same K concatenation (rows of the second tensor follow the first's)
template <int ROWS>
struct LoadMCDense2 : MCSlots<ROWS> {
  using S = MCSlots<ROWS>;
  const float* base;
  const float* base2;
  int ld, ld2, kend, ksplit, c0, nrows, k0;
  __device__ void init(const float* b, int ld_, const float* b2, int ld2_, int ksplit_, int row0, int nrows_, int kend_) {
    base = b;
    base2 = b2;
    ld = ld_;
    ld2 = ld2_;
    ksplit = ksplit_;
    kend = kend_;
    nrows = nrows_;
    c0 = row0 + S::rq4();
  }
  __device__ __forceinline__ void prep(int k0_, unsigned& mask) {
    k0 = k0_;
    mask = 0;
  }
  __device__ __forceinline__ const float* src(int i) const {
    int k = k0 + S::krow(i);
    bool ok = k < kend && c0 < nrows;
    return k >= ksplit ? sel_src(base2, (long)(k - ksplit) * ld2 + c0, ok) : sel_src(base, (long)k * ld + c0, ok);
  }
  __device__ __forceinline__ void slot(int, f32x4*, unsigned&) const {}
};

// dense [k][row]
template <int ROWS, int VEC>
struct LoadMCDense : MCSlots<ROWS> {
  using S = MCSlots<ROWS>;
  const float* base;
  int ld, kend, c0, nrows, k0;
  __device__ void init(const float* b, int ld_, int row0, int nrows_, int kend_) {
    base = b;
    ld = ld_;
    kend = kend_;
    nrows = nrows_;
    c0 = row0 + S::rq4();
  }
  __device__ __forceinline__ void prep(int k0_, unsigned& mask) {
    k0 = k0_;
    mask = 0;
  }
  __device__ __forceinline__ const float* src(int i) const {
    int k = k0 + S::krow(i);
    bool ok = k < kend && c0 < nrows;
    return sel_src(base, (long)k * ld + c0, ok);
  }
  __device__ __forceinline__ void slot(int i, f32x4* v, unsigned& mask) const {
    int k = k0 + S::krow(i);
    bool kok = k < kend;
    long off = kok ? (long)k * ld : 0;
    f32x4 t = zero4();
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      bool ok = kok && c0 + e < nrows;
      float x = base[off + (ok ? c0 + e : 0)];
      t[e] = ok ? x : 0.f;
    }
    v[i] = t;
    mask |= 1u << i;
  }
};

// ------------------------------------------------------------------------------------
// Lean dense loaders (float4 path, K a multiple of 32 - checked on the host).  Every non-MFMA instruction of a K step
// costs MFMA issue time (tools/micro/mfma_loop_model.hip: 64 full-rate VALU per 64 MFMAs = 3.5 %; a 64 x 64 tile has 16
// MFMAs per wave and step), and the general loaders above spend ~9 VALU per DMA slot on validity selects against the
// zero block and on rebuilding the address.  Here nothing needs masking: rows (or row quads) beyond the tensor are
// CLAMPED to the last valid one - they only feed output rows / columns the epilogue never stores -, K has no tail,
// and the stage fetched "past the end" (never consumed) re-reads the last step.  A slot's pointer is fixed per tile and
// a step adds one wave-uniform offset: one 64-bit add per slot.
// ------------------------------------------------------------------------------------
template <int ROWS>
struct LeanKC : KCSlots<ROWS> {                 // dense [row][k]
  using S = KCSlots<ROWS>;
  const float* ptr[S::NS];
  int kend, koff;
  __device__ void init(const float* b, int ld, int row0, int nrows, int kend_) {
    kend = kend_;
#pragma unroll
    for (int i = 0; i < S::NS; ++i) {
      int r = row0 + S::row(i);
      r = r < nrows ? r : nrows - 1;
      ptr[i] = b + (long)r * ld + S::kq4();
    }
  }
  __device__ __forceinline__ void prep(int k0, unsigned& mask) { koff = k0 < kend ? k0 : kend - BK; mask = 0; }
  __device__ __forceinline__ const float* src(int i) const { return ptr[i] + koff; }
  __device__ __forceinline__ void slot(int, f32x4*, unsigned&) const {}
};
template <int ROWS>
struct LeanMC : MCSlots<ROWS> {                 // dense [k][row]
  using S = MCSlots<ROWS>;
  const float* ptr[S::NS];
  int kend, ld;
  long koff;
  __device__ void init(const float* b, int ld_, int row0, int nrows, int kend_) {
    kend = kend_;
    ld = ld_;
    int c0 = row0 + S::rq4();
    c0 = c0 < nrows ? c0 : nrows - 4;
#pragma unroll
    for (int i = 0; i < S::NS; ++i) ptr[i] = b + (long)S::krow(i) * ld + c0;
  }
  __device__ __forceinline__ void prep(int k0, unsigned& mask) { koff = (long)(k0 < kend ? k0 : kend - BK) * ld; mask = 0; }
  __device__ __forceinline__ const float* src(int i) const { return ptr[i] + koff; }
  __device__ __forceinline__ void slot(int, f32x4*, unsigned&) const {}
};
template <int ROWS>
struct LeanKC2 : KCSlots<ROWS> {                // dense [row][k], K continued in a second tensor at ksplit
  using S = KCSlots<ROWS>;
  const float* ptr[S::NS];
  const float* ptr2[S::NS];
  int kend, ksplit, koff;
  bool second;
  __device__ void init(const float* b, int ld, const float* b2, int ld2, int ksplit_, int row0, int nrows, int kend_) {
    kend = kend_;
    ksplit = ksplit_;
#pragma unroll
    for (int i = 0; i < S::NS; ++i) {
      int r = row0 + S::row(i);
      r = r < nrows ? r : nrows - 1;
      ptr[i] = b + (long)r * ld + S::kq4();
      ptr2[i] = b2 + (long)r * ld2 + S::kq4();
    }
  }
  __device__ __forceinline__ void prep(int k0, unsigned& mask) {
    const int k = k0 < kend ? k0 : kend - BK;
    second = k >= ksplit;
    koff = second ? k - ksplit : k;
    mask = 0;
  }
  __device__ __forceinline__ const float* src(int i) const { return (second ? ptr2[i] : ptr[i]) + koff; }
  __device__ __forceinline__ void slot(int, f32x4*, unsigned&) const {}
};
template <int ROWS>
struct LeanMC2 : MCSlots<ROWS> {                // dense [k][row] with the same K concatenation
  using S = MCSlots<ROWS>;
  const float* ptr[S::NS];
  const float* ptr2[S::NS];
  int kend, ksplit, ld, ld2;
  long koff;
  bool second;
  __device__ void init(const float* b, int ld_, const float* b2, int ld2_, int ksplit_, int row0, int nrows, int kend_) {
    kend = kend_;
    ksplit = ksplit_;
    ld = ld_;
    ld2 = ld2_;
    int c0 = row0 + S::rq4();
    c0 = c0 < nrows ? c0 : nrows - 4;
#pragma unroll
    for (int i = 0; i < S::NS; ++i) {
      ptr[i] = b + (long)S::krow(i) * ld + c0;
      ptr2[i] = b2 + (long)S::krow(i) * ld2 + c0;
    }
  }
  __device__ __forceinline__ void prep(int k0, unsigned& mask) {
    const int k = k0 < kend ? k0 : kend - BK;
    second = k >= ksplit;
    koff = second ? (long)(k - ksplit) * ld2 : (long)k * ld;
    mask = 0;
  }
  __device__ __forceinline__ const float* src(int i) const { return (second ? ptr2[i] : ptr[i]) + koff; }
  __device__ __forceinline__ void slot(int, f32x4*, unsigned&) const {}
};

// im2col gather, rows = output pixels, k = (r, s, c).  TRANSPOSED = dgrad form:
// rows = pixels of the conv INPUT grid, source = dy, src = (row + pad - tap)/stride.
template <int ROWS, bool TRANSPOSED, int VEC, bool TWO = false>
struct LoadConvRows : KCSlots<ROWS> {
  using S = KCSlots<ROWS>;
  const float* x;
  const float* x2;    // TWO: second source of the channel concatenation
  int csplit, ldx2;
  gad_conv_geom g;
  FastDiv fdC, fdKW;
  int bh[S::NS], bw[S::NS], boff[S::NS];  // per row: base h, base w, image pixel offset
  unsigned rowmask;
  int kend, hlim, wlim;
  int k, c, r, s;   // decode of the current K step (prep)
  bool kok;
  __device__ void init(const float* x_, const DevArgs& p, int row0, int nrows, int kend_) {
    x = x_;
    x2 = p.A2;
    csplit = p.a_split;
    ldx2 = p.ldx2;
    g = p.g;
    fdC = p.fdC;
    fdKW = p.fdKW;
    kend = kend_;
    hlim = g.upsample ? 2 * g.H : g.H;
    wlim = g.upsample ? 2 * g.W : g.W;
    rowmask = 0;
#pragma unroll
    for (int i = 0; i < S::NS; ++i) {
      int m = row0 + S::row(i);
      bool ok = m < nrows;
      int mm = ok ? m : 0;
      int img = p.fdHoWo.div(mm), rem = mm - img * (g.Ho * g.Wo);
      int oh = p.fdWo.div(rem), ow = rem - oh * g.Wo;
      boff[i] = img * g.H * g.W;
      rowmask |= (unsigned)ok << i;
      if (TRANSPOSED) {
        bh[i] = oh + g.pad_t;
        bw[i] = ow + g.pad_l;
      } else {
        bh[i] = oh * g.stride - g.pad_t;
        bw[i] = ow * g.stride - g.pad_l;
      }
    }
  }
  // element offset of slot i's pixel for tap (rr,ss); computed unconditionally, `ok` says if it is real
  __device__ __forceinline__ long pix(int i, int rr, int ss, bool& ok) const { return (long)pixidx(i, rr, ss, ok) * g.ldx; }
  __device__ __forceinline__ int pixidx(int i, int rr, int ss, bool& ok) const {
    int ih, iw;
    if (TRANSPOSED) {
      int nh = bh[i] - rr, nw = bw[i] - ss;
      ok = (nh | nw) >= 0;
      if (g.stride == 2) {
        ok = ok && !((nh | nw) & 1);
        nh >>= 1;
        nw >>= 1;
      } else if (g.stride != 1) {
        ok = ok && (nh % g.stride == 0) && (nw % g.stride == 0);
        nh /= g.stride;
        nw /= g.stride;
      }
      ih = nh;
      iw = nw;
    } else {
      ih = bh[i] + rr;
      iw = bw[i] + ss;
      ok = (ih | iw) >= 0;
    }
    ok = ok && ih < hlim && iw < wlim;
    if (g.upsample) {
      ih >>= 1;
      iw >>= 1;
    }
    return boff[i] + ih * g.W + iw;
  }
  __device__ __forceinline__ void prep(int k0, unsigned& mask) {
    k = k0 + S::kq4();
    kok = k < kend;
    int kk = kok ? k : 0;
    int tap = fdC.div(kk);
    c = kk - tap * g.C;
    r = fdKW.div(tap);
    s = tap - r * g.KW;
    mask = rowmask;
  }
  __device__ __forceinline__ const float* src(int i) const {
    bool ok;
    if (TWO) {
      int pi = pixidx(i, r, s, ok);
      ok = ok && kok && ((rowmask >> i) & 1u);
      const bool second = c >= csplit;   // a 32-channel K step lies inside one source (a_split % 32 == 0)
      long off = second ? (long)pi * ldx2 + (c - csplit) : (long)pi * g.ldx + c;
      return sel_src(second ? x2 : x, off, ok);
    }
    long off = pix(i, r, s, ok) + c;
    ok = ok && kok && ((rowmask >> i) & 1u);
    return sel_src(x, off, ok);
  }
  __device__ __forceinline__ void slot(int i, f32x4* v, unsigned& mask) const {
    f32x4 t = zero4();
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      int ke = k + e;
      bool ko = ke < kend;
      int kk = ko ? ke : 0;
      int tap = fdC.div(kk), cc = kk - tap * g.C;
      int rr = fdKW.div(tap), ss = tap - rr * g.KW;
      bool ok;
      long off = pix(i, rr, ss, ok) + cc;
      ok = ok && ko;
      float val = x[off & -(long)ok];
      t[e] = ok ? val : 0.f;
    }
    v[i] = t;
  }
};

// conv weight W[co][tap][ci] read as B[k = tap*Cout + co][n = ci]   (MC-type)
template <int ROWS, int VEC>
struct LoadWDgrad : MCSlots<ROWS> {
  using S = MCSlots<ROWS>;
  const float* base;
  FastDiv fdC;
  int Cout, taps, ncols, kend, c0, k0;
  __device__ void init(const float* w, const DevArgs& p, int col0, int ncols_, int kend_) {
    base = w;
    fdC = p.fdC;
    Cout = p.g.C;
    taps = p.g.KH * p.g.KW;
    ncols = ncols_;
    kend = kend_;
    c0 = col0 + S::rq4();
  }
  __device__ __forceinline__ void prep(int k0_, unsigned& mask) {
    k0 = k0_;
    mask = 0;
  }
  __device__ __forceinline__ const float* src(int i) const {
    int k = k0 + S::krow(i);
    bool ok = k < kend && c0 < ncols;
    int kk = ok ? k : 0;
    int tap = fdC.div(kk), co = kk - tap * Cout;
    return sel_src(base, ((long)co * taps + tap) * ncols + c0, ok);
  }
  __device__ __forceinline__ void slot(int i, f32x4* v, unsigned& mask) const {   // N % 4 == 0 is required
    v[i] = ldg4(src(i));
    mask |= 1u << i;
  }
};

// im2col gather as B[k = pixel][n = (r,s,c)]   (MC-type, wgrad)
template <int ROWS, int VEC>
struct LoadConvCols : MCSlots<ROWS> {
  using S = MCSlots<ROWS>;
  static constexpr int NE = VEC == 4 ? 1 : 4;
  const float* x;
  gad_conv_geom g;
  FastDiv fdHoWo, fdWo;
  int r[NE], s[NE], c[NE];
  bool nok[NE];
  int kend, hlim, wlim, k0;
  __device__ void init(const float* x_, const DevArgs& p, int col0, int ncols, int kend_) {
    x = x_;
    g = p.g;
    fdHoWo = p.fdHoWo;
    fdWo = p.fdWo;
    kend = kend_;
    hlim = g.upsample ? 2 * g.H : g.H;
    wlim = g.upsample ? 2 * g.W : g.W;
    int n = col0 + S::rq4();
#pragma unroll
    for (int e = 0; e < NE; ++e) {
      int ne = n + e;
      nok[e] = ne < ncols;
      int nn = nok[e] ? ne : 0;
      int tap = p.fdC.div(nn);
      c[e] = nn - tap * g.C;
      r[e] = p.fdKW.div(tap);
      s[e] = tap - r[e] * g.KW;
    }
  }
  __device__ __forceinline__ void prep(int k0_, unsigned& mask) {
    k0 = k0_;
    mask = 0;
  }
  __device__ __forceinline__ long off_of(int i, int e, bool& ok) const {
    int m = k0 + S::krow(i);
    bool mok = m < kend;
    int mm = mok ? m : 0;
    int img = fdHoWo.div(mm), rem = mm - img * (g.Ho * g.Wo);
    int oh = fdWo.div(rem), ow = rem - oh * g.Wo;
    int ih = oh * g.stride - g.pad_t + r[e], iw = ow * g.stride - g.pad_l + s[e];
    ok = mok && nok[e] && (ih | iw) >= 0 && ih < hlim && iw < wlim;
    if (g.upsample) {
      ih >>= 1;
      iw >>= 1;
    }
    return (long)(img * g.H * g.W + ih * g.W + iw) * g.ldx + c[e];
  }
  __device__ __forceinline__ const float* src(int i) const {
    bool ok;
    long off = off_of(i, 0, ok);
    return sel_src(x, off, ok);
  }
  __device__ __forceinline__ void slot(int i, f32x4* v, unsigned& mask) const {
    f32x4 t = zero4();
#pragma unroll
    for (int e = 0; e < NE; ++e) {
      bool ok;
      long off = off_of(i, e, ok);
      float val = x[off & -(long)ok];
      t[e] = ok ? val : 0.f;
    }
    v[i] = t;
    mask |= 1u << i;
  }
};

template <int MODE, int ROWS, int VEC>
struct ALoader;
template <int ROWS, int VEC>
struct ALoader<GAD_A_KC, ROWS, VEC> : LoadKCDense<ROWS, VEC> {
  static constexpr bool KC = true;
  __device__ void setup(const DevArgs& p, const float* a, int row0, int kend) { this->init(a, p.lda, row0, p.M, kend); }
};
template <int ROWS, int VEC>
struct ALoader<GAD_A_MC, ROWS, VEC> : LoadMCDense<ROWS, VEC> {
  static constexpr bool KC = false;
  __device__ void setup(const DevArgs& p, const float* a, int row0, int kend) { this->init(a, p.lda, row0, p.M, kend); }
};
template <int ROWS, int VEC>
struct ALoader<GAD_A_CONV, ROWS, VEC> : LoadConvRows<ROWS, false, VEC> {
  static constexpr bool KC = true;
  __device__ void setup(const DevArgs& p, const float* a, int row0, int kend) { this->init(a, p, row0, p.M, kend); }
};
constexpr int A_CONV2 = 16;   // internal: A_CONV reading a two-source channel concatenation
template <int ROWS, int VEC>
struct ALoader<A_CONV2, ROWS, VEC> : LoadConvRows<ROWS, false, VEC, true> {
  static constexpr bool KC = true;
  __device__ void setup(const DevArgs& p, const float* a, int row0, int kend) { this->init(a, p, row0, p.M, kend); }
};
template <int ROWS, int VEC>
struct ALoader<GAD_A_CONVT, ROWS, VEC> : LoadConvRows<ROWS, true, VEC> {
  static constexpr bool KC = true;
  __device__ void setup(const DevArgs& p, const float* a, int row0, int kend) { this->init(a, p, row0, p.M, kend); }
};

constexpr int A_KC2 = 17;     // internal: A_KC whose K axis continues in a second tensor (fused LoRA)
template <int ROWS, int VEC>
struct ALoader<A_KC2, ROWS, VEC> : LoadKCDense2<ROWS> {
  static constexpr bool KC = true;
  __device__ void setup(const DevArgs& p, const float* a, int row0, int kend) {
    this->init(a, p.lda, p.Ak2, p.lda2, p.k_split, row0, p.M, kend);
  }
};

// internal: the lean forms of the dense modes (K % 32 == 0, float4)
constexpr int A_KC_L = 20, A_MC_L = 21, B_KC_L = 22, B_MC_L = 23, A_KC2_L = 24, B_KC2_L = 25, B_MC2_L = 26;
template <int ROWS, int VEC>
struct ALoader<A_KC_L, ROWS, VEC> : LeanKC<ROWS> {
  static constexpr bool KC = true;
  __device__ void setup(const DevArgs& p, const float* a, int row0, int kend) { this->init(a, p.lda, row0, p.M, kend); }
};
template <int ROWS, int VEC>
struct ALoader<A_MC_L, ROWS, VEC> : LeanMC<ROWS> {
  static constexpr bool KC = false;
  __device__ void setup(const DevArgs& p, const float* a, int row0, int kend) { this->init(a, p.lda, row0, p.M, kend); }
};
template <int ROWS, int VEC>
struct ALoader<A_KC2_L, ROWS, VEC> : LeanKC2<ROWS> {
  static constexpr bool KC = true;
  __device__ void setup(const DevArgs& p, const float* a, int row0, int kend) {
    this->init(a, p.lda, p.Ak2, p.lda2, p.k_split, row0, p.M, kend);
  }
};

template <int MODE, int ROWS, int VEC>
struct BLoader;
constexpr int B_KC2 = 18, B_MC2 = 19;   // internal: B_KC / B_MC with the same K concatenation
template <int ROWS, int VEC>
struct BLoader<B_KC_L, ROWS, VEC> : LeanKC<ROWS> {
  static constexpr bool KC = true;
  __device__ void setup(const DevArgs& p, const float* b, int col0, int kend) { this->init(b, p.ldb, col0, p.N, kend); }
};
template <int ROWS, int VEC>
struct BLoader<B_MC_L, ROWS, VEC> : LeanMC<ROWS> {
  static constexpr bool KC = false;
  __device__ void setup(const DevArgs& p, const float* b, int col0, int kend) { this->init(b, p.ldb, col0, p.N, kend); }
};
template <int ROWS, int VEC>
struct BLoader<B_KC2_L, ROWS, VEC> : LeanKC2<ROWS> {
  static constexpr bool KC = true;
  __device__ void setup(const DevArgs& p, const float* b, int col0, int kend) {
    this->init(b, p.ldb, p.Bk2, p.ldb2, p.k_split, col0, p.N, kend);
  }
};
template <int ROWS, int VEC>
struct BLoader<B_MC2_L, ROWS, VEC> : LeanMC2<ROWS> {
  static constexpr bool KC = false;
  __device__ void setup(const DevArgs& p, const float* b, int col0, int kend) {
    this->init(b, p.ldb, p.Bk2, p.ldb2, p.k_split, col0, p.N, kend);
  }
};
template <int ROWS, int VEC>
struct BLoader<B_KC2, ROWS, VEC> : LoadKCDense2<ROWS> {
  static constexpr bool KC = true;
  __device__ void setup(const DevArgs& p, const float* b, int col0, int kend) {
    this->init(b, p.ldb, p.Bk2, p.ldb2, p.k_split, col0, p.N, kend);
  }
};
template <int ROWS, int VEC>
struct BLoader<B_MC2, ROWS, VEC> : LoadMCDense2<ROWS> {
  static constexpr bool KC = false;
  __device__ void setup(const DevArgs& p, const float* b, int col0, int kend) {
    this->init(b, p.ldb, p.Bk2, p.ldb2, p.k_split, col0, p.N, kend);
  }
};
template <int ROWS, int VEC>
struct BLoader<GAD_B_KC, ROWS, VEC> : LoadKCDense<ROWS, VEC> {
  static constexpr bool KC = true;
  __device__ void setup(const DevArgs& p, const float* b, int col0, int kend) { this->init(b, p.ldb, col0, p.N, kend); }
};
template <int ROWS, int VEC>
struct BLoader<GAD_B_MC, ROWS, VEC> : LoadMCDense<ROWS, VEC> {
  static constexpr bool KC = false;
  __device__ void setup(const DevArgs& p, const float* b, int col0, int kend) { this->init(b, p.ldb, col0, p.N, kend); }
};
template <int ROWS, int VEC>
struct BLoader<GAD_B_WDGRAD, ROWS, VEC> : LoadWDgrad<ROWS, VEC> {
  static constexpr bool KC = false;
  __device__ void setup(const DevArgs& p, const float* b, int col0, int kend) { this->init(b, p, col0, p.N, kend); }
};
template <int ROWS, int VEC>
struct BLoader<GAD_B_CONV, ROWS, VEC> : LoadConvCols<ROWS, VEC> {
  static constexpr bool KC = false;
  __device__ void setup(const DevArgs& p, const float* b, int col0, int kend) { this->init(b, p, col0, p.N, kend); }
};


// TAG only names an instance apart in profiles (1: the 36 batched products of the F(4x4) Winograd route)
template <int AM, int BMODE, int BM, int BN, int VEC, int TAG = 0>
__global__ __launch_bounds__(NTHREADS) void gemm_kernel(const DevArgs p) {
  constexpr int TM = BM / 64, TN = BN / 64;
  using AL = ALoader<AM, BM, VEC>;
  using BL = BLoader<BMODE, BN, VEC>;
  constexpr int A_TILE = BK * BM;
  constexpr int B_TILE = BK * BN;
  __shared__ __attribute__((aligned(16))) float lds[2 * (A_TILE + B_TILE)];

  // ---- block -> (batch z, split, tile_m, tile_n), XCD-aware (bijective) ----
  const int t = xcd_remap(blockIdx.x, gridDim.x);
  int tiles = p.tiles_m * p.tiles_n;
  int zs = t / tiles, rem = t - zs * tiles;
  int tile_m = rem / p.tiles_n, tile_n = rem - tile_m * p.tiles_n;
  int z = zs / p.splitk, split = zs - z * p.splitk;
  int z0 = z / p.batch_inner, z1 = z - z0 * p.batch_inner;
  const float* A = p.A + z0 * p.sA0 + z1 * p.sA1;
  const float* B = p.B + z0 * p.sB0 + z1 * p.sB1;

  int row0 = tile_m * BM, col0 = tile_n * BN;
  int kbeg = split * p.ktiles_per_split * BK;
  int kend = min(p.K, kbeg + p.ktiles_per_split * BK);
  int nkt = (kend - kbeg + BK - 1) / BK;
  // K-step order.  For the conv gathers the natural (tap-major) order walks a workgroup's whole input
  // footprint once per tap - (rows+2) x W x C floats, tens to hundreds of KB, evicted from L1/L2 between
  // taps - so every tap re-fetches it through the fabric.  Visiting the KH*KW taps of one 32-channel chunk
  // back to back keeps the live footprint at (rows+2) x W x 32 floats and the re-reads on chip.  Any order
  // gives the same sum up to fp32 reassociation.
  const int kt0 = split * p.ktiles_per_split;
  auto k0_of = [&](int kt) -> int {
    if (!p.kperm) return (kt0 + kt) * BK;
    int j = kt0 + kt;
    int chunk = p.fdTaps.div(j), tap = j - chunk * p.taps;
    return tap * p.g.C + chunk * BK;
  };
  if (p.kperm) kend = p.K;

  AL al;
  BL bl;
  al.setup(p, A, row0, kend);
  bl.setup(p, B, col0, kend);

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int wm = wave >> 1, wn = wave & 1, h = lane >> 5, l31 = lane & 31;

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  // stage(tile buffers, k0): bring the K step starting at k0 into LDS.  VEC==4: one DMA per slot;
  // VEC==1: scalar gathers into registers (ra/rb), written to LDS by stage_commit().
  f32x4 ra[VEC == 4 ? 1 : AL::NS], rb[VEC == 4 ? 1 : BL::NS];
  unsigned ma = 0, mb = 0;
  auto stage_slot = [&](int piece, float* ta, float* tb) {
    constexpr int NSA = AL::NS, NSB = BL::NS;
    if (piece < NSA) {
      if (VEC == 4) glds16(al.src(piece), AL::dma_dst(ta, piece));
      else al.slot(piece, ra, ma);
    } else if (piece < NSA + NSB) {
      if (VEC == 4) glds16(bl.src(piece - NSA), BL::dma_dst(tb, piece - NSA));
      else bl.slot(piece - NSA, rb, mb);
    }
  };
  auto stage_commit = [&](float* ta, float* tb) {
    if (VEC != 4) {
      AL::store(ta, ra, ma);
      BL::store(tb, rb, mb);
    }
  };
  if (nkt > 0) {
    al.prep(k0_of(0), ma);
    bl.prep(k0_of(0), mb);
#pragma unroll
    for (int q = 0; q < AL::NS + BL::NS; ++q) stage_slot(q, lds, lds + A_TILE);
    stage_commit(lds, lds + A_TILE);
  }
  barrier_after_dma();

  // One K step = 16 "pieces" of TM*TN MFMAs (4 fragment groups x 4 MFMA steps).  The staging of step
  // kt+1 (into the other buffer, last read before the previous barrier) is issued one slot per piece
  // from the first pieces on - unconditional: past the end it fetches the zero block - pinned there by
  // sched_barrier so its address VALU runs in the shadow of the 64-cycle MFMAs; the fragments of
  // group g+1 are read during group g.  (mfma_kstep of gemm_dev.h is this step; written out here because
  // through the shared function hipcc computes the fragment addresses of every instance differently.)
  for (int kt = 0; kt < nkt; ++kt) {
    float* cur = lds + (kt & 1) * (A_TILE + B_TILE);
    float* nxt = lds + ((kt + 1) & 1) * (A_TILE + B_TILE);
    const float* la = cur;
    const float* lb = cur + A_TILE;
    const int knext = (kt + 1 < nkt) ? k0_of(kt + 1) : p.K;   // past the end: k >= kend, every slot reads zeros
    al.prep(knext, ma);
    bl.prep(knext, mb);
    f32x4 fa[2][TM], fb[2][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i) fa[0][i] = read_frag<AL::KC, BM>(la, wm * (BM / 2) + i * 32 + l31, 0, h);
#pragma unroll
    for (int j = 0; j < TN; ++j) fb[0][j] = read_frag<BL::KC, BN>(lb, wn * (BN / 2) + j * 32 + l31, 0, h);
#pragma unroll
    for (int g = 0; g < 4; ++g) {
#pragma unroll
      for (int s = 0; s < 4; ++s) {
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[g & 1][i][s], fb[g & 1][j][s], acc[i][j], 0, 0, 0);
        stage_slot(g * 4 + s, nxt, nxt + A_TILE);
        if (s == 1 && g < 3) {   // prefetch the next group's fragments into the other register set
#pragma unroll
          for (int i = 0; i < TM; ++i) fa[(g + 1) & 1][i] = read_frag<AL::KC, BM>(la, wm * (BM / 2) + i * 32 + l31, g + 1, h);
#pragma unroll
          for (int j = 0; j < TN; ++j) fb[(g + 1) & 1][j] = read_frag<BL::KC, BN>(lb, wn * (BN / 2) + j * 32 + l31, g + 1, h);
        }
        // within the piece: alternate 1 MFMA with <= 7 VALU so the staging arithmetic never holds back
        // the next MFMA by more than its 64-cycle shadow
#pragma unroll
        for (int q = 0; q < TM * TN; ++q) {
          __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
          __builtin_amdgcn_sched_group_barrier(0x002, 7, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    stage_commit(nxt, nxt + A_TILE);
    barrier_after_dma();   // all DMA of step kt+1 landed (vmcnt(0)) and every wave is done reading `cur`
  }

  // ---- epilogue: C/D map col = lane&31, row = (reg&3) + 8*(reg>>2) + 4*(lane>>5) ----
  const bool direct = p.splitk == 1;
  float* C = direct ? p.C + z0 * p.sC0 + z1 * p.sC1 : p.ws + (long)zs * p.M * p.N;
  const float* R = (direct && p.residual) ? p.residual + z0 * p.sC0 + z1 * p.sC1 : nullptr;
  const int ldc = direct ? p.ldc : p.N;
  store_block<TM, TN, BM, BN>(p, acc, row0, col0, wm, wn, h, l31, C, ldc, R, direct, lds + (tid >> 6) * EPI_WAVE);
}

// ------------------------------------------------------------------------------------
// bf16-operand variant (gad_gemm_args.operand_precision == 1): A and B are still fp32 in HBM; the loaders'
// 16-B gathers go through registers, are rounded to bf16 (RNE, v_cvt_pk_bf16_f32) and stored into bf16 LDS tiles
// [rows][32 k + 8 pad] (80-B rows: a wave's ds_read_b128 of 16 consecutive rows covers all 64 banks once); the
// products run on v_mfma_f32_32x32x16_bf16 (lane l: row l&31, k = 8(l>>5)+j) with fp32 accumulation and the same
// C/D map and epilogue as the fp32 kernel.  Row-contiguous (MC-type) operands keep their [k][row] image and are
// read with the transposing ds_read_b64_tr_b16.  All six operand pairs are instantiated; launches whose operands
// cannot be read as aligned float4 (Cin = 3, Tk = 77 ...) stay on the fp32 kernel.
// ------------------------------------------------------------------------------------
constexpr int LDK = BK + 8;
// MC-type tiles [32 k][rows + pad]: the row stride in dwords is 16 (mod 64) (rows 128) or 48 (mod 64) (rows 64), so the
// 4 k-rows x 16-dword segments one 32-lane half of a ds_read_b64_tr_b16 touches are 64 distinct banks
template <int ROWS> struct LdmOf { static constexpr int v = ROWS == 128 ? 160 : 96; };

__device__ __forceinline__ void store_bf16x4(unsigned short* dst, f32x4 v) {
  bf16x4 h = {(__bf16)v[0], (__bf16)v[1], (__bf16)v[2], (__bf16)v[3]};
  *reinterpret_cast<bf16x4*>(dst) = h;
}

// bf16 tile of one operand: element count, where a thread's slot i goes, and the MFMA fragment of a 32-row
// block (rows r0 .. r0+31) for k sub-step ks (16 k each): lane l holds k = 16 ks + 8 (l>>5) + j, j = 0..7
template <bool KC, int ROWS>
struct Bf16Tile;
template <int ROWS>
struct Bf16Tile<true, ROWS> {
  static constexpr int ELEMS = LDK * ROWS;
  __device__ static void put(unsigned short* tile, int i, f32x4 v) {
    store_bf16x4(tile + KCSlots<ROWS>::row(i) * LDK + KCSlots<ROWS>::kq4(), v);
  }
  __device__ static bf16x8 frag(const unsigned short* tile, int r0, int ks, int lane) {
    return *reinterpret_cast<const bf16x8*>(tile + (r0 + (lane & 31)) * LDK + ks * 16 + 8 * (lane >> 5));
  }
};
template <int ROWS>
struct Bf16Tile<false, ROWS> {
  static constexpr int LDM = LdmOf<ROWS>::v;
  static constexpr int ELEMS = BK * LDM;
  __device__ static void put(unsigned short* tile, int i, f32x4 v) {
    store_bf16x4(tile + MCSlots<ROWS>::krow(i) * LDM + MCSlots<ROWS>::rq4(), v);
  }
  // transposed read: per 16-lane group a 4(k) x 16(row) block; lane 4q+p supplies row q, columns 4p..4p+3 and
  // receives the 4 k-values of column (lane & 15)  (every lane must be active: EXEC all ones)
  __device__ static bf16x8 frag(const unsigned short* tile, int r0, int ks, int lane) {
    const int q = (lane & 15) >> 2, pp = lane & 3;
    const unsigned short* a0 = tile + (ks * 16 + 8 * (lane >> 5) + q) * LDM + r0 + 16 * ((lane >> 4) & 1) + 4 * pp;
    s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)a0);
    s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(a0 + 4 * LDM));
    s16x8 both = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(bf16x8, both);
  }
};

template <int AM, int BMODE, int BM, int BN>
__global__ __launch_bounds__(NTHREADS) void gemm_bf16_kernel(const DevArgs p) {
  constexpr int TM = BM / 64, TN = BN / 64;
  using AL = ALoader<AM, BM, 4>;
  using BL = BLoader<BMODE, BN, 4>;
  using AT = Bf16Tile<AL::KC, BM>;
  using BT = Bf16Tile<BL::KC, BN>;
  constexpr int A_TILE = AT::ELEMS;
  constexpr int B_TILE = BT::ELEMS;
  __shared__ __attribute__((aligned(16))) unsigned short lds[2 * (A_TILE + B_TILE)];

  const int t = xcd_remap(blockIdx.x, gridDim.x);
  int tiles = p.tiles_m * p.tiles_n;
  int zs = t / tiles, rem = t - zs * tiles;
  int tile_m = rem / p.tiles_n, tile_n = rem - tile_m * p.tiles_n;
  int z = zs / p.splitk, split = zs - z * p.splitk;
  int z0 = z / p.batch_inner, z1 = z - z0 * p.batch_inner;
  const float* A = p.A + z0 * p.sA0 + z1 * p.sA1;
  const float* B = p.B + z0 * p.sB0 + z1 * p.sB1;

  int row0 = tile_m * BM, col0 = tile_n * BN;
  int kbeg = split * p.ktiles_per_split * BK;
  int kend = min(p.K, kbeg + p.ktiles_per_split * BK);
  int nkt = (kend - kbeg + BK - 1) / BK;
  const int kt0 = split * p.ktiles_per_split;
  auto k0_of = [&](int kt) -> int {
    if (!p.kperm) return (kt0 + kt) * BK;
    int j = kt0 + kt;
    int chunk = p.fdTaps.div(j), tap = j - chunk * p.taps;
    return tap * p.g.C + chunk * BK;
  };
  if (p.kperm) kend = p.K;

  AL al;
  BL bl;
  al.setup(p, A, row0, kend);
  bl.setup(p, B, col0, kend);

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int wm = wave >> 1, wn = wave & 1, h = lane >> 5, l31 = lane & 31;

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  f32x4 ra[AL::NS], rb[BL::NS];
  unsigned mdummy = 0;
  // all of a thread's gathers of one K step are issued together (invalid slots read the zero block)
  auto fetch = [&](int k0) {
    al.prep(k0, mdummy);
    bl.prep(k0, mdummy);
#pragma unroll
    for (int i = 0; i < AL::NS; ++i) ra[i] = ldg4(al.src(i));
#pragma unroll
    for (int i = 0; i < BL::NS; ++i) rb[i] = ldg4(bl.src(i));
  };
  auto commit = [&](unsigned short* ta, unsigned short* tb) {
#pragma unroll
    for (int i = 0; i < AL::NS; ++i) AT::put(ta, i, ra[i]);
#pragma unroll
    for (int i = 0; i < BL::NS; ++i) BT::put(tb, i, rb[i]);
  };
  if (nkt > 0) {
    fetch(k0_of(0));
    commit(lds, lds + A_TILE);
  }
  __syncthreads();

  for (int kt = 0; kt < nkt; ++kt) {
    unsigned short* cur = lds + (kt & 1) * (A_TILE + B_TILE);
    unsigned short* nxt = lds + ((kt + 1) & 1) * (A_TILE + B_TILE);
    const unsigned short* la = cur;
    const unsigned short* lb = cur + A_TILE;
    fetch((kt + 1 < nkt) ? k0_of(kt + 1) : p.K);   // past the end every slot reads zeros
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8 fa[TM], fb[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i) fa[i] = AT::frag(la, wm * (BM / 2) + i * 32, ks, lane);
#pragma unroll
      for (int j = 0; j < TN; ++j) fb[j] = BT::frag(lb, wn * (BN / 2) + j * 32, ks, lane);
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i], fb[j], acc[i][j], 0, 0, 0);
    }
    commit(nxt, nxt + A_TILE);   // `nxt` was last read before the previous barrier
    __syncthreads();
  }

  const bool direct = p.splitk == 1;
  float* C = direct ? p.C + z0 * p.sC0 + z1 * p.sC1 : p.ws + (long)zs * p.M * p.N;
  const float* R = (direct && p.residual) ? p.residual + z0 * p.sC0 + z1 * p.sC1 : nullptr;
  const int ldc = direct ? p.ldc : p.N;
  static_assert(sizeof(lds) >= 4 * EPI_WAVE * sizeof(float), "epilogue scratch");
  store_block<TM, TN, BM, BN>(p, acc, row0, col0, wm, wn, h, l31, C, ldc, R, direct, reinterpret_cast<float*>(lds) + (tid >> 6) * EPI_WAVE);
}

// ------------------------------------------------------------------------------------
// 3x3 / stride 1 / pad 1 convolution forward with bf16 operands from an LDS-resident input patch.
// A workgroup owns 128 consecutive output pixels of one image = TR = 128 / W whole rows.  Per 32-channel chunk the
// (TR+2) x (W+2) input patch (halo included, zeros outside the image) is fetched ONCE, rounded to bf16 and kept in LDS;
// the nine taps read their A fragments from that patch at shifted pixel offsets (ds_read_b128, 80-B pixel stride:
// conflict-free), so the input is not re-gathered per tap: global fetch of the A operand drops 9x -> (TR+2)(W+2)/(TR W)x
// and the per-step address arithmetic disappears.  Weights stream through a double-buffered [128][32+8] bf16 tile
// per (chunk, tap) exactly as in gemm_bf16_kernel.  K order = (chunk, tap); fp32 accumulation; same epilogue.
// ------------------------------------------------------------------------------------
// WB: the weights come as a bf16 copy (cast once per set of weights on the host side): their [128][32] tile is 64-B rows
// filled by LDS-DMA - 16 rows per wave-instruction, two instructions per wave and step, no registers, no convert, no
// ds_write - with the four 16-B chunks of a row XOR-swizzled by (row >> 2) & 3 on the source side, so that the 16 rows of a
// ds_read_b128 phase cover the 64 banks once.
template <int W, int NI, bool WB>
__global__ __launch_bounds__(NTHREADS, (W == 64 || NI == 8) ? 2 : 3) void conv3x3_patch_bf16_kernel(const DevArgs p) {   // 3 waves / SIMD (<= 168 registers) where LDS allows 3 workgroups
  constexpr int BM = 128, BN = 128, TM = 2, TN = 2;
  // NI = 1: the tile is TR = 128 / W rows of one image.  NI > 1 (small maps): the tile is NI whole TR x W images,
  // each with its own halo'd sub-patch.
  constexpr int TR = BM / (W * NI), PW = W + 2, PR = TR + 2, NPIX = NI * PR * PW;
  constexpr int PSLOTS = (NPIX * 8 + NTHREADS - 1) / NTHREADS;      // float4 slots per thread per patch
  constexpr int P_TILE = NPIX * LDK;                                 // bf16 elements
  constexpr int B_TILE = WB ? BN * BK : BN * LDK;
  using BL = BLoader<GAD_B_KC, BN, 4>;
  __shared__ __attribute__((aligned(16))) unsigned short lds[2 * P_TILE + 2 * B_TILE];
  unsigned short* const patch0 = lds;
  unsigned short* const btile0 = lds + 2 * P_TILE;

  const int t = xcd_remap(blockIdx.x, gridDim.x);
  int tile_m = t / p.tiles_n, tile_n = t - tile_m * p.tiles_n;
  const int row0 = tile_m * BM, col0 = tile_n * BN;
  // H x W: the conv's input grid as the taps see it (= output grid); with the fused nearest-2x upsample the stored
  // tensor is (H/2) x (W/2) and patch pixel (ih, iw) reads stored pixel (ih>>1, iw>>1)
  const int H = p.g.Ho, C = p.g.C, ups = p.g.upsample;
  const int img = row0 / (H * W), oh0 = NI == 1 ? (row0 - img * (H * W)) / W : 0;
  const int nchunks = C / BK;

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int wm = wave >> 1, wn = wave & 1, h = lane >> 5, l31 = lane & 31;

  // patch slots of this thread: slot j = tid + 256 i -> patch pixel j / 8, float4 j % 8
  int poff[PSLOTS];     // element offsets fit 32 bits (the host checks pixels * ldx < 2^31)
  unsigned pvalid = 0;
#pragma unroll
  for (int i = 0; i < PSLOTS; ++i) {
    int j = tid + NTHREADS * i;
    int pp = j >> 3, q4 = (j & 7) * 4;
    int il = pp / (PR * PW), prem = pp - il * (PR * PW);
    int pr = prem / PW, pc = prem - pr * PW;
    int ih = oh0 + pr - 1, iw = pc - 1;
    bool ok = pp < NPIX && ih >= 0 && ih < H && iw >= 0 && iw < W;
    poff[i] = ok ? (((img + il) * p.g.H + (ih >> ups)) * p.g.W + (iw >> ups)) * p.g.ldx + q4 : 0;
    pvalid |= (unsigned)ok << i;
  }
  static_assert(PSLOTS <= 9, "one patch slot per tap, committed at the next tap");
  // slot i of the NEXT chunk's patch is fetched at tap i and written to the other patch buffer at tap i + 1
  // (that buffer was last read in the previous chunk), so only one float4 of the patch is in registers at a time
  f32x4 rp1;
  auto fetch_slot = [&](int i, int chunk) { rp1 = ldg4(sel_src(p.A, (long)poff[i] + chunk * BK, (pvalid >> i) & 1u)); };
  auto commit_slot = [&](int i, unsigned short* dst) {
    int j = tid + NTHREADS * i;
    if (j < NPIX * 8) store_bf16x4(dst + (j >> 3) * LDK + (j & 7) * 4, rp1);
  };

  BL bl;
  bl.setup(p, p.B, col0, p.K);
  f32x4 rb[BL::NS];
  unsigned mdummy = 0;
  auto fetch_b = [&](int k0) {
    bl.prep(k0, mdummy);
#pragma unroll
    for (int i = 0; i < BL::NS; ++i) rb[i] = ldg4(bl.src(i));
  };
  auto commit_b = [&](unsigned short* tb) {
#pragma unroll
    for (int i = 0; i < BL::NS; ++i) Bf16Tile<true, BN>::put(tb, i, rb[i]);
  };
  // WB: DMA of the bf16 weight tile of the step starting at k0 (lane -> row lane/4 of 16, physical chunk lane&3)
  auto dma_b = [&](int k0, unsigned short* tb) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int row = j * 64 + wave * 16 + (lane >> 2);
      const int c = (lane & 3) ^ ((row >> 2) & 3);
      const bool ok = col0 + row < p.N && k0 < p.K;
      const unsigned short* src = ok ? p.Bh + (long)(col0 + row) * p.ldb + k0 + c * 8 : g_zero_block.b16;
      glds16(src, tb + (j * 64 + wave * 16) * BK);
    }
  };
  auto frag_b = [&](const unsigned short* tb, int r0, int ks) -> bf16x8 {
    if (!WB) return Bf16Tile<true, BN>::frag(tb, r0, ks, lane);
    const int row = r0 + l31;
    return *reinterpret_cast<const bf16x8*>(tb + row * BK + (((2 * ks + h) ^ ((row >> 2) & 3)) << 3));
  };

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  // A-fragment base of this lane inside a patch: output pixel m -> patch pixel (m / W) * PW + m % W (+ tap shift)
  int abase[TM];
#pragma unroll
  for (int i = 0; i < TM; ++i) {
    int m = wm * (BM / 2) + i * 32 + l31;
    abase[i] = ((m / (TR * W)) * (PR * PW) + ((m / W) % TR) * PW + (m % W)) * LDK + 8 * h;
  }

#pragma unroll
  for (int i = 0; i < PSLOTS; ++i) {
    fetch_slot(i, 0);
    commit_slot(i, patch0);
  }
  if (WB) dma_b(0, btile0);
  else {
    fetch_b(0);
    commit_b(btile0);
  }
  if (WB) barrier_after_dma();
  else __syncthreads();

  const int nsteps = nchunks * 9;
  int chunk = 0, tap = 0;
  for (int st = 0; st < nsteps; ++st) {
    const unsigned short* pa = patch0 + (chunk & 1) * P_TILE;
    const unsigned short* lb = btile0 + (st & 1) * B_TILE;
    unsigned short* nb = btile0 + ((st + 1) & 1) * B_TILE;
    // next step's weights; at the first tap also the next chunk's patch (past the end: zeros / clamped chunk)
    int ntap = tap + 1, nchunk = chunk;
    if (ntap == 9) { ntap = 0; ++nchunk; }
    const int knext = st + 1 < nsteps ? ntap * C + nchunk * BK : p.K;
    if (WB) dma_b(knext, nb);
    else fetch_b(knext);
    unsigned short* const pnext = patch0 + ((chunk + 1) & 1) * P_TILE;
    const int cnext = chunk + 1 < nchunks ? chunk + 1 : chunk;
#pragma unroll
    for (int i = 0; i < PSLOTS; ++i)      // tap is workgroup-uniform; the unrolled compare keeps poff[] in registers
      if (tap == i + 1) commit_slot(i, pnext);
#pragma unroll
    for (int i = 0; i < PSLOTS; ++i)
      if (tap == i) fetch_slot(i, cnext);
    const int r = tap / 3, s3 = tap - r * 3;
    const int tshift = (r * PW + s3) * LDK;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8 fa[TM], fb[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i) fa[i] = *reinterpret_cast<const bf16x8*>(pa + abase[i] + tshift + ks * 16);
#pragma unroll
      for (int j = 0; j < TN; ++j) fb[j] = frag_b(lb, wn * (BN / 2) + j * 32, ks);
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i], fb[j], acc[i][j], 0, 0, 0);
    }
    if (!WB) commit_b(nb);
    if (PSLOTS == 9 && tap == 8) commit_slot(8, pnext);   // a ninth slot (W = 64) has no next tap to ride on
    if (WB) barrier_after_dma();
  else __syncthreads();
    tap = ntap;
    chunk = nchunk;
  }

  store_block<TM, TN, BM, BN>(p, acc, row0, col0, wm, wn, h, l31, p.C, p.ldc, p.residual, true, reinterpret_cast<float*>(lds) + (tid >> 6) * EPI_WAVE);
}

// ------------------------------------------------------------------------------------
// fp32 twin of the LDS-patch convolution: exact f32 MFMAs, weights streamed by LDS-DMA exactly as in gemm_kernel, the
// A operand read from an fp32 input patch [(TR+2)(W+2)][32 + 4 pad] (144-B pixel stride: a phase of 16 consecutive
// pixels of a ds_read_b128 covers all 64 banks).  Versus the generic kernel the per-step A gather (half of the LDS-DMA
// traffic, all of the im2col address arithmetic) is gone; the input is fetched (TR+2)(W+2)/(TR W) ~ 1.6x instead of 9x.
// One patch buffer: the next chunk's patch is prefetched into registers, one float4 per tap, and written between two
// barriers after the chunk's last tap (one extra barrier per 9 K steps).
// ------------------------------------------------------------------------------------
constexpr int PLD = BK + 4;
// DG = true: the data gradient of the same convolution - rows are input pixels, the patch holds dy, tap (r, s) reads it at
// (ih + 1 - r, iw + 1 - s) (mirrored shifts) and the weights W[co][r][s][ci] stream as B[k = (tap, co)][n = ci]
// ([k][n] tiles, read like the generic dgrad).
// Forward: 4 x 1 waves of 32 pixels x BN_ channels, BN_ = 128, or 96 / 160 for output-channel counts that 128 would pad
// by a quarter or more (pruned widths 96 / 192 / 288, CelebA 672, SD 320).  4 x 1 measured 1-4 % over 2 x 2 waves of
// 64 x 64 at BN_ = 128 (tools/ab_patch.py).  The data gradient keeps 2 x 2 (its [k][n] weight tiles are read per column).
template <int W, int NI, bool DG, int BN_ = 128, int WM_ = (DG ? 2 : 4)>
__global__ __launch_bounds__(NTHREADS) void conv3x3_patch_f32_kernel(const DevArgs p) {
  constexpr int BM = 128, BN = BN_, WM = WM_, WN = 4 / WM, TM = BM / (32 * WM), TN = BN / (32 * WN);
  static_assert(!DG || BN_ == 128, "the data-gradient form streams [k][n] weight tiles: 128 columns only");
  // NI = 1: the tile is TR = 128 / W rows of one image.  NI > 1 (small maps): the tile is NI whole TR x W images,
  // each with its own halo'd sub-patch.
  constexpr int TR = BM / (W * NI), PW = W + 2, PR = TR + 2, NPIX = NI * PR * PW;
  constexpr int PSLOTS = (NPIX * 8 + NTHREADS - 1) / NTHREADS;
  constexpr int B_TILE = BK * BN;
  using BL = BLoader<DG ? GAD_B_WDGRAD : GAD_B_KC, BN, 4>;
  static_assert(PSLOTS <= 9, "one patch slot per tap");
  __shared__ __attribute__((aligned(16))) float lds[NPIX * PLD + 2 * B_TILE];
  float* const patch = lds;
  float* const btile0 = lds + NPIX * PLD;

  const int t = xcd_remap(blockIdx.x, gridDim.x);
  // split-K over the 32-channel chunks (small maps: few tiles, long K): split s owns chunks [c_begin, c_end)
  const int tiles = p.tiles_m * p.tiles_n;
  const int split = t / tiles, trem = t - split * tiles;
  int tile_m = trem / p.tiles_n, tile_n = trem - tile_m * p.tiles_n;
  const int row0 = tile_m * BM, col0 = tile_n * BN;
  // H x W: the conv's input grid as the taps see it (= output grid); with the fused nearest-2x upsample the stored
  // tensor is (H/2) x (W/2) and patch pixel (ih, iw) reads stored pixel (ih>>1, iw>>1)
  const int H = p.g.Ho, C = p.g.C, ups = p.g.upsample;
  const int img = row0 / (H * W), oh0 = NI == 1 ? (row0 - img * (H * W)) / W : 0;
  const int c_begin = split * p.ktiles_per_split;
  const int c_end = min(C / BK, c_begin + p.ktiles_per_split);

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int wm = wave / WN, wn = wave % WN, h = lane >> 5, l31 = lane & 31;

  int poff[PSLOTS];
  unsigned pvalid = 0;
#pragma unroll
  for (int i = 0; i < PSLOTS; ++i) {
    int j = tid + NTHREADS * i;
    int pp = j >> 3, q4 = (j & 7) * 4;
    int il = pp / (PR * PW), prem = pp - il * (PR * PW);
    int pr = prem / PW, pc = prem - pr * PW;
    int ih = oh0 + pr - 1, iw = pc - 1;
    bool ok = pp < NPIX && ih >= 0 && ih < H && iw >= 0 && iw < W;
    poff[i] = ok ? (((img + il) * p.g.H + (ih >> ups)) * p.g.W + (iw >> ups)) * p.g.ldx + q4 : 0;
    pvalid |= (unsigned)ok << i;
  }
  f32x4 rp[PSLOTS];
  auto commit_patch = [&]() {
#pragma unroll
    for (int i = 0; i < PSLOTS; ++i) {
      int j = tid + NTHREADS * i;
      if (j < NPIX * 8) *reinterpret_cast<f32x4*>(patch + (j >> 3) * PLD + (j & 7) * 4) = rp[i];
    }
  };

  // A lean weight stream instead of the generic loaders.  Every non-MFMA instruction of the K step costs MFMA issue
  // time (tools/micro/mfma_loop_model.hip: 64 full-rate VALU per step = 3.5 %), and the generic loader spent ~9 VALU + a
  // readfirstlane per DMA slot on validity selects and address rebuilds.  Here a slot's row pointer is fixed per tile
  // (rows beyond N are clamped to N - 1: they only feed output columns the epilogue never stores; K is a multiple of 32,
  // so there is no K tail), the K offset of a step is one wave-uniform scalar added per slot, and the LDS destination is
  // scalar arithmetic on the wave index.
  // Data gradient: the weights W[co][tap][ci] stream as [k = co of the chunk][n = ci] rows of one tap: slot pointer =
  // W + (co_local * 9) * Cin + ci quad (quads beyond Cin clamped), step offset = ((chunk * 32) * 9 + tap) * Cin.
  constexpr int NSB = BL::NS;
  const float* bsrc[NSB];
  if (!DG) {
#pragma unroll
    for (int q = 0; q < NSB; ++q) {
      int n = col0 + (tid >> 3) + 32 * q;
      n = n < p.N ? n : p.N - 1;
      bsrc[q] = p.B + (long)n * p.ldb + KCSlots<BN>::kq4();
    }
  } else {
    int c0 = col0 + MCSlots<BN>::rq4();
    c0 = c0 < p.N ? c0 : p.N - 4;
#pragma unroll
    for (int q = 0; q < NSB; ++q) bsrc[q] = p.B + (long)MCSlots<BN>::krow(q) * 9 * p.N + c0;
  }
  auto b_offset = [&](int tp, int ch) -> long {               // wave-uniform: where the K step (tap tp, chunk ch) starts
    return DG ? ((long)ch * BK * 9 + tp) * p.N : (long)tp * C + ch * BK;
  };
  const int wv = wave_id();
  auto stream_b = [&](int q, long off, float* tile) {         // slot q of the K step at offset off -> tile
    float* dst = BL::KC ? tile + (wv * 8 + 32 * q) * BK : tile + (wv * (MCSlots<BN>::KSTEP / 4) + MCSlots<BN>::KSTEP * q) * BN;
    glds16(DG ? bsrc[q] + off : bsrc[q] + (int)off, dst);
  };

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  int abase[TM];
#pragma unroll
  for (int i = 0; i < TM; ++i) {
    int m = wm * (BM / WM) + i * 32 + l31;
    abase[i] = ((m / (TR * W)) * (PR * PW) + ((m / W) % TR) * PW + (m % W)) * PLD + 4 * h;
  }

  // prologue: patch of the first chunk and the weights of step 0
#pragma unroll
  for (int q = 0; q < NSB; ++q) stream_b(q, b_offset(0, c_begin), btile0);
#pragma unroll
  for (int i = 0; i < PSLOTS; ++i) rp[i] = ldg4(sel_src(p.A, (long)poff[i] + c_begin * BK, (pvalid >> i) & 1u));
  commit_patch();
  barrier_after_dma();

  const int nsteps = (c_end - c_begin) * 9;
  int chunk = c_begin, tap = 0;
  for (int st = 0; st < nsteps; ++st) {
    const float* lb = btile0 + (st & 1) * B_TILE;
    float* nb = btile0 + ((st + 1) & 1) * B_TILE;
    int ntap = tap + 1, nchunk = chunk;
    if (ntap == 9) { ntap = 0; ++nchunk; }
    const bool more = st + 1 < nsteps;           // nothing is staged after the last step
    const long onext = b_offset(ntap, nchunk);
    const int cnext = chunk + 1 < c_end ? chunk + 1 : chunk;
#pragma unroll
    for (int i = 0; i < PSLOTS; ++i)      // tap is workgroup-uniform: one float4 of the next chunk's patch per tap
      if (tap == i) rp[i] = ldg4(sel_src(p.A, (long)poff[i] + cnext * BK, (pvalid >> i) & 1u));
    const int r = tap / 3, s3 = tap - r * 3;
    const float* pa = patch + (DG ? (2 - r) * PW + (2 - s3) : r * PW + s3) * PLD;
    f32x4 fa[2][TM], fb[2][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i) fa[0][i] = *reinterpret_cast<const f32x4*>(pa + abase[i]);
#pragma unroll
    for (int j = 0; j < TN; ++j) fb[0][j] = read_frag<BL::KC, BN>(lb, wn * (BN / WN) + j * 32 + l31, 0, h);
#pragma unroll
    for (int g = 0; g < 4; ++g) {
#pragma unroll
      for (int s = 0; s < 4; ++s) {
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[g & 1][i][s], fb[g & 1][j][s], acc[i][j], 0, 0, 0);
        if (g * 4 + s < NSB && more) stream_b(g * 4 + s, onext, nb);
        if (s == 1 && g < 3) {
#pragma unroll
          for (int i = 0; i < TM; ++i) fa[(g + 1) & 1][i] = *reinterpret_cast<const f32x4*>(pa + abase[i] + 8 * (g + 1));
#pragma unroll
          for (int j = 0; j < TN; ++j) fb[(g + 1) & 1][j] = read_frag<BL::KC, BN>(lb, wn * (BN / WN) + j * 32 + l31, g + 1, h);
        }
#pragma unroll
        for (int q = 0; q < TM * TN; ++q) {
          __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
          __builtin_amdgcn_sched_group_barrier(0x002, 7, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    barrier_after_dma();            // weights of step st+1 landed; every wave is done with this tap's reads
    if (tap == 8) {             // chunk boundary: swap in the prefetched patch
      commit_patch();
      __syncthreads();
    }
    tap = ntap;
    chunk = nchunk;
  }

  const bool direct = p.splitk == 1;          // partial sums of a split go to the workspace; splitk_reduce_kernel finishes
  float* Cp = direct ? p.C : p.ws + (long)split * p.M * p.N;
  const float* R = direct ? p.residual : nullptr;
  const int ldc = direct ? p.ldc : p.N;
  store_block<TM, TN, BM, BN, WM, WN>(p, acc, row0, col0, wm, wn, h, l31, Cp, ldc, R, direct, lds + wave * EPI_WAVE);
}

// ------------------------------------------------------------------------------------
// Weight gradient of the 3x3 / stride 1 / pad 1 convolution from an LDS patch:
//   dW[co][tap][ci] = sum_pixels dy[pix][co] * x[pix + tap shift][ci]
// A workgroup owns 128 output channels x one 32-channel input chunk x ALL nine taps (a 128 x 288 slab of dW, 9
// accumulator tiles per wave) and a range of pixels.  A K step is 32 consecutive pixels (one row at W = 32, two rows at
// W = 16, four at W = 8 - always inside one image): the dy tile [32 px][128 co] and the halo'd x rows [(rows+2)(W+2) px][32 ci] arrive by LDS-DMA; the nine taps
// read their B fragments (lane = ci, the two lane halves = two adjacent pixels) from the same patch rows at shifted
// pixel offsets, and one dy fragment (lane = co) feeds nine MFMAs.  Per 2.36 MFLOP the step stages 29 KB (the im2col
// kernel: 32 KB per 1.05 MFLOP) and computes no im2col addresses.  Partial slabs of the pixel splits go to the
// workspace and through splitk_reduce_kernel, as for the generic split-K.
// ------------------------------------------------------------------------------------
// Output-channel tiles.  BM = 128: wave w owns channels [32 w, 32 w + 32) and all nine taps (9 accumulator tiles).
// BM = 96 (the pruned widths 96 / 192 that unlearn.py:363-367 fine-tunes, CelebA's 672), 64, 32 (the tail of 160 = 128 + 32):
// a 128-channel tile would leave waves idle, so the BM / 32 channel groups x 9 taps (group, tap) units are dealt evenly to
// the four waves - 27 units as 7 / 7 / 7 / 6, 18 as 5 / 5 / 4 / 4, 9 as 3 / 2 / 2 / 2 -, consecutive units per wave, which
// touch at most two channel groups and never repeat a tap.  Which accumulator meets which fragment must be static, so the
// K loop is instantiated per wave (WAVE = 0..3; -1 = the BM = 128 form, wave at run time).
template <int BM, int WAVE>
struct WgradUnits {
  static constexpr int NU = BM / 32 * 9;                                       // (channel group, tap) units of the tile
  static constexpr int U0 = BM == 128 ? 0 : WAVE * (NU / 4) + (WAVE < NU % 4 ? WAVE : NU % 4);
  static constexpr int N = BM == 128 ? 9 : NU / 4 + (WAVE < NU % 4 ? 1 : 0);  // 96: 7 7 7 6;  64: 5 5 4 4;  32: 3 2 2 2
  static constexpr int CG0 = BM == 128 ? 0 : U0 / 9;                          // BM = 128: + wave at run time
  static constexpr bool TWO = BM != 128 && (U0 + N - 1) / 9 != CG0;            // the units span two channel groups
  static constexpr int tap(int i) { return BM == 128 ? i : (U0 + i) % 9; }
  static constexpr int grp(int i) { return BM == 128 ? 0 : (U0 + i) / 9 - CG0; }
};

template <int W, int BM, int WAVE>
__device__ __forceinline__ void wgrad_patch_body(const DevArgs& p, float* lds) {
  using U = WgradUnits<BM, WAVE>;
  // a K step is 32 consecutive pixels: WS = min(W, 32) columns of ROWS = 32 / WS image rows (W = 64: half a row - the
  // step's first column `seg` alternates 0 / 32 and the halo columns seg - 1, seg + 32 come from the same row)
  constexpr int WS = W < BK ? W : BK, ROWS = BK / WS;
  constexpr int PW = WS + 2, PRW = ROWS + 2, NPX = PRW * PW;
  constexpr int PSL = (NPX * 8 + NTHREADS - 1) / NTHREADS;      // DMA slots per thread for the patch
  constexpr int PSIZE = PSL * 32 * BK;                            // floats (whole wave-instructions)
  constexpr int A_TILE = BK * BM;
  constexpr int ANS = BM / 32;                    // dy-tile DMA pieces (1 KiB each) per wave
  static_assert(ANS + PSL <= 16, "one DMA slot per pixel pair");

  // block -> (pixel split, co tile, ci chunk); chunks of one (split, co tile) are adjacent: they share the dy tiles in L2
  const int nci = p.g.C / BK;
  int bid = blockIdx.x;
  const int cchunk = bid % nci;
  bid /= nci;
  const int tile_m = bid % p.tiles_m, split = bid / p.tiles_m;
  const int row0 = tile_m * BM, ci0 = cchunk * BK;
  const int HW = p.g.Ho * p.g.Wo, ups = p.g.upsample;
  const int kt0 = split * p.ktiles_per_split;
  const int kend = min(p.K, (kt0 + p.ktiles_per_split) * BK);
  const int nkt = (kend - kt0 * BK + BK - 1) / BK;

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, h = lane >> 5, l31 = lane & 31;
  const int cg0 = BM == 128 ? wave : U::CG0;      // first channel group of this wave's units

  // patch slots: slot i covers patch pixel i*32 + tid/8, float4 tid%8
  int prow[PSL], pcol[PSL];
#pragma unroll
  for (int i = 0; i < PSL; ++i) {
    int px = i * 32 + (tid >> 3);
    prow[i] = px < NPX ? px / PW : -100000;      // rows far outside -> always invalid
    pcol[i] = px % PW - 1;
  }
  auto patch_src = [&](int i, int k0) -> const float* {
    int img = k0 / HW, rem = k0 - img * HW;
    int ih = rem / W - 1 + prow[i], iw = (W > WS ? rem % W : 0) + pcol[i];
    bool ok = k0 < kend && ih >= 0 && ih < p.g.Ho && iw >= 0 && iw < W;
    long off = ((long)(img * p.g.H + (ih >> ups)) * p.g.W + (iw >> ups)) * p.g.ldx + ci0 + (tid & 7) * 4;
    return sel_src(p.B, off, ok);
  };
  // Lean staging (see LeanKC above: every VALU instruction of the K step costs MFMA issue time; the general form spent ~200
  // per step here, most of it on k0 / HW and rem / W per patch slot).  dy: the [32 px][BM co] tile is BM / 32 pieces of
  // 1 KiB per wave; piece (wave + 4 i) covers float4s 64 (wave + 4 i) .. + 63 of the image, i.e. pixel f4 / (BM / 4),
  // channel quad f4 % (BM / 4) - fixed per lane (channel quads beyond M clamped) plus one wave-uniform k offset.  x: a K
  // step is ROWS whole rows of ONE image, so (image, first row) advance as scalars from step to step and a slot's address
  // is a per-slot constant plus one uniform row offset; only the halo test (row inside the image) is per slot and step.
  // The fused-upsample geometry keeps the general form.
  const int wv = wave_id();
  const float* aptr[ANS];
#pragma unroll
  for (int i = 0; i < ANS; ++i) {
    const int f4 = (wave + 4 * i) * 64 + lane;
    const int px = f4 / (BM / 4);
    int c0 = row0 + (f4 - px * (BM / 4)) * 4;
    c0 = c0 < p.M ? c0 : p.M - 4;
    aptr[i] = p.A + (long)px * p.lda + c0;
  }
  int xoff[PSL];               // (prow * W + pcol) * ldx + ci0 + float4 column: the slot's offset from the step's row base
  unsigned colok = 0;          // slot's column inside the image (and the slot exists)
#pragma unroll
  for (int i = 0; i < PSL; ++i) {
    xoff[i] = prow[i] >= 0 ? (prow[i] * W + pcol[i]) * p.g.ldx + ci0 + (tid & 7) * 4 : 0;
    colok |= (unsigned)(prow[i] >= 0 && pcol[i] >= 0 && pcol[i] < W) << i;
  }
  auto stage = [&](int piece, int k0, int img, int oh, int seg, float* ta, float* tp) {
    if (piece < ANS) {
      glds16(aptr[piece] + (long)k0 * p.lda, ta + (wv + 4 * piece) * 256);
    } else if (piece < ANS + PSL) {
      const int i = piece - ANS;
      float* dst = tp + (i * 32 + wv * 8) * BK;
      if (ups) {
        glds16(patch_src(i, k0), dst);
      } else {
        const int ih = oh - 1 + prow[i];
        bool ok = ((colok >> i) & 1u) && ih >= 0 && ih < p.g.Ho;
        if (W > WS) ok = prow[i] >= 0 && ih >= 0 && ih < p.g.Ho && seg + pcol[i] >= 0 && seg + pcol[i] < W;
        const long rowbase = (((long)img * p.g.H + (oh - 1)) * W + seg) * p.g.ldx;     // wave-uniform
        glds16(sel_src(p.B, rowbase + xoff[i], ok), dst);
      }
    }
  };

  f32x16 acc[U::N];
#pragma unroll
  for (int t = 0; t < U::N; ++t)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[t][e] = 0.f;

  int img = (kt0 * BK) / HW, oh = ((kt0 * BK) - img * HW) / W;      // the first step's image and first row (scalars)
  int seg = W > WS ? ((kt0 * BK) - img * HW) % W : 0;              // ... and first column
  if (nkt > 0) {
#pragma unroll
    for (int q = 0; q < ANS + PSL; ++q) stage(q, kt0 * BK, img, oh, seg, lds, lds + A_TILE);
  }
  barrier_after_dma();

  // fragment bases: A[(2j + h)][32 cg + l31]; B: pixel q = 2j + h -> patch pixel (q / W) * PW + q % W (+ tap shift)
  for (int kt = 0; kt < nkt; ++kt) {
    const float* la = lds + (kt & 1) * (A_TILE + PSIZE);
    const float* lp = la + A_TILE;
    float* na = lds + ((kt + 1) & 1) * (A_TILE + PSIZE);
    const bool more = kt + 1 < nkt;                                  // nothing is staged after the last step
    const int knext = (kt0 + kt + 1) * BK;
    int nimg = img, noh = oh + ROWS, nseg = 0;
    if (W > WS) {
      nseg = seg + WS;
      noh = oh;
      if (nseg >= W) { nseg = 0; noh = oh + 1; }
    }
    if (noh >= p.g.Ho) { noh = 0; ++nimg; }
    float fa[2][2], fb[2][U::N];
    auto load_frags = [&](int j, int buf) {
      const int q = 2 * j + h;
      fa[buf][0] = la[q * BM + cg0 * 32 + l31];
      if (U::TWO) fa[buf][1] = la[q * BM + cg0 * 32 + 32 + l31];
      const float* pb = lp + ((q / WS) * PW + (q % WS)) * BK + l31;
#pragma unroll
      for (int t = 0; t < U::N; ++t) fb[buf][t] = pb[((U::tap(t) / 3) * PW + (U::tap(t) % 3)) * BK];
    };
    load_frags(0, 0);
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      if (j + 1 < 16) load_frags(j + 1, (j + 1) & 1);
#pragma unroll
      for (int t = 0; t < U::N; ++t)
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[j & 1][U::grp(t)], fb[j & 1][t], acc[t], 0, 0, 0);
      if (more) stage(j, knext, nimg, noh, nseg, na, na + A_TILE);     // one DMA slot per pixel pair (ANS + PSL <= 16)
    }
    img = nimg;
    oh = noh;
    seg = nseg;
    barrier_after_dma();
  }

  // epilogue: D row = co (32 cg + (e&3) + 8(e>>2) + 4h), D col = ci (l31); N index = tap * C + ci0 + ci
  const bool direct = p.splitk == 1;
  float* Cp = direct ? p.C : p.ws + (long)split * p.M * p.N;
  const int ldc = direct ? p.ldc : p.N;
#pragma unroll
  for (int t = 0; t < U::N; ++t) {
    const int n = U::tap(t) * p.g.C + ci0 + l31;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      int m = row0 + (cg0 + U::grp(t)) * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
      if (m < p.M) Cp[(long)m * ldc + n] = direct ? acc[t][e] * p.alpha : acc[t][e];
    }
  }
}

template <int W, int BM = 128>
__global__ __launch_bounds__(NTHREADS, 2) void wgrad3x3_patch_f32_kernel(const DevArgs p) {   // 2 waves / SIMD: <= 256 registers
  constexpr int WS = W < BK ? W : BK, ROWS = BK / WS, NPX = (ROWS + 2) * (WS + 2), PSL = (NPX * 8 + NTHREADS - 1) / NTHREADS;
  __shared__ __attribute__((aligned(16))) float lds[2 * (BK * BM + PSL * 32 * BK)];
  if (BM == 128) {
    wgrad_patch_body<W, BM, -1>(p, lds);
  } else {                                        // every instance runs the same barriers: one per K step
    switch (wave_id()) {
      case 0: wgrad_patch_body<W, BM, 0>(p, lds); break;
      case 1: wgrad_patch_body<W, BM, 1>(p, lds); break;
      case 2: wgrad_patch_body<W, BM, 2>(p, lds); break;
      default: wgrad_patch_body<W, BM, 3>(p, lds); break;
    }
  }
}

// ------------------------------------------------------------------------------------
// 3x3 / stride 1 / pad 1 convolution with FEW output channels (conv_out of the U-Nets: 128 -> 3, 224 -> 3, 320 -> 4).
// On the MFMA kernels such a launch is >= 90 % padding (N = 3 in a 64-wide tile: 5 TF/s, 13x its HBM time); its
// arithmetic (9 C N FMAs per pixel) fits the vector ALUs inside the time HBM needs to deliver the input once.  So: a
// workgroup = 256 consecutive pixels (whole rows of one image), one thread per pixel; the halo'd input patch of a
// 32-channel chunk lives in LDS exactly as in conv3x3_patch_f32_kernel (144-B pixel stride, next chunk prefetched
// into registers); the weights are workgroup-uniform, so they arrive through the SCALAR cache as SGPR operands of the
// FMAs (no LDS, no vector loads); a thread accumulates its pixel's NOUT outputs over all taps and channels
// (channel-sequential within a chunk, chunk-major: a fixed order) and writes bias + alpha * sum.
// ------------------------------------------------------------------------------------
template <int W, int NOUT>
__global__ __launch_bounds__(NTHREADS) void conv3x3_fewout_kernel(const DevArgs p) {
  constexpr int TP = NTHREADS, TR = TP / W, PW = W + 2, PR = TR + 2, NPIX = PR * PW;
  constexpr int PSL = (NPIX * 8 + NTHREADS - 1) / NTHREADS;
  __shared__ __attribute__((aligned(16))) float patch[NPIX * PLD];

  const int row0 = blockIdx.x * TP;
  const int H = p.g.Ho, C = p.g.C;
  const int img = row0 / (H * W), oh0 = (row0 - img * (H * W)) / W;
  const int tid = threadIdx.x;

  int poff[PSL];
  unsigned pvalid = 0;
#pragma unroll
  for (int i = 0; i < PSL; ++i) {
    int j = tid + NTHREADS * i;
    int pp = j >> 3, q4 = (j & 7) * 4;
    int pr = pp / PW, pc = pp - pr * PW;
    int ih = oh0 + pr - 1, iw = pc - 1;
    bool ok = pp < NPIX && ih >= 0 && ih < H && iw >= 0 && iw < W;
    poff[i] = ok ? ((img * p.g.H + ih) * p.g.W + iw) * p.g.ldx + q4 : 0;
    pvalid |= (unsigned)ok << i;
  }
  f32x4 rp[PSL];
  auto fetch = [&](int chunk) {
#pragma unroll
    for (int i = 0; i < PSL; ++i) rp[i] = ldg4(sel_src(p.A, (long)poff[i] + chunk * BK, (pvalid >> i) & 1u));
  };
  auto commit = [&]() {
#pragma unroll
    for (int i = 0; i < PSL; ++i) {
      int j = tid + NTHREADS * i;
      if (j < NPIX * 8) *reinterpret_cast<f32x4*>(patch + (j >> 3) * PLD + (j & 7) * 4) = rp[i];
    }
  };

  f32x2 acc[NOUT];
#pragma unroll
  for (int n = 0; n < NOUT; ++n) acc[n] = f32x2{0.f, 0.f};
  const float* px0 = patch + ((tid / W) * PW + (tid % W)) * PLD;

  const int nchunks = C / BK;
  fetch(0);
  commit();
  __syncthreads();
  for (int chunk = 0; chunk < nchunks; ++chunk) {
    if (chunk + 1 < nchunks) fetch(chunk + 1);
    const float* wc = p.B + chunk * BK;                  // B[n][tap][c]: workgroup-uniform addresses -> scalar loads
#pragma unroll 1
    for (int tap = 0; tap < 9; ++tap) {
      const float* px = px0 + ((tap / 3) * PW + (tap % 3)) * PLD;
      const float* wt = wc + tap * C;
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const f32x4 x = *reinterpret_cast<const f32x4*>(px + 4 * q);
#pragma unroll
        for (int n = 0; n < NOUT; ++n) {
          const float* w = wt + (long)n * p.ldb + 4 * q;
          acc[n] = f32x2{x[0], x[1]} * f32x2{w[0], w[1]} + acc[n];
          acc[n] = f32x2{x[2], x[3]} * f32x2{w[2], w[3]} + acc[n];
        }
      }
    }
    __syncthreads();                                     // every thread is done with this chunk's patch
    if (chunk + 1 < nchunks) {
      commit();
      __syncthreads();
    }
  }
  const int m = row0 + tid;
  if (m < p.M) {
#pragma unroll
    for (int n = 0; n < NOUT; ++n)
      if (n < p.N) p.C[(long)m * p.ldc + n] = __builtin_fmaf(acc[n][0] + acc[n][1], p.alpha, p.bias ? p.bias[n] : 0.f);
  }
}

// split-K: C = epilogue(sum_s ws[z][s][m][n])
__global__ void splitk_reduce_kernel(const DevArgs p, int batch) {
  const long mn = (long)p.M * p.N;
  if (p.epi_vec) {
    // float4 form (every tensor involved is 16-byte addressable at columns that are multiples of 4; N % 4 == 0): the
    // same per-element sums in the same order as the scalar form below
    const long total4 = (long)batch * mn / 4;
    for (long i4 = (long)blockIdx.x * blockDim.x + threadIdx.x; i4 < total4; i4 += (long)gridDim.x * blockDim.x) {
      const long idx = i4 * 4;
      int z = 0;
      long r = idx;
      if (batch > 1) { z = (int)(idx / mn); r = idx - (long)z * mn; }
      const int m = mn < (1L << 31) ? (int)((unsigned)r / (unsigned)p.N) : (int)(r / p.N);
      const int n = (int)(r - (long)m * p.N);
      const float* w = p.ws + (long)z * p.splitk * mn + r;
      f32x4 v = zero4();
      for (int s = 0; s < p.splitk; ++s) v += ldg4(w + (long)s * mn);
      const f32x4 b = p.bias ? ldg4(p.bias + n) : zero4();
      v = f32x4{__builtin_fmaf(v[0], p.alpha, b[0]), __builtin_fmaf(v[1], p.alpha, b[1]), __builtin_fmaf(v[2], p.alpha, b[2]),
                __builtin_fmaf(v[3], p.alpha, b[3])};
      if (p.rowadd) v += ldg4(p.rowadd + (long)p.fdRpg.div(m) * p.ld_rowadd + n);
      const int z0 = z / p.batch_inner, z1 = z - z0 * p.batch_inner;
      const long coff = z0 * p.sC0 + z1 * p.sC1;
      if (p.residual) v += ldg4(p.residual + coff + (long)m * p.ldr + n);
      *reinterpret_cast<f32x4*>(p.C + coff + (long)m * p.ldc + n) = v;
    }
    return;
  }
  long total = (long)batch * mn;
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
    int z = (int)(idx / mn);
    long r = idx - (long)z * mn;
    int m = (int)(r / p.N), n = (int)(r - (long)m * p.N);
    const float* w = p.ws + (long)z * p.splitk * mn + r;
    float v = 0.f;
    for (int s = 0; s < p.splitk; ++s) v += w[(long)s * mn];
    v = __builtin_fmaf(v, p.alpha, p.bias ? p.bias[n] : 0.f);
    if (p.rowadd) v += p.rowadd[(long)(m / p.rows_per_group) * p.ld_rowadd + n];
    int z0 = z / p.batch_inner, z1 = z - z0 * p.batch_inner;
    long coff = z0 * p.sC0 + z1 * p.sC1;
    if (p.residual) v += p.residual[coff + (long)m * p.ldr + n];
    p.C[coff + (long)m * p.ldc + n] = v;
  }
}

static void launch_splitk_reduce(const DevArgs& d, int batch, hipStream_t st) {
  const long items = (long)batch * d.M * d.N / (d.epi_vec ? 4 : 1);
  const int blocks = (int)(gad_ceil_div(items, 256) < 2048 ? gad_ceil_div(items, 256) : 2048);
  hipLaunchKernelGGL(splitk_reduce_kernel, dim3(blocks > 0 ? blocks : 1), dim3(256), 0, st, d, batch);
}

static int pick_vec(const gad_gemm_args* a) {
  int vec = 4;
  const int am = a->a_mode, bmode = a->b_mode;
  if (am == GAD_A_KC && (a->K % 4 != 0 || a->lda % 4 != 0)) vec = 1;
  if (am == GAD_A_MC && (a->M % 4 != 0 || a->lda % 4 != 0)) vec = 1;
  if (bmode == GAD_B_KC && (a->K % 4 != 0 || a->ldb % 4 != 0)) vec = 1;
  if (bmode == GAD_B_MC && (a->N % 4 != 0 || a->ldb % 4 != 0)) vec = 1;
  if ((am == GAD_A_CONV || am == GAD_A_CONVT || bmode == GAD_B_CONV) && (a->g.C % 4 != 0 || a->g.ldx % 4 != 0)) vec = 1;
  // batched launches: slab z starts at A + z0 * strideA0 + z1 * strideA1 (B likewise), which must stay on the float4 grid too
  if (a->batch > 1 && (a->strideA0 % 4 != 0 || a->strideA1 % 4 != 0 || a->strideB0 % 4 != 0 || a->strideB1 % 4 != 0)) vec = 1;
  return vec;
}

// tile_hint values that force a route or a tile (A/B tools, tests; 0 = the planner decides): include/gad.h
enum : int32_t {
  HINT_128 = 1,              // engine: 128 x 128 tiles; patch weight gradient: 128-channel tiles
  HINT_64 = 2,               // engine: 64 x 64 tiles (keeps the LDS-patch kernels out)
  HINT_128x64 = 3,           // engine: 128 x 64 tiles (dense fp32 forms)
  HINT_WGRAD_96 = 4, HINT_WGRAD_64 = 5, HINT_WGRAD_32 = 6,   // patch weight gradient on 96 / 64 / 32-channel tiles
  HINT_WINO2 = 7,            // Winograd F(2x2)
  HINT_WINO4 = 8,            // Winograd F(4x4), the planner's form; the Winograd weight gradient
  HINT_WINO4_FUSED32 = 9,    // F(4x4) one-launch form on 32-tile blocks
  HINT_WINO4_THREE = 10,     // F(4x4) three-launch forms
  HINT_WINO4_FUSED64 = 11,   // F(4x4) one-launch form on 64-tile blocks
  HINT_SPLIT_M = 1000,       // + m1: patch weight gradient as two launches, rows [0, m1) on 128-channel tiles, the rest planned
};

struct Plan {
  int bm, bn, tiles_m, tiles_n, splitk, ktiles_per_split;
  long nblocks;
};

// Tile / split-K choice by a small analytic cost model (cycles at ~2 GHz), calibrated on the MI355X
// sweep in tools/sweep_conv.py: a CU holds 2 (128x128) or 4 (64x64) workgroups whose waves share each
// SIMD's matrix pipe; one K step costs conc*mfma + X cycles (X = load/barrier time that is not hidden);
// split-K adds a reduction pass over (sk+1)*M*N floats.
static bool dense_128x64_ok(const gad_gemm_args* a) {
  const bool dense = (a->a_mode == GAD_A_KC || a->a_mode == GAD_A_MC) && (a->b_mode == GAD_B_KC || a->b_mode == GAD_B_MC) &&
                     !(a->a_mode == GAD_A_MC && a->b_mode == GAD_B_KC);
  return dense && !a->A2 && pick_vec(a) == 4 && !(a->operand_precision == 1);     // incl. the K-concatenated (LoRA) forms
}
static Plan make_plan(const gad_gemm_args* a) {
  const long batch = a->batch > 0 ? a->batch : 1;
  const int kt = (int)gad_ceil_div(a->K, BK) > 0 ? (int)gad_ceil_div(a->K, BK) : 1;
  static const int sks[] = {1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64, 96, 128};
  double best = 1e30;
  Plan pl{};
  for (int bm = 128; bm >= 64; bm -= 64) {
    if (a->tile_hint == HINT_128 && bm != 128) continue;
    if (a->tile_hint == HINT_64 && bm != 64) continue;
    // bf16-operand kernels: 3 / 6 workgroups per CU; a K step is bound by staging (gather + convert + LDS), not by
    // the 8 / 2 MFMAs, so the per-step cost of a 64x64 tile is about a third of a 128x128 tile's, not a quarter
    const bool bf = a->operand_precision == 1 && pick_vec(a) == 4;
    const int cap = bf ? (bm == 128 ? 3 : 6) : (bm == 128 ? 2 : 4);
    const double mfma = bf ? (bm == 128 ? 1200.0 : 420.0) : (bm == 128 ? 4096.0 : 1100.0);
    const double X = bf ? (bm == 128 ? 600.0 : 300.0) : (bm == 128 ? 1200.0 : 600.0);
    const double fixed = bf ? (bm == 128 ? 4000.0 : 2000.0) : (bm == 128 ? 6000.0 : 3000.0);
    const long tiles = gad_ceil_div(a->M, bm) * gad_ceil_div(a->N, bm) * batch;
    for (int sk : sks) {
      if (a->splitk_hint > 0) sk = a->splitk_hint < kt ? a->splitk_hint : kt;
      else if (sk > 1 && sk > kt / 4) break;
      const int per = (int)gad_ceil_div(kt, sk);
      const int sk_eff = (int)gad_ceil_div(kt, per);
      const long blocks = tiles * sk_eff;
      const long slots = 256L * cap;
      const long rounds = gad_ceil_div(blocks, slots);
      double occ = (double)(blocks - (rounds - 1) * slots) / 256.0;
      double conc = occ < 1.0 ? 1.0 : (occ > cap ? cap : occ);
      conc = (double)(long)(conc + 0.999);
      double cyc = per * ((rounds - 1) * (cap * mfma + X) + (conc * mfma + X)) + rounds * fixed;
      double us = cyc / 2000.0;
      if (sk_eff > 1) us += 4.0 + (double)batch * a->M * a->N * 4.0 * (sk_eff + 1) / 3.0e6;
      // Short-K launches are not compute-bound: every round moves its operand / residual / output bytes through HBM and
      // only part of that overlaps the few K steps of a tile.  Measured on the attention projections (tools/ab_linear.py,
      // K = 256 and 512): the exposed share is ~1.4 x (8 / steps) of the launch's HBM time with 2 workgroups per CU and
      // ~0.4 x (8 / steps) with 4 (64x64 tiles) - which is what makes the small tile win there.
      {
        const bool convA_ = a->a_mode == GAD_A_CONV || a->a_mode == GAD_A_CONVT;
        const double a_el = convA_ ? (double)(a->M / (a->g.Ho * a->g.Wo > 0 ? a->g.Ho * a->g.Wo : 1)) * a->g.H * a->g.W * a->g.C
                                   : (double)a->M * a->K;
        const double b_el = a->b_mode == GAD_B_CONV ? (double)(a->K / (a->g.Ho * a->g.Wo > 0 ? a->g.Ho * a->g.Wo : 1)) * a->g.H * a->g.W * a->g.C
                                                    : (double)a->N * a->K;
        const double bytes = 4.0 * batch * (a_el + b_el + (double)a->M * a->N * (a->residual ? 2.0 : 1.0));
        double ratio = 8.0 / per;
        if (ratio > 2.0) ratio = 2.0;
        us += bytes / 4.0e6 * (bm == 128 ? 1.4 : 0.4) * ratio;
      }
      if (us < best) {
        best = us;
        pl.bm = bm;
        pl.bn = bm;
        pl.tiles_m = (int)gad_ceil_div(a->M, bm);
        pl.tiles_n = (int)gad_ceil_div(a->N, bm);
        pl.splitk = sk_eff;
        pl.ktiles_per_split = per;
        pl.nblocks = blocks;
      }
      if (a->splitk_hint > 0) break;
    }
  }
  // 128 x 64 tiles (3 workgroups per CU, 1.5x the FLOPs per staged byte of 64 x 64, no padding for N = 320 / 640 / 192):
  // where the model above prefers 64 x 64 without a split and there are rows enough for > 1 round of them, this shape
  // measured +3..7 % on the forward / data-gradient forms (tools/sweep_gemm.py, profiles/r02_sd_gemm_tile_sweep.txt)
  const bool auto_128x64 = a->tile_hint == 0 && a->splitk_hint <= 0 && pl.bm == 64 && pl.splitk == 1 && batch == 1 &&
                           a->M >= 16384 && a->a_mode == GAD_A_KC;
  // ... and where N is a whole number of 128-wide tiles and the launch is many rounds deep, the 128 x 128 tile measured another
  // 3-9 % faster (attention projections / 1x1 shortcuts of the CIFAR sampler at B = 1024: tools/ab_dense_tiles.py,
  // profiles/r04_ab_dense_tiles.txt) - N = 320 / 640 (SD) keep 128 x 64, which pads nothing there
  auto whole_k = [&](int bn) {                 // 128 x bn tiles, no split
    pl.bm = 128; pl.bn = bn;
    pl.tiles_m = (int)gad_ceil_div(a->M, 128);
    pl.tiles_n = (int)gad_ceil_div(a->N, bn);
    pl.splitk = 1;
    pl.ktiles_per_split = kt;
    pl.nblocks = (long)pl.tiles_m * pl.tiles_n * batch;
    return pl;
  };
  if (auto_128x64 && a->N % 128 == 0 && (long)gad_ceil_div(a->M, 128) * (a->N / 128) >= 1024) return whole_k(128);
  if ((a->tile_hint == HINT_128x64 || auto_128x64) && dense_128x64_ok(a)) return whole_k(64);
  return pl;
}

template <int AM, int BMODE, int VEC, int TAG = 0>
static void launch_mode(const DevArgs& d, const Plan& pl, hipStream_t st) {
  dim3 grid((unsigned)pl.nblocks), block(NTHREADS);
  if (pl.bm == 128 && pl.bn == 64) {
    if constexpr (VEC == 4 && (((AM == GAD_A_KC || AM == GAD_A_MC) && (BMODE == GAD_B_KC || BMODE == GAD_B_MC) &&
                                !(AM == GAD_A_MC && BMODE == GAD_B_KC)) ||
                               (AM == A_KC2 && (BMODE == B_KC2 || BMODE == B_MC2)) ||
                               (AM == A_KC_L && (BMODE == B_KC_L || BMODE == B_MC_L)) || (AM == A_MC_L && BMODE == B_MC_L) ||
                               (AM == A_KC2_L && (BMODE == B_KC2_L || BMODE == B_MC2_L))))
      hipLaunchKernelGGL((gemm_kernel<AM, BMODE, 128, 64, VEC, TAG>), grid, block, 0, st, d);
  } else if (pl.bm == 128)
    hipLaunchKernelGGL((gemm_kernel<AM, BMODE, 128, 128, VEC, TAG>), grid, block, 0, st, d);
  else
    hipLaunchKernelGGL((gemm_kernel<AM, BMODE, 64, 64, VEC, TAG>), grid, block, 0, st, d);
}

template <int AM, int BMODE>
static void launch_bf16(const DevArgs& d, const Plan& pl, hipStream_t st) {
  dim3 grid((unsigned)pl.nblocks), block(NTHREADS);
  if (pl.bm == 128)
    hipLaunchKernelGGL((gemm_bf16_kernel<AM, BMODE, 128, 128>), grid, block, 0, st, d);
  else
    hipLaunchKernelGGL((gemm_bf16_kernel<AM, BMODE, 64, 64>), grid, block, 0, st, d);
}

}  // namespace


// bf16 operands are used when the caller allows them and a bf16 instance exists for the operand pair
static bool use_bf16(const gad_gemm_args* a) {
  return a->operand_precision == 1 && pick_vec(a) == 4;
}

// 3x3 / stride 1 / pad 1 with output maps the size of the (upsampled) input: the geometry of the patch and Winograd kernels
static bool same_3x3(const gad_conv_geom& g) {
  return g.KH == 3 && g.KW == 3 && g.stride == 1 && g.pad_t == 1 && g.pad_l == 1 && g.Ho == (g.upsample ? 2 * g.H : g.H) &&
         g.Wo == (g.upsample ? 2 * g.W : g.W);
}

// 3x3 / stride 1 / pad 1 forward conv whose 128-pixel tiles are whole rows of one image: the LDS-patch kernel applies
static bool patch_conv_geom(const gad_gemm_args* a, bool dgrad = false) {
  const gad_conv_geom& g = a->g;
  const bool modes = dgrad ? (a->a_mode == GAD_A_CONVT && a->b_mode == GAD_B_WDGRAD && !g.upsample)
                           : (a->a_mode == GAD_A_CONV && a->b_mode == GAD_B_KC);
  return pick_vec(a) == 4 && modes && !a->A2 && same_3x3(g) &&
         (((g.Wo == 64 || g.Wo == 32 || g.Wo == 16) && (g.Ho * g.Wo) % 128 == 0) ||
          ((g.Wo == 8 || g.Wo == 4) && g.Ho == g.Wo && a->M % 128 == 0)) && g.C % BK == 0 && a->tile_hint != HINT_64 && a->splitk_hint <= 1 &&
         (a->batch <= 1) && (long)a->M * g.ldx < (1L << 31) && !(a->flags & GAD_GEMM_NO_PATCH);
}
static bool use_patch_conv(const gad_gemm_args* a) { return use_bf16(a) && patch_conv_geom(a); }
// fp32 patch kernel: its own plan - 128-pixel tiles, split-K over the 32-channel chunks when the tiles alone cannot fill
// the 512 workgroup slots (small maps); launches too small even then stay on the generic kernel
struct PatchPlan {
  int splitk, chunks_per_split, bn;
  long blocks;
};
// Plan of the fp32 patch kernels.  Forward: the output-channel tile is the one of {128, 160, 96} with the least modelled time =
// rounds of 512 resident workgroups x K steps per workgroup x tile width - i.e. padding AND round quantisation count
// (640 channels at 16x16, B = 64: five 128-wide tiles = 640 workgroups = two rounds, four 160-wide tiles = one round).
// Small maps split K over the channel chunks until ~512 workgroups exist.
static void patch_plan_for(const gad_gemm_args* a, int bn, PatchPlan* pp) {
  pp->bn = bn;
  const long tiles = gad_ceil_div(a->M, 128) * gad_ceil_div(a->N, bn);
  const int nchunks = a->g.C / BK;
  pp->chunks_per_split = nchunks;
  pp->splitk = 1;
  pp->blocks = tiles;
  if (tiles < 384) {           // split K: the split count just below or just above one round of workgroups, whichever is faster
    double best = 1e30;
    for (long sk0 = 512 / tiles; sk0 <= gad_ceil_div(512, tiles); ++sk0) {
      long sk = sk0;
      if (sk > nchunks / 2) sk = nchunks / 2;    // >= 2 chunks (18 K steps) per workgroup
      if (sk < 1) sk = 1;
      const int per = (int)gad_ceil_div(nchunks, sk);
      const int ske = (int)gad_ceil_div(nchunks, per);
      const double c = (double)gad_ceil_div(tiles * ske, 512) * per;
      if (c < best) {
        best = c;
        pp->chunks_per_split = per;
        pp->splitk = ske;
        pp->blocks = tiles * ske;
      }
    }
  }
}
static bool use_patch_conv_f32(const gad_gemm_args* a, PatchPlan* pp) {
  if (use_bf16(a) || !(patch_conv_geom(a) || patch_conv_geom(a, true))) return false;
  if (a->N < 64) return false;               // conv_out (3 output channels): a 128-wide tile would be 98 % padding
  patch_plan_for(a, 128, pp);
  if (patch_conv_geom(a)) {                  // forward: three channel-tile widths (the data gradient streams 128 columns)
    auto cost = [](const PatchPlan& q) { return (double)gad_ceil_div(q.blocks, 512) * q.chunks_per_split * q.bn; };
    double best = cost(*pp);
    const int cand[2] = {160, 96};
    for (int bn : cand) {
      PatchPlan q;
      patch_plan_for(a, bn, &q);
      const double c = cost(q);
      if (c < best && q.blocks >= 192) { best = c; *pp = q; }
    }
  }
  return pp->blocks >= 192;
}

// Channel counts that no single tile width divides (CelebA-HQ LDM: 224 = 128 + 96, 448 = 2 x 128 + 2 x 96;
// ddpm_config.py:425-450) run as TWO launches over disjoint column ranges - the first n1 columns on 128-wide tiles, the
// rest on 96-wide tiles - when that models faster than the best padded single launch (128-wide tiles waste an eighth of
// the MFMA work there).  Forward form only (which the data gradients share, ops.dgrad_as_forward), no split-K.
static bool patch_split_n(const gad_gemm_args* a, int* n1_out) {
  if (use_bf16(a) || !patch_conv_geom(a) || a->N % 32 != 0 || a->N < 224 || a->tile_hint != 0) return false;
  PatchPlan single;
  if (!use_patch_conv_f32(a, &single) || single.splitk != 1) return false;
  auto cost = [](const PatchPlan& q) { return (double)gad_ceil_div(q.blocks, 512) * q.chunks_per_split * q.bn; };
  if (gad_ceil_div(a->N, single.bn) * single.bn == a->N) return false;        // already exact
  for (int n2 = 96; n2 < a->N; n2 += 96) {
    const int n1 = a->N - n2;
    if (n1 % 128 != 0) continue;
    gad_gemm_args lo = *a, hi = *a;
    lo.N = n1;
    hi.N = n2;
    PatchPlan pl, ph;
    patch_plan_for(&lo, 128, &pl);
    patch_plan_for(&hi, 96, &ph);
    if (pl.splitk != 1 || ph.splitk != 1 || pl.blocks < 192 || ph.blocks < 192) continue;
    if (cost(pl) + cost(ph) < 0.97 * cost(single)) {
      *n1_out = n1;
      return true;
    }
  }
  return false;
}

// 3x3 / stride 1 / pad 1 forward conv with <= 4 output channels on whole 256-pixel row tiles: the vector-ALU kernel
static bool use_fewout_conv(const gad_gemm_args* a) {
  const gad_conv_geom& g = a->g;
  return a->a_mode == GAD_A_CONV && a->b_mode == GAD_B_KC && a->N <= 4 && !a->A2 && !a->A_k2 && pick_vec(a) == 4 &&
         same_3x3(g) && !g.upsample &&
         (g.W == 64 || g.W == 32 || g.W == 16) && (g.H * g.W) % 256 == 0 && a->M % 256 == 0 && g.C % BK == 0 &&
         a->batch <= 1 && !a->rowadd && !a->residual && a->tile_hint == 0 && a->splitk_hint <= 1 &&
         (long)a->M * g.ldx < (1L << 31) && !(a->flags & GAD_GEMM_NO_PATCH);
}

// 3x3 / stride 1 / pad 1 weight gradient with the LDS-patch kernel: pixel-split count (0 = not eligible) and the
// output-channel tile: 96 / 64 / 32 where 128-channel tiles would idle waves (M = 96, 192, 288; 64; 32), by modelled time.
// Modelled time of ONE weight-gradient patch launch over M output channels on bm-channel tiles, calibrated on
// tools/ab_wgrad_tiles.py (profiles/r03_ab_wgrad_tiles.txt: within ~3 % of the measured ratios): rounds of 512 resident
// workgroups x (K steps per workgroup + 3 steps' worth of prologue / epilogue) x the tile's cost per step - accumulator units
// of the busiest wave, the dealt forms (96 / 64 / 32) reading more fragments per MFMA.
static double wgrad_unit(int bm) { return bm == 128 ? 9.0 : bm == 96 ? 7.7 : bm == 64 ? 5.3 : 4.5; }
static long wgrad_sp(long M, int bm, int C, long ksteps) {
  const long groups = gad_ceil_div(M, bm) * (C / BK);
  long sp = 512 / groups;                 // one round of 2 workgroups per CU
  if (sp > ksteps / 8) sp = ksteps / 8;   // >= 8 K steps per workgroup
  return sp < 1 ? 1 : sp;
}
static double wgrad_launch_cost(const gad_gemm_args* a, long M, int bm) {
  const long ksteps = a->K / BK, groups = gad_ceil_div(M, bm) * (a->g.C / BK), sp = wgrad_sp(M, bm, a->g.C, ksteps);
  const long per = gad_ceil_div(ksteps, sp), spe = gad_ceil_div(ksteps, per);
  return (double)gad_ceil_div(groups * spe, 512) * (double)(per + 3) * wgrad_unit(bm);
}
static int wgrad_best_bm(const gad_gemm_args* a, long M, double* cost_out = nullptr) {
  int best = 128;
  double bc = 1e300;
  const int cand[4] = {128, 96, 64, 32};
  for (int bm : cand) {
    const double c = wgrad_launch_cost(a, M, bm);
    if (c < bc * (1 - 1e-9)) { bc = c; best = bm; }
  }
  if (cost_out) *cost_out = bc;
  return best;
}
static int wgrad_patch_bm(const gad_gemm_args* a) { return a->M % 4 == 0 ? wgrad_best_bm(a, a->M) : 128; }
static int wgrad_patch_splits(const gad_gemm_args* a, int* bm_out = nullptr) {
  const gad_conv_geom& g = a->g;
  if (a->flags & GAD_GEMM_NO_PATCH) return 0;
  if (use_bf16(a) || pick_vec(a) != 4 || a->a_mode != GAD_A_MC || a->b_mode != GAD_B_CONV) return 0;
  if (!same_3x3(g)) return 0;
  if (!(g.Wo == 64 || g.Wo == 32 || g.Wo == 16 || g.Wo == 8) || (g.Ho * g.Wo) % BK != 0 || a->K % BK != 0 || g.C % BK != 0 || a->M % 32 != 0) return 0;
  if (a->batch > 1 || a->tile_hint == HINT_64 || a->splitk_hint > 0 || a->lda % 4 != 0) return 0;
  if ((long)(a->K / (g.Ho * g.Wo)) * g.H * g.W * g.ldx >= (1L << 31)) return 0;
  const int bm = a->tile_hint == HINT_128 ? 128 : a->tile_hint == HINT_WGRAD_96 ? 96 : a->tile_hint == HINT_WGRAD_64 ? 64
               : a->tile_hint == HINT_WGRAD_32 ? 32 : wgrad_patch_bm(a);
  if (bm_out) *bm_out = bm;
  return (int)wgrad_sp(a->M, bm, g.C, a->K / BK);
}

// The same for the weight gradient's output channels (M): 224 = 128 + 96, 160 = 128 + 32, 320 = 256 + 64, 448 = 256 + 192,
// 672 = 384 + 288 run as two launches over disjoint row ranges (128-channel tiles, then one narrower width) when the
// launch model prefers that to the best single width by 2 % or more.
static bool wgrad_split_m(const gad_gemm_args* a, int* m1_out) {
  if (a->tile_hint >= HINT_SPLIT_M) {                        // forced split point (A/B tools)
    gad_gemm_args probe = *a;
    probe.tile_hint = 0;
    const int m1 = a->tile_hint - HINT_SPLIT_M;
    if (m1 <= 0 || m1 >= a->M || m1 % 128 != 0 || (a->M - m1) % 32 != 0 || !wgrad_patch_splits(&probe)) return false;
    *m1_out = m1;
    return true;
  }
  if (a->tile_hint != 0 || a->M % 32 != 0 || a->M < 160 || !wgrad_patch_splits(a)) return false;
  double single;
  wgrad_best_bm(a, a->M, &single);
  double best = 0.98 * single;
  bool found = false;
  for (int m1 = 128; m1 < a->M; m1 += 128) {                  // 128-channel tiles first, the rest on its best single width
    double c2;
    wgrad_best_bm(a, a->M - m1, &c2);
    const double c = wgrad_launch_cost(a, m1, 128) + c2;
    if (c < best) { best = c; *m1_out = m1; found = true; }
  }
  return found;
}

// 1x1 / stride 1 / pad 0 convolutions (ResNet shortcuts, attention projections of the LDM / SD blocks written as convs) are
// dense GEMMs over the pixel rows - and a two-source one (the shortcut of an up block reading cat([h, skip])) is the
// K-concatenated dense form.  Running them on the dense lean loaders instead of the im2col gather drops the per-slot
// coordinate arithmetic from the K loop; same products in the same order (bit-identical).
static bool as_dense_1x1(const gad_gemm_args* a, gad_gemm_args* out) {
  if (!a || (a->flags & GAD_GEMM_GENERAL_LOADERS)) return false;
  const gad_conv_geom& g = a->g;
  if (a->a_mode != GAD_A_CONV || a->b_mode != GAD_B_KC || a->A_k2) return false;
  if (g.KH != 1 || g.KW != 1 || g.stride != 1 || g.pad_t != 0 || g.pad_l != 0 || g.upsample || g.Ho != g.H || g.Wo != g.W) return false;
  if (a->K != g.C || a->K % 4 != 0 || g.ldx % 4 != 0 || a->batch > 1) return false;
  if (a->A2) {
    if (a->a_split <= 0 || a->a_split >= g.C || a->a_split % 32 != 0 || (g.C - a->a_split) % 4 != 0 || g.ldx < a->a_split ||
        a->ldx2 < g.C - a->a_split || a->ldx2 % 4 != 0 || !gad_aligned16(a->A2))
      return false;
  } else if (g.ldx < g.C) return false;
  *out = *a;
  out->a_mode = GAD_A_KC;
  out->lda = g.ldx;
  if (a->A2) {
    out->A_k2 = a->A2; out->lda_k2 = a->ldx2;
    out->B_k2 = a->B + a->a_split; out->ldb_k2 = a->ldb;
    out->k_split = a->a_split;
    out->A2 = nullptr; out->a_split = 0;
  }
  return true;
}
static gad_gemm_args canonical(const gad_gemm_args* a) {
  gad_gemm_args c;
  return as_dense_1x1(a, &c) ? c : *a;
}

// Winograd F(2x2, 3x3) route of the fp32 3x3 / stride 1 / pad 1 forward convolution (and, through ops.dgrad_as_forward, of
// its data gradient): taken when the caller supplies the transformed weights (B_wino) and the launch has tiles enough to
// fill the chip - small maps at small batch keep the direct LDS-patch kernels and their split-K.
static bool use_wino(const gad_gemm_args* a, WinoPlan* wp) {
  const gad_conv_geom& g = a->g;
  if ((!a->B_wino && !a->B_wino4) || a->operand_precision != 0 || a->a_mode != GAD_A_CONV || a->b_mode != GAD_B_KC || a->A2 || a->A_k2) return false;
  if (!same_3x3(g) || (g.Ho & 1) || (g.Wo & 1)) return false;
  if (g.C % BK != 0 || g.ldx % 4 != 0 || a->N % 4 != 0 || a->N < 64 || (a->tile_hint != 0 && (a->tile_hint < HINT_WINO2 || a->tile_hint > HINT_WINO4_FUSED64)) || a->splitk_hint > 0 || a->batch > 1) return false;
  if (a->flags & (GAD_GEMM_NO_WINO | GAD_GEMM_NO_PATCH | GAD_GEMM_SCALAR_EPILOGUE | GAD_GEMM_TAP_MAJOR_K)) return false;
  if (a->rowadd && a->rows_per_group != g.Ho * g.Wo) return false;
  if (a->M % (g.Ho * g.Wo) != 0) return false;
  const bool vec_ok = gad_aligned16(a->A) && gad_aligned16(a->C) && a->ldc % 4 == 0 && (!a->bias || gad_aligned16(a->bias)) &&
                      (!a->rowadd || (gad_aligned16(a->rowadd) && a->ld_rowadd % 4 == 0)) &&
                      (!a->residual || (gad_aligned16(a->residual) && a->ldr % 4 == 0));
  if (!vec_ok) return false;
  const bool force4 = a->tile_hint >= HINT_WINO4 && a->tile_hint <= HINT_WINO4_FUSED64;
  const bool f2_ok = a->B_wino != nullptr && (long)a->M / 4 < (1L << 30) && !force4;
  const bool f4_ok = a->B_wino4 != nullptr && (g.Ho & 3) == 0 && (g.Wo & 3) == 0 && a->tile_hint != HINT_WINO2;
  // Modelled times (calibrated on tools/ab_winograd.py, profiles/r03_ab_winograd.txt).  Transform launches stream their bytes
  // at ~4.9 TB/s.  F(2x2): a CU runs the 16-position product of one block at ~0.43 TF/s whether it holds one block or two,
  // so the GEMM takes ceil(blocks / 256) block times.  F(4x4): 36 batched products on 128 x 128 tiles, rounds of 512
  // workgroups, (K steps + 1) step times each.  Direct: the patch plan's rounds of 512 workgroups at ~0.26 TF/s each.
  const double x_bytes = 4.0 * (double)(a->M / (g.Ho * g.Wo)) * g.H * g.W * g.C;
  const double y_bytes = 4.0 * (double)a->M * a->N * (a->residual ? 2.0 : 1.0);
  double t2 = 1e30, t4 = 1e30;
  WinoPlan p2{}, p4{};
  if (f2_ok) {
    p2.f = 2;
    p2.T = (long)a->M / 4;
    p2.bytes = (int64_t)16 * p2.T * g.C * (int64_t)sizeof(float);
    double best = 1e30;
    for (int v = 0; v < 2; ++v) {
      const int bm = v ? 128 : 64, bn = v ? 64 : 128;
      const long tm = gad_ceil_div(p2.T, bm), tn = gad_ceil_div(a->N, bn);
      const double t = (double)gad_ceil_div(tm * tn, 256) * (16.0 * bm * bn * g.C * 2.0) / 0.43e12;
      if (t < best) { best = t; p2.bm = bm; p2.bn = bn; p2.tiles_m = (int)tm; p2.tiles_n = (int)tn; }
    }
    t2 = best + (x_bytes + (double)p2.bytes) / 4.9e12 + 6e-6;
  }
  if (f4_ok) {
    p4.f = 4;
    p4.T = (long)a->M / 16;
    // large launches: the six-position product kernel (one block per (xi, 64 x 128 tile): -5..13 % at >= 1024 blocks, where the
    // round quantisation of its one-block-per-CU rate is small); others: 36 batched products on the engine's own plan (64 x 64
    // tiles, split K) - profiles/r03_ab_winograd.txt
    const long pad128 = gad_ceil_div(a->N, 128) * 128, pad64 = gad_ceil_div(a->N, 64) * 64;
    if (pad64 < pad128) { p4.bm = 128; p4.bn = 64; } else { p4.bm = 64; p4.bn = 128; }
    p4.tiles_m = (int)gad_ceil_div(p4.T, p4.bm);
    p4.tiles_n = (int)gad_ceil_div(a->N, p4.bn);
    p4.fused4 = ((long)p4.tiles_m * p4.tiles_n * 6 >= 1024 && !(a->flags & GAD_GEMM_GENERAL_LOADERS)) ? 1 : 0;   // >= 4 rounds of one block per CU
    // one-launch form (wino4_fused.hip): a (32 tiles x 64 channels) block carries all 36 positions, two workgroups per CU at
    // ~0.2 TF/s executed each (rounds of 512); its epilogue reads the residual under the other workgroup's K loop, which costs
    // about the residual's bytes at 2.2 TB/s (profiles/r04_ab_winograd.txt, r04_wino4_fused_experiments.txt).  Taken when it
    // models no more than 5 % slower than the three-launch form (it moves a third less through HBM, and measured 0-3 % faster at
    // the shapes where the model calls a draw: profiles/r04_wino4_fused_experiments.txt run C) and its blocks fill most of a round.
    // block shape: 32 tiles x 64 channels, or 64 tiles x 32 channels where that pads the output channels less (N = 96, 160, 224, 288 ...)
    const bool narrow = gad_ceil_div(a->N, 32) * 32 < gad_ceil_div(a->N, 64) * 64;
    const long blocks32 = narrow ? gad_ceil_div(p4.T, 64) * gad_ceil_div(a->N, 32) : gad_ceil_div(p4.T, 32) * gad_ceil_div(a->N, 64);
    const double y_once = 4.0 * (double)a->M * a->N;
    const double t_full = (double)gad_ceil_div(blocks32, 512) * 36.0 * (g.C / BK) * (32.0 * 64.0 * BK * 2.0) / 0.20e12 +
                          (a->residual ? y_once / 2.2e12 : y_once / 20e12);
    const double vb = 36.0 * p4.T * g.C * 4.0;
    const long blocks = gad_ceil_div(p4.T, 128) * gad_ceil_div(a->N, 128) * 36;
    const double t_gemm = (double)gad_ceil_div(blocks, 512) * (g.C / BK + 1) * (128.0 * 128.0 * BK * 2.0) / 0.254e12;
    const double mb3 = (p4.fused4 ? 24.0 : 36.0) * p4.T * a->N * 4.0;
    const double t3 = t_gemm + (mb3 + y_bytes) / 4.9e12 + 12e-6;
    const bool full_ok = !(a->flags & GAD_GEMM_GENERAL_LOADERS) && a->tile_hint != HINT_WINO4_THREE;
    if (full_ok && (a->tile_hint == HINT_WINO4_FUSED32 || a->tile_hint == HINT_WINO4_FUSED64 || (t_full < 1.05 * t3 && blocks32 >= 320))) {
      p4.fused4 = 2;
      p4.bm = a->tile_hint == HINT_WINO4_FUSED64 ? 64 : narrow ? 65 : 32;       // 65 names the 64-tile x 32-channel shape (64: the one-workgroup-per-CU form kept for A/B)
      p4.bn = p4.bm == 65 ? 32 : 64;
      p4.tiles_m = (int)gad_ceil_div(p4.T, p4.bm == 32 ? 32 : 64);
      p4.tiles_n = (int)gad_ceil_div(a->N, p4.bn);
    }
    const double mb = p4.fused4 == 2 ? 0.0 : mb3;
    p4.bytes = (int64_t)(vb + mb);
    t4 = (x_bytes + vb) / 4.9e12 + (p4.fused4 == 2 ? t_full : t3) + 6e-6;
  }
  if (a->tile_hint == HINT_WINO2 || force4) {    // A/B tools force a route
    if (a->tile_hint == HINT_WINO2 && f2_ok) { *wp = p2; return true; }
    if (force4 && f4_ok) { *wp = p4; return true; }
    return false;
  }
  double t_direct;
  PatchPlan pp;
  if (use_patch_conv_f32(a, &pp)) {
    t_direct = (double)gad_ceil_div(pp.blocks, 512) * pp.chunks_per_split * 9.0 * (128.0 * pp.bn * 64.0) / 0.264e12;
    if (pp.splitk > 1) t_direct += 4e-6 + (double)a->M * a->N * 4.0 * (pp.splitk + 1) / 3.0e12;
  } else {
    t_direct = 2.0 * a->M * (double)a->N * a->K / 110e12;
  }
  const double tw = t2 < t4 ? t2 : t4;
  if (!(tw < 0.9 * t_direct)) return false;
  *wp = t2 < t4 ? p2 : p4;
  return true;
}

// Winograd F(4x4, 3x3) weight gradient: opted into by the caller (GAD_GEMM_WINO_WGRAD + wino_ws), taken when it models >= 10 %
// faster than the direct kernels (transform bytes at 4.9 TB/s + the 36 batched products at ~100 TF/s + three small launches)
static bool use_wino_wgrad(const gad_gemm_args* a, WinoWgradPlan* wq) {
  const gad_conv_geom& g = a->g;
  if (!(a->flags & GAD_GEMM_WINO_WGRAD) || (a->flags & (GAD_GEMM_NO_WINO | GAD_GEMM_NO_PATCH | GAD_GEMM_INTERNAL_WINO4))) return false;
  if (a->operand_precision != 0 || a->a_mode != GAD_A_MC || a->b_mode != GAD_B_CONV || a->A2 || a->A_k2 || a->batch > 1) return false;
  if (!same_3x3(g) || (g.Ho & 3) || (g.Wo & 3)) return false;
  if (g.C % 4 != 0 || g.ldx % 4 != 0 || a->M % 4 != 0 || a->lda % 4 != 0 || a->N != 9 * g.C || a->ldc % 4 != 0) return false;
  if ((a->tile_hint != 0 && a->tile_hint != HINT_WINO4) || a->splitk_hint > 0 || a->K % (g.Ho * g.Wo) != 0) return false;
  if (a->alpha != 1.f || a->bias || a->rowadd || a->residual) return false;
  if (!(gad_aligned16(a->A) && gad_aligned16(a->B) && gad_aligned16(a->C))) return false;
  wq->T = (long)a->K / 16;
  wq->wy_bytes = (int64_t)36 * wq->T * a->M * 4;
  wq->v_bytes = (int64_t)36 * wq->T * g.C * 4;
  wq->du_bytes = (int64_t)36 * a->M * g.C * 4;
  wq->bytes = wq->wy_bytes + wq->v_bytes + wq->du_bytes;
  if (a->tile_hint == HINT_WINO4) return true;
  const double dy_bytes = 4.0 * a->K * a->M, x_bytes = 4.0 * (double)(a->K / (g.Ho * g.Wo)) * g.H * g.W * g.C;
  const double t_w = (dy_bytes + x_bytes + (double)wq->wy_bytes + (double)wq->v_bytes) / 4.9e12 + 36.0 * wq->T * a->M * (double)g.C * 2.0 / 100e12 +
                     3.0 * (double)wq->du_bytes / 3.0e12 + 30e-6;
  const double t_direct = 2.0 * a->K * (double)a->M * a->N / 115e12;
  return t_w < 0.9 * t_direct;
}

// ---- the route: which kernels run a launch, and on what plan ----
// route_of is the one place that orders the routes; the size queries and gad_gemm all read the Route it returns.
enum class RouteKind { ENGINE, PATCH_F32, PATCH_BF16, FEWOUT, WGRAD_PATCH, WINO, WINO_WGRAD, SPLIT_N, SPLIT_M };
struct Route {
  RouteKind kind;
  gad_gemm_args a;           // the canonical arguments (as_dense_1x1)
  int vec;                   // pick_vec: 4 = the float4 loaders
  bool bf16;                 // use_bf16: the caller allows bf16 operands and the operands suit the bf16 instances
  Plan plan;                 // ENGINE
  PatchPlan pp;              // PATCH_F32; SPLIT_N: the single padded launch the split beats
  WinoPlan wp;               // WINO
  WinoWgradPlan wq;          // WINO_WGRAD
  int wbm, wsplits;          // WGRAD_PATCH, SPLIT_M: output-channel tile and pixel splits
  int split;                 // SPLIT_N: output columns of the first launch; SPLIT_M: its output rows
};

static Route route_of(const gad_gemm_args* args) {
  Route r{};
  r.a = canonical(args);
  const gad_gemm_args* a = &r.a;
  r.vec = pick_vec(a);
  r.bf16 = use_bf16(a);
  if (use_wino_wgrad(a, &r.wq)) r.kind = RouteKind::WINO_WGRAD;
  else if (use_wino(a, &r.wp)) r.kind = RouteKind::WINO;
  else if (patch_split_n(a, &r.split)) {
    r.kind = RouteKind::SPLIT_N;
    use_patch_conv_f32(a, &r.pp);
  } else if (wgrad_split_m(a, &r.split)) {
    r.kind = RouteKind::SPLIT_M;
    r.wsplits = wgrad_patch_splits(a, &r.wbm);
  } else if (use_fewout_conv(a)) r.kind = RouteKind::FEWOUT;
  else if ((r.wsplits = wgrad_patch_splits(a, &r.wbm))) r.kind = RouteKind::WGRAD_PATCH;
  else if (use_patch_conv(a)) r.kind = RouteKind::PATCH_BF16;
  else if (use_patch_conv_f32(a, &r.pp)) r.kind = RouteKind::PATCH_F32;
  else {
    r.kind = RouteKind::ENGINE;
    r.plan = make_plan(a);
  }
  return r;
}

// what gad_gemm_kernel_id and gad_gemm_plan report for a route: kernel family, tile, split
struct Report { int kid, tile, splitk; };
static Report report(const Route& r) {
  switch (r.kind) {
    case RouteKind::ENGINE: return {r.bf16 ? 1 : 0, r.plan.bm, r.plan.splitk};
    case RouteKind::PATCH_F32: return {2, r.pp.bn, r.pp.splitk};                       // 128 pixels x bn channels
    case RouteKind::SPLIT_N: return {2, 224, r.pp.splitk};                             // 224: two launches, 128-wide tiles then 96-wide ones
    case RouteKind::SPLIT_M: return {2, 224, r.wsplits};                               //      (weight gradient: 128-channel tiles, then the rest)
    case RouteKind::WGRAD_PATCH: return {2, r.wbm, r.wsplits};                         // output channels x pixel splits
    case RouteKind::PATCH_BF16: return {3, 128, 1};                                    // 128 x 128, never split
    case RouteKind::FEWOUT: return {4, 256, 1};                                        // 256 pixels x all (<= 4) output channels
    case RouteKind::WINO: return {r.wp.f == 2 ? 5 : 6, r.wp.f == 2 ? r.wp.bn : (r.wp.fused4 == 2 ? r.wp.bm : 128), 1};   // F(4x4): the block's tiles
    case RouteKind::WINO_WGRAD: return {7, 128, 1};                                    // 36 batched products on the engine's own plan
  }
  return {-1, 0, 0};
}

// the two launches of SPLIT_N (disjoint output columns) and SPLIT_M (disjoint output rows of a weight gradient)
static void split_halves(const Route& r, gad_gemm_args* lo, gad_gemm_args* hi) {
  const gad_gemm_args* a = &r.a;
  const int s = r.split;
  *lo = *a;
  *hi = *a;
  if (r.kind == RouteKind::SPLIT_M) {
    if (a->tile_hint >= HINT_SPLIT_M) lo->tile_hint = hi->tile_hint = 0;
    lo->M = s;
    hi->M = a->M - s;
    hi->A = a->A + s;                        // A_MC: dy [pixels][Cout], the output channel is the contiguous index
    hi->C = a->C + (long)s * a->ldc;
    return;
  }
  lo->B_wino = lo->B_wino4 = hi->B_wino = hi->B_wino4 = nullptr;    // the halves are direct launches: the transformed weights' position stride is the FULL Cout
  lo->wino_ws = hi->wino_ws = nullptr;
  lo->wino_ws_bytes = hi->wino_ws_bytes = 0;
  lo->N = s;
  hi->N = a->N - s;
  hi->B = a->B + (long)s * a->ldb;
  hi->C = a->C + s;
  if (a->bias) hi->bias = a->bias + s;
  if (a->rowadd) hi->rowadd = a->rowadd + s;
  if (a->residual) hi->residual = a->residual + s;
}

static int64_t workspace_bytes(const Route& r) {
  const gad_gemm_args* a = &r.a;
  switch (r.kind) {
    case RouteKind::ENGINE: case RouteKind::PATCH_F32: case RouteKind::WGRAD_PATCH: case RouteKind::PATCH_BF16: case RouteKind::FEWOUT: {
      const int splitk = report(r).splitk;              // one M x N slab of partial sums per split (and batch: the engine's)
      return splitk > 1 ? (int64_t)(a->batch > 0 ? a->batch : 1) * splitk * a->M * a->N * (int64_t)sizeof(float) : 0;
    }
    case RouteKind::WINO: {
      if (r.wp.f == 2 || r.wp.fused4) return 0;         // (the product kernels of both fused forms never split K)
      const gad_gemm_args sub = wino4_products_args(a, r.wp, nullptr, nullptr);     // the 36 batched products may split K
      return gad_gemm_workspace_bytes(&sub);
    }
    case RouteKind::WINO_WGRAD: {
      const gad_gemm_args sub = wino_wgrad_products_args(a, r.wq, nullptr, nullptr, nullptr);
      return gad_gemm_workspace_bytes(&sub);
    }
    case RouteKind::SPLIT_N: case RouteKind::SPLIT_M: {   // one launch after the other on the same workspace
      gad_gemm_args lo, hi;
      split_halves(r, &lo, &hi);
      const int64_t wl = gad_gemm_workspace_bytes(&lo), wh = gad_gemm_workspace_bytes(&hi);
      return wl > wh ? wl : wh;
    }
  }
  return 0;
}

extern "C" int gad_gemm_uses_bf16(const gad_gemm_args* a) { return a && route_of(a).bf16 ? 1 : 0; }

extern "C" int gad_gemm_kernel_id(const gad_gemm_args* a) { return a ? report(route_of(a)).kid : -1; }

extern "C" int gad_gemm_plan(const gad_gemm_args* a, int32_t* tile, int32_t* splitk, int32_t* vec) {
  GAD_CHECK(a && tile && splitk && vec, "gad_gemm_plan: null pointer");
  const Route r = route_of(a);
  const Report rep = report(r);
  *tile = rep.tile;
  *splitk = rep.splitk;
  *vec = r.vec;
  return 0;
}

extern "C" int64_t gad_gemm_wino_bytes(const gad_gemm_args* a) {
  if (!a) return 0;
  const Route r = route_of(a);
  return r.kind == RouteKind::WINO ? r.wp.bytes : r.kind == RouteKind::WINO_WGRAD ? r.wq.bytes : 0;
}

extern "C" int64_t gad_gemm_workspace_bytes(const gad_gemm_args* a) { return a ? workspace_bytes(route_of(a)) : 0; }

// ---- gad_gemm: check the arguments, resolve the route, dispatch on its kind ----

// shape / alignment contracts of the float4 paths (checked on the host so that a mismatch is an error, never an
// out-of-bounds access on the device)
static int check_args(const gad_gemm_args* a) {
  GAD_CHECK(a->M > 0 && a->N > 0 && a->K > 0, "gad_gemm: bad shape M=%d N=%d K=%d", a->M, a->N, a->K);
  const int am = a->a_mode, bmode = a->b_mode;
  GAD_CHECK(gad_aligned16(a->A) && gad_aligned16(a->B), "gad_gemm: A/B must be 16-byte aligned");
  const int k_first = a->A_k2 ? a->k_split : a->K;      // K-concatenated form: the first tensor covers k < k_split only
  if (am == GAD_A_KC) GAD_CHECK(a->lda >= k_first, "gad_gemm: A_KC needs lda >= K (K=%d lda=%d)", k_first, a->lda);
  if (am == GAD_A_MC) GAD_CHECK(a->lda >= a->M, "gad_gemm: A_MC needs lda >= M (M=%d lda=%d)", a->M, a->lda);
  if (bmode == GAD_B_KC) GAD_CHECK(a->ldb >= k_first, "gad_gemm: B_KC needs ldb >= K (K=%d ldb=%d)", k_first, a->ldb);
  if (bmode == GAD_B_MC) GAD_CHECK(a->ldb >= a->N, "gad_gemm: B_MC needs ldb >= N (N=%d ldb=%d)", a->N, a->ldb);
  const bool convA = am == GAD_A_CONV || am == GAD_A_CONVT;
  if (convA || bmode == GAD_B_CONV || bmode == GAD_B_WDGRAD) {
    const gad_conv_geom& g = a->g;
    GAD_CHECK(g.H > 0 && g.W > 0 && g.C > 0 && g.Ho > 0 && g.Wo > 0 && g.KH > 0 && g.KW > 0 && g.stride > 0 &&
              g.ldx >= (a->A2 ? a->a_split : g.C), "gad_gemm: bad conv geometry");
    GAD_CHECK((long)g.H * g.W * g.ldx < (1L << 31), "gad_gemm: image too large for 32-bit pixel offsets");
    if (convA) {
      GAD_CHECK(a->K == g.KH * g.KW * g.C, "gad_gemm: conv K=%d != KH*KW*C=%d", a->K, g.KH * g.KW * g.C);
      GAD_CHECK(a->M % (g.Ho * g.Wo) == 0, "gad_gemm: conv M=%d not a multiple of Ho*Wo", a->M);
      GAD_CHECK((long)(a->M / (g.Ho * g.Wo)) * g.H * g.W < (1L << 31), "gad_gemm: too many pixels");
    }
    if (bmode == GAD_B_WDGRAD) {
      GAD_CHECK(am == GAD_A_CONVT, "gad_gemm: B_WDGRAD pairs with A_CONVT");
      GAD_CHECK(a->N % 4 == 0, "gad_gemm: B_WDGRAD needs N%%4==0 (N=%d)", a->N);
    }
    if (bmode == GAD_B_CONV) {
      GAD_CHECK(a->N == g.KH * g.KW * g.C, "gad_gemm: wgrad N=%d != KH*KW*C=%d", a->N, g.KH * g.KW * g.C);
      GAD_CHECK(a->K % (g.Ho * g.Wo) == 0, "gad_gemm: wgrad K=%d not a multiple of Ho*Wo", a->K);
      GAD_CHECK((long)(a->K / (g.Ho * g.Wo)) * g.H * g.W < (1L << 31), "gad_gemm: too many pixels");
    }
  }
  const int vec = pick_vec(a);
  if (a->A2) {
    GAD_CHECK(am == GAD_A_CONV && bmode == GAD_B_KC, "gad_gemm: A2 (two-source gather) is an A_CONV x B_KC feature");
    GAD_CHECK(a->a_split > 0 && a->a_split < a->g.C && a->a_split % 32 == 0 && a->g.C % 32 == 0,
              "gad_gemm: two-source gather needs a_split and C multiples of 32 (a_split=%d C=%d)", a->a_split, a->g.C);
    GAD_CHECK(a->ldx2 >= a->g.C - a->a_split && a->ldx2 % 4 == 0 && gad_aligned16(a->A2) && vec == 4,
              "gad_gemm: two-source gather: bad ldx2 / alignment");
  }
  if (a->A_k2) {
    GAD_CHECK(am == GAD_A_KC && (bmode == GAD_B_KC || bmode == GAD_B_MC) && a->B_k2 && !a->A2 && a->batch <= 1,
              "gad_gemm: the K-concatenated form (A_k2 / B_k2) is an A_KC x B_KC|B_MC feature");
    GAD_CHECK(a->k_split > 0 && a->k_split < a->K && a->k_split % 32 == 0, "gad_gemm: k_split must be a multiple of 32 inside (0, K) (k_split=%d K=%d)", a->k_split, a->K);
    const int k2 = a->K - a->k_split;
    GAD_CHECK(a->lda >= a->k_split && a->lda_k2 >= k2 && a->lda_k2 % 4 == 0 && k2 % 4 == 0 && gad_aligned16(a->A_k2) && gad_aligned16(a->B_k2),
              "gad_gemm: K-concatenated operands need 16-byte alignment and K2 %% 4 == 0 (K2=%d lda_k2=%d)", k2, a->lda_k2);
    if (bmode == GAD_B_KC) GAD_CHECK(a->ldb >= a->k_split && a->ldb_k2 >= k2 && a->ldb_k2 % 4 == 0, "gad_gemm: bad ldb_k2");
    else GAD_CHECK(a->ldb_k2 >= a->N && a->ldb_k2 % 4 == 0, "gad_gemm: bad ldb_k2");
    GAD_CHECK(vec == 4, "gad_gemm: the K-concatenated form needs the float4 path");
  }
  if (a->rowadd) GAD_CHECK(a->rows_per_group > 0 && a->ld_rowadd >= a->N, "gad_gemm: bad rowadd");
  if (a->residual) GAD_CHECK(a->ldr >= a->N, "gad_gemm: bad residual stride");
  GAD_CHECK(a->ldc >= a->N, "gad_gemm: ldc < N");
  GAD_CHECK(a->operand_precision == 0 || a->operand_precision == 1, "gad_gemm: operand_precision must be 0 (f32) or 1 (bf16 allowed)");
  return 0;
}

// GAD_GEMM_WINO_ONLY_INPUT / _SKIP_INPUT run one stage of a Winograd launch: on any other route they would silently run a
// direct kernel that reads A (which a caller holding only the transformed image does not have), so they are refused there
static int check_stage_flags(const Route& r) {
  const bool only_input = (r.a.flags & GAD_GEMM_WINO_ONLY_INPUT) != 0, skip_input = (r.a.flags & GAD_GEMM_WINO_SKIP_INPUT) != 0;
  GAD_CHECK(!(only_input && skip_input), "gad_gemm: GAD_GEMM_WINO_ONLY_INPUT and GAD_GEMM_WINO_SKIP_INPUT exclude each other");
  GAD_CHECK(!only_input || r.kind == RouteKind::WINO,
            "gad_gemm: GAD_GEMM_WINO_ONLY_INPUT on a launch that takes no Winograd forward route (kernel id %d)", report(r).kid);
  GAD_CHECK(!skip_input || r.kind == RouteKind::WINO || r.kind == RouteKind::WINO_WGRAD,
            "gad_gemm: GAD_GEMM_WINO_SKIP_INPUT on a launch that takes no Winograd route (kernel id %d)", report(r).kid);
  return 0;
}

static DevArgs dev_args(const gad_gemm_args* a) {
  DevArgs d;
  d.A = a->A; d.B = a->B; d.C = a->C;
  d.A2 = a->A2; d.a_split = a->a_split; d.ldx2 = a->ldx2;
  d.Ak2 = a->A_k2; d.Bk2 = a->B_k2; d.lda2 = a->lda_k2; d.ldb2 = a->ldb_k2; d.k_split = a->k_split;
  d.Bh = nullptr;
  d.M = a->M; d.N = a->N; d.K = a->K;
  d.lda = a->lda; d.ldb = a->ldb; d.ldc = a->ldc;
  d.batch_inner = a->batch_inner > 0 ? a->batch_inner : 1;
  d.sA0 = a->strideA0; d.sA1 = a->strideA1; d.sB0 = a->strideB0; d.sB1 = a->strideB1;
  d.sC0 = a->strideC0; d.sC1 = a->strideC1;
  d.g = a->g;
  d.fdC = make_fastdiv(a->g.C);
  d.fdKW = make_fastdiv(a->g.KW);
  d.fdHoWo = make_fastdiv((unsigned)a->g.Ho * a->g.Wo);
  d.fdWo = make_fastdiv(a->g.Wo);
  d.fdRpg = make_fastdiv(a->rows_per_group > 0 ? a->rows_per_group : 1);
  d.taps = a->g.KH * a->g.KW;
  d.fdTaps = make_fastdiv(d.taps > 0 ? d.taps : 1);
  const bool convA = a->a_mode == GAD_A_CONV || a->a_mode == GAD_A_CONVT;
  d.kperm = (convA && d.taps > 1 && a->g.C % BK == 0 && !(a->flags & GAD_GEMM_TAP_MAJOR_K)) ? 1 : 0;
  d.alpha = a->alpha;
  d.bias = a->bias; d.rowadd = a->rowadd; d.rows_per_group = a->rows_per_group > 0 ? a->rows_per_group : 1;
  d.ld_rowadd = a->ld_rowadd; d.residual = a->residual; d.ldr = a->ldr;
  d.ws = (float*)a->ws;
  d.tiles_m = d.tiles_n = d.splitk = d.ktiles_per_split = 1;
  // float4 epilogue: every tensor the epilogue touches can be addressed as aligned float4 at columns that are multiples of 4
  d.epi_vec = (!(a->flags & GAD_GEMM_SCALAR_EPILOGUE) && gad_aligned16(a->C) && a->ldc % 4 == 0 && a->N % 4 == 0 &&
               a->strideC0 % 4 == 0 && a->strideC1 % 4 == 0 && (!a->bias || gad_aligned16(a->bias)) &&
               (!a->rowadd || (gad_aligned16(a->rowadd) && a->ld_rowadd % 4 == 0)) &&
               (!a->residual || (gad_aligned16(a->residual) && a->ldr % 4 == 0)) && (!a->ws || gad_aligned16(a->ws))) ? 1 : 0;
  return d;
}

static int launch_fewout(const Route& r, const DevArgs& d, hipStream_t st) {
  const gad_gemm_args* a = &r.a;
  dim3 grid((unsigned)(a->M / 256)), block(NTHREADS);
#define GAD_FEWOUT(W_)                                                                          \
  do {                                                                                          \
    if (a->N <= 3) hipLaunchKernelGGL((conv3x3_fewout_kernel<W_, 3>), grid, block, 0, st, d);   \
    else hipLaunchKernelGGL((conv3x3_fewout_kernel<W_, 4>), grid, block, 0, st, d);             \
  } while (0)
  if (a->g.W == 64) GAD_FEWOUT(64);
  else if (a->g.W == 32) GAD_FEWOUT(32);
  else GAD_FEWOUT(16);
#undef GAD_FEWOUT
  GAD_LAUNCH_CHECK("gad_gemm(conv3x3 few outputs)");
  return 0;
}

static int launch_wgrad_patch(const Route& r, DevArgs& d, hipStream_t st) {
  const gad_gemm_args* a = &r.a;
  const int wbm = r.wbm;
  const long ksteps = a->K / BK;
  d.tiles_m = (int)gad_ceil_div(a->M, wbm);
  d.ktiles_per_split = (int)gad_ceil_div(ksteps, r.wsplits);
  d.splitk = (int)gad_ceil_div(ksteps, d.ktiles_per_split);
  if (d.splitk > 1) {
    int64_t need = (int64_t)d.splitk * a->M * a->N * (int64_t)sizeof(float);
    GAD_CHECK(a->ws && a->ws_bytes >= need, "gad_gemm: wgrad workspace too small (%lld < %lld)", (long long)a->ws_bytes, (long long)need);
  }
  dim3 grid((unsigned)(d.splitk * d.tiles_m * (a->g.C / BK))), block(NTHREADS);
#define GAD_WGRAD(W_)                                                                                   \
  do {                                                                                                  \
    if (wbm == 96) hipLaunchKernelGGL((wgrad3x3_patch_f32_kernel<W_, 96>), grid, block, 0, st, d);      \
    else if (wbm == 64) hipLaunchKernelGGL((wgrad3x3_patch_f32_kernel<W_, 64>), grid, block, 0, st, d); \
    else if (wbm == 32) hipLaunchKernelGGL((wgrad3x3_patch_f32_kernel<W_, 32>), grid, block, 0, st, d); \
    else hipLaunchKernelGGL((wgrad3x3_patch_f32_kernel<W_, 128>), grid, block, 0, st, d);               \
  } while (0)
  if (a->g.Wo == 64) GAD_WGRAD(64);
  else if (a->g.Wo == 32) GAD_WGRAD(32);
  else if (a->g.Wo == 16) GAD_WGRAD(16);
  else GAD_WGRAD(8);
#undef GAD_WGRAD
  GAD_LAUNCH_CHECK("gad_gemm(wgrad3x3 patch)");
  if (d.splitk > 1) {
    launch_splitk_reduce(d, 1, st);
    GAD_LAUNCH_CHECK("gad_gemm(wgrad splitk reduce)");
  }
  return 0;
}

static int launch_patch_bf16(const Route& r, DevArgs& d, hipStream_t st) {
  const gad_gemm_args* a = &r.a;
  d.tiles_m = (int)gad_ceil_div(a->M, 128);
  d.tiles_n = (int)gad_ceil_div(a->N, 128);
  d.splitk = 1;
  dim3 grid((unsigned)(d.tiles_m * d.tiles_n)), block(NTHREADS);
  const bool wb = a->B_bf16 != nullptr;
  if (wb) GAD_CHECK(gad_aligned16(a->B_bf16) && a->ldb % 8 == 0, "gad_gemm: B_bf16 must be 16-byte aligned with ldb %% 8 == 0");
  d.Bh = (const unsigned short*)a->B_bf16;
#define GAD_PATCH_BF16(W_, NI_)                                                                         \
  do {                                                                                                  \
    if (wb) hipLaunchKernelGGL((conv3x3_patch_bf16_kernel<W_, NI_, true>), grid, block, 0, st, d);      \
    else hipLaunchKernelGGL((conv3x3_patch_bf16_kernel<W_, NI_, false>), grid, block, 0, st, d);        \
  } while (0)
  if (a->g.Wo == 64) GAD_PATCH_BF16(64, 1);
  else if (a->g.Wo == 32) GAD_PATCH_BF16(32, 1);
  else if (a->g.Wo == 16) GAD_PATCH_BF16(16, 1);
  else if (a->g.Wo == 8) GAD_PATCH_BF16(8, 2);
  else GAD_PATCH_BF16(4, 8);
#undef GAD_PATCH_BF16
  GAD_LAUNCH_CHECK("gad_gemm(conv3x3 patch)");
  return 0;
}

static int launch_patch_f32(const Route& r, DevArgs& d, hipStream_t st) {
  const gad_gemm_args* a = &r.a;
  const PatchPlan& pp = r.pp;
  d.tiles_m = (int)gad_ceil_div(a->M, 128);
  d.tiles_n = (int)gad_ceil_div(a->N, pp.bn);
  d.splitk = pp.splitk;
  d.ktiles_per_split = pp.chunks_per_split;
  if (pp.splitk > 1) {
    int64_t need = (int64_t)pp.splitk * a->M * a->N * (int64_t)sizeof(float);
    GAD_CHECK(a->ws && a->ws_bytes >= need, "gad_gemm: patch-conv split-K workspace too small (%lld < %lld)", (long long)a->ws_bytes, (long long)need);
  }
  dim3 grid((unsigned)pp.blocks), block(NTHREADS);
  const bool dg = a->a_mode == GAD_A_CONVT;
#define GAD_PATCH(W_, NI_)                                                                                           \
  do {                                                                                                               \
    if (dg) hipLaunchKernelGGL((conv3x3_patch_f32_kernel<W_, NI_, true>), grid, block, 0, st, d);                    \
    else if (pp.bn == 96) hipLaunchKernelGGL((conv3x3_patch_f32_kernel<W_, NI_, false, 96>), grid, block, 0, st, d);   \
    else if (pp.bn == 160) hipLaunchKernelGGL((conv3x3_patch_f32_kernel<W_, NI_, false, 160>), grid, block, 0, st, d); \
    else hipLaunchKernelGGL((conv3x3_patch_f32_kernel<W_, NI_, false>), grid, block, 0, st, d);                      \
  } while (0)
  if (a->g.Wo == 64) GAD_PATCH(64, 1);
  else if (a->g.Wo == 32) GAD_PATCH(32, 1);
  else if (a->g.Wo == 16) GAD_PATCH(16, 1);
  else if (a->g.Wo == 8) GAD_PATCH(8, 2);
  else GAD_PATCH(4, 8);
#undef GAD_PATCH
  GAD_LAUNCH_CHECK("gad_gemm(conv3x3 patch f32)");
  if (pp.splitk > 1) {
    launch_splitk_reduce(d, 1, st);
    GAD_LAUNCH_CHECK("gad_gemm(patch splitk reduce)");
  }
  return 0;
}

// the generic engine: the one place the tile / split-K cost model (make_plan) runs
static int launch_engine(const Route& r, DevArgs& d, hipStream_t st) {
  const gad_gemm_args* a = &r.a;
  const Plan& pl = r.plan;
  const int am = a->a_mode, bmode = a->b_mode, vec = r.vec;
  const bool bf16 = r.bf16;
  const long batch = a->batch > 0 ? a->batch : 1;
  GAD_CHECK(pl.nblocks > 0 && pl.nblocks < (1L << 31), "gad_gemm: grid too large");
  if (pl.splitk > 1) {
    int64_t need = (int64_t)batch * pl.splitk * a->M * a->N * (int64_t)sizeof(float);
    GAD_CHECK(a->ws && a->ws_bytes >= need, "gad_gemm: split-K workspace too small (%lld < %lld)", (long long)a->ws_bytes, (long long)need);
  }
  d.tiles_m = pl.tiles_m; d.tiles_n = pl.tiles_n; d.splitk = pl.splitk; d.ktiles_per_split = pl.ktiles_per_split;
  if (a->A2) {
    if (bf16) launch_bf16<A_CONV2, GAD_B_KC>(d, pl, st);
    else launch_mode<A_CONV2, GAD_B_KC, 4>(d, pl, st);
  } else if (a->A_k2) {
    const bool lean = vec == 4 && a->K % BK == 0 && a->k_split % BK == 0 && !(a->flags & GAD_GEMM_GENERAL_LOADERS);
    if (bmode == GAD_B_KC) {
      if (bf16 && lean) launch_bf16<A_KC2_L, B_KC2_L>(d, pl, st);
      else if (bf16) launch_bf16<A_KC2, B_KC2>(d, pl, st);
      else if (lean) launch_mode<A_KC2_L, B_KC2_L, 4>(d, pl, st);
      else launch_mode<A_KC2, B_KC2, 4>(d, pl, st);
    } else {
      if (bf16 && lean) launch_bf16<A_KC2_L, B_MC2_L>(d, pl, st);
      else if (bf16) launch_bf16<A_KC2, B_MC2>(d, pl, st);
      else if (lean) launch_mode<A_KC2_L, B_MC2_L, 4>(d, pl, st);
      else launch_mode<A_KC2, B_MC2, 4>(d, pl, st);
    }
  } else if (vec == 4 && a->K % BK == 0 && !(a->flags & GAD_GEMM_GENERAL_LOADERS) &&
             ((am == GAD_A_KC && (bmode == GAD_B_KC || bmode == GAD_B_MC)) || (am == GAD_A_MC && bmode == GAD_B_MC))) {
    // dense operands without a K tail: the lean loaders (row clamp instead of masks, one add per slot and step)
    if (bf16) {
      if (am == GAD_A_KC && bmode == GAD_B_KC) launch_bf16<A_KC_L, B_KC_L>(d, pl, st);
      else if (am == GAD_A_KC) launch_bf16<A_KC_L, B_MC_L>(d, pl, st);
      else launch_bf16<A_MC_L, B_MC_L>(d, pl, st);
    } else if (am == GAD_A_KC && bmode == GAD_B_KC) {
      if (a->flags & GAD_GEMM_INTERNAL_WINO4) launch_mode<A_KC_L, B_KC_L, 4, 1>(d, pl, st);
      else launch_mode<A_KC_L, B_KC_L, 4>(d, pl, st);
    }
    else if (am == GAD_A_KC) launch_mode<A_KC_L, B_MC_L, 4>(d, pl, st);
    else launch_mode<A_MC_L, B_MC_L, 4>(d, pl, st);
  } else
#define GAD_CASE(AMODE, BMODE_)                                                        \
  if (am == AMODE && bmode == BMODE_) {                                                \
    if (bf16) launch_bf16<AMODE, BMODE_>(d, pl, st);                                   \
    else if (vec == 4) launch_mode<AMODE, BMODE_, 4>(d, pl, st);                       \
    else launch_mode<AMODE, BMODE_, 1>(d, pl, st);                                     \
  } else
  GAD_CASE(GAD_A_KC, GAD_B_KC)
  GAD_CASE(GAD_A_KC, GAD_B_MC)
  GAD_CASE(GAD_A_MC, GAD_B_MC)
  GAD_CASE(GAD_A_CONV, GAD_B_KC)
  GAD_CASE(GAD_A_CONVT, GAD_B_WDGRAD)
  GAD_CASE(GAD_A_MC, GAD_B_CONV)
  {
    gad_set_error("gad_gemm: unsupported mode pair a_mode=%d b_mode=%d", am, bmode);
    return 1;
  }
#undef GAD_CASE
  GAD_LAUNCH_CHECK("gad_gemm");
  if (pl.splitk > 1) {
    launch_splitk_reduce(d, (int)batch, st);
    GAD_LAUNCH_CHECK("gad_gemm(splitk reduce)");
  }
  return 0;
}

extern "C" int gad_gemm(const gad_gemm_args* args, void* stream) {
  GAD_CHECK(args && args->A && args->B && args->C, "gad_gemm: null pointer");
  const gad_gemm_args canon = canonical(args);
  if (const int rc = check_args(&canon)) return rc;
  const Route r = route_of(&canon);
  if (const int rc = check_stage_flags(r)) return rc;
  hipStream_t st = (hipStream_t)stream;
  DevArgs d = dev_args(&r.a);
  switch (r.kind) {
    case RouteKind::SPLIT_N: case RouteKind::SPLIT_M: {
      gad_gemm_args lo, hi;
      split_halves(r, &lo, &hi);
      const int rc = gad_gemm(&lo, stream);
      return rc ? rc : gad_gemm(&hi, stream);
    }
    case RouteKind::WINO_WGRAD: return launch_wino_wgrad(&r.a, r.wq, stream);
    case RouteKind::WINO: return launch_wino(&r.a, r.wp, d, stream);
    case RouteKind::FEWOUT: return launch_fewout(r, d, st);
    case RouteKind::WGRAD_PATCH: return launch_wgrad_patch(r, d, st);
    case RouteKind::PATCH_BF16: return launch_patch_bf16(r, d, st);
    case RouteKind::PATCH_F32: return launch_patch_f32(r, d, st);
    case RouteKind::ENGINE: return launch_engine(r, d, st);
  }
  return 1;
}
