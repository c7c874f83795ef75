"""A CPU restatement of gad_gemm's dense ABI (include/gad.h: gad_gemm_args) in plain torch on FLAT buffers: every address
the launch may touch is written out as index arithmetic here, so that leading dimensions, batch strides, pointer offsets,
the K-concatenated operands and the epilogue's own strides are part of what a test compares.  fp64 throughout; no GPU and
no import of the package under test.

    C[z0*sC0 + z1*sC1 + m*ldc + n] = alpha * sum_k A(z, m, k) * B(z, n, k) + bias[n] + rowadd[m // rows_per_group][n]
                                     + residual[z0*sC0 + z1*sC1 + m*ldr + n]            z = z0 * batch_inner + z1

`expected` returns the WHOLE output buffer: the computed elements as above, every other float as the caller filled it (a
sentinel), so that row padding, the gaps between batch slabs and the floats before a misaligned C are compared too."""
from dataclasses import dataclass

import torch

A_KC, A_MC = 0, 1             # enum gad_a_mode: A[m][k] / A[k][m], row stride lda
B_KC, B_MC = 0, 1             # enum gad_b_mode: B[n][k] / B[k][n], row stride ldb


@dataclass(frozen=True)
class Launch:
    """One dense gad_gemm launch.  Pointers are (flat buffer, offset in floats) pairs: the off_* fields are the offsets."""
    a_mode: int
    b_mode: int
    M: int
    N: int
    K: int
    lda: int
    ldb: int
    ldc: int
    batch: int = 1
    batch_inner: int = 1      # <= 0 means 1
    sA: tuple = (0, 0)
    sB: tuple = (0, 0)
    sC: tuple = (0, 0)        # the residual uses these too
    alpha: float = 1.0
    rows_per_group: int = 1
    ld_rowadd: int = 0
    ldr: int = 0
    k_split: int = 0          # > 0: k >= k_split reads A_k2[m][k - k_split] (row stride lda_k2) and B_k2 (laid out like B, ldb_k2)
    lda_k2: int = 0
    ldb_k2: int = 0
    off_A: int = 0
    off_B: int = 0
    off_C: int = 0
    off_bias: int = 0
    off_rowadd: int = 0
    off_residual: int = 0

    @property
    def inner(self):
        return self.batch_inner if self.batch_inner > 0 else 1

    def slabs(self):
        """(z0, z1) of every batch index z = z0 * inner + z1."""
        return [divmod(z, self.inner) for z in range(max(1, self.batch))]


def _operand(buf, off, k_contiguous, rows, k0, k1, ld):
    """[rows][k1 - k0] in fp64 out of a flat buffer: element (r, k) at off + r*ld + k (k contiguous) or off + k*ld + r."""
    r = torch.arange(rows, dtype=torch.int64)[:, None]
    k = torch.arange(k0, k1, dtype=torch.int64)[None, :]
    idx = off + (r * ld + k if k_contiguous else k * ld + r)
    return buf[idx].double()


def products(L, A, B, A_k2=None, B_k2=None, magnitudes=False):
    """Yield (z0, z1, acc [M][N] fp64) for every batch slab: the plain sums over k, before alpha and the epilogue
    (magnitudes: sum_k |A| |B| instead, which bounds every partial sum in any summation order)."""
    k1 = L.k_split if L.k_split > 0 else L.K
    for z0, z1 in L.slabs():
        a = _operand(A, L.off_A + z0 * L.sA[0] + z1 * L.sA[1], L.a_mode == A_KC, L.M, 0, k1, L.lda)
        b = _operand(B, L.off_B + z0 * L.sB[0] + z1 * L.sB[1], L.b_mode == B_KC, L.N, 0, k1, L.ldb)
        if L.k_split > 0:
            a = torch.cat([a, _operand(A_k2, 0, True, L.M, 0, L.K - k1, L.lda_k2)], dim=1)
            b = torch.cat([b, _operand(B_k2, 0, L.b_mode == B_KC, L.N, 0, L.K - k1, L.ldb_k2)], dim=1)
        yield z0, z1, (a.abs() @ b.abs().T if magnitudes else a @ b.T)


def expected(L, A, B, C0, bias=None, rowadd=None, residual=None, A_k2=None, B_k2=None):
    """The whole output buffer after the launch, fp64.  C0: the output buffer as it is before the launch (sentinel-filled)."""
    out = C0.double().clone()
    m = torch.arange(L.M, dtype=torch.int64)[:, None]
    n = torch.arange(L.N, dtype=torch.int64)[None, :]
    for z0, z1, acc in products(L, A, B, A_k2, B_k2):
        coff = z0 * L.sC[0] + z1 * L.sC[1]
        c = L.alpha * acc
        if bias is not None:
            c = c + bias[L.off_bias + n].double()
        if rowadd is not None:
            c = c + rowadd[L.off_rowadd + (m // L.rows_per_group) * L.ld_rowadd + n].double()
        if residual is not None:
            c = c + residual[L.off_residual + coff + m * L.ldr + n].double()
        out[L.off_C + coff + m * L.ldc + n] = c
    return out


def max_scaled_acc(L, A, B, A_k2=None, B_k2=None):
    """max |alpha| sum_k |A| |B| over the launch: at least max |alpha * acc|, and a bound on every partial sum, split-K slab
    and scaled accumulator a kernel can form on the way, whatever its summation order."""
    return max(float(abs(L.alpha) * acc.max()) for _, _, acc in products(L, A, B, A_k2, B_k2, magnitudes=True))
