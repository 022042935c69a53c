"""Split-K products (few output tiles, long k) through gemm against the phase path split + products + recombine,
which never splits k: the same bytes of C, nothing outside C or the workspace touched, the expected products
kernel, and an error against the double-double product no larger than the phase path's."""
import pytest
import torch

import gemmul8 as G

pytestmark = pytest.mark.gpu
SK, SENTINEL, TAIL = "gemm_i8_splitk_kernel", -7.25, 4096

# m, n, k, N, kwargs (kernel: the expected products kernel; None: anything but split-K)
CASES = [
    (200, 130, 16400, 14, {}),                                   # one ragged tile, S = 2, ranges of 128 + 129 steps
    (300, 520, 20000, 8, dict(alpha=0.5, beta=-0.5, pad=(3, 5, 9), opA=G.OP_T)),  # 6 tiles, 313 steps in 2, decode
    (70, 90, 70000, 14, dict(fast=False)),                       # padded k in (2^16, 2^17], S = 8, 1094 steps
    (520, 520, 140000, 14, {}),                                  # 126 units, S = 2, two chunks per split
    (200, 130, 16400, 10, dict(dtype=torch.float32)),            # one-level CRT downstream
    (70, 90, 10000, 12, dict(dtype=torch.complex128, ctype=G.COMPLEX_BIG_MATRIX_ENCODE)),  # big matrix, k doubled
    (200, 130, 8192, 14, dict(kernel="gemm_i8_kernel")),         # 128 steps: below the domain
    (1024, 1024, 8192, 14, dict(kernel=None)),                   # 224 units: above it
]


@pytest.mark.parametrize("m,n,k,N,kw", CASES)
def test_splitk_gemm_matches_the_phase_path(m, n, k, N, kw):
    dtype, fast, ct = kw.get("dtype", torch.float64), kw.get("fast", True), kw.get("ctype", G.REAL_DEFAULT)
    alpha, beta, opA = kw.get("alpha", 1.0), kw.get("beta", 0.0), kw.get("opA", G.OP_N)
    dlda, dldb, dldc = kw.get("pad", (0, 0, 0))
    ra, ca = (m, k) if opA == G.OP_N else (k, m)
    lda, ldb, ldc = ra + dlda, k + dldb, m + dldc

    def operand(rows, cols, ld, seed):
        buf = torch.zeros(ld * cols, dtype=dtype, device="cuda")
        buf.view(cols, ld)[:, :rows].copy_(G.randmat(rows, cols, dtype, seed=seed))
        return buf

    bufA, bufB = operand(ra, ca, lda, 100), operand(k, n, ldb, 200)
    view = lambda buf: buf[:ldc * n].view(n, ldc)[:, :m]  # [col, row]
    C0 = torch.full((ldc * n + 3,), SENTINEL, dtype=dtype, device="cuda")
    view(C0).copy_(G.randmat(m, n, dtype, seed=900))
    inside = torch.zeros_like(C0, dtype=torch.bool)
    view(inside)[:] = True
    Cg, Cp = C0.clone(), C0.clone()
    size = G.workSize(m, n, k, N, ct)
    works = [torch.full((size + TAIL,), 0xA5, dtype=torch.uint8, device="cuda") for _ in range(2)]

    G.gemm(opA, G.OP_N, m, n, k, alpha, bufA, lda, bufB, ldb, beta, Cg, ldc, N, fast, works[0], ct)
    kernel = G.last_products_kernel()
    G.split(opA, G.OP_N, m, n, k, bufA, lda, bufB, ldb, N, fast, works[1], dtype, computeType=ct)
    G.products(m, n, k, N, works[1], computeType=ct)
    G.recombine(m, n, k, N, alpha, beta, Cp, ldc, works[1], computeType=ct)
    torch.cuda.synchronize()

    u8 = lambda x: x.contiguous().view(torch.uint8)
    assert u8(Cg[inside]).equal(u8(Cp[inside]))                       # 1. the phase path's bytes
    assert u8(Cg[~inside]).equal(u8(C0[~inside]))                     # 2. ldc padding and tails untouched
    assert all(bool((w[size:] == 0xA5).all()) for w in works)
    want = kw.get("kernel", SK)                                       # 3. the products kernel
    assert kernel == want if want else kernel != SK, kernel
    if dtype == torch.float64:                                        # 4. no worse than the phase path
        Av = bufA.view(ca, lda)[:, :ra]
        X = (Av if opA == G.OP_N else Av.t()).contiguous()
        C1, C2 = G.dd_gemm(X, bufB.view(n, ldb)[:, :k].contiguous(), m, n, k)
        err = [G.relerr_dd(((view(c) - beta * view(C0)) / alpha).contiguous(), C1, C2)[0] for c in (Cg, Cp)]
        print(f"max rel err gemm {err[0]:.3e} phases {err[1]:.3e}, products: {kernel}")
        assert err[0] <= err[1]
