"""herk against gemm(A, A^H): off the diagonal the triangle carries gemm's bits, the diagonal its real part and a
+0.0 imaginary part, nothing outside the triangle is touched, and the error against the complex128 product is no
larger than gemm's."""
import pytest
import torch

import gemmul8 as G

pytestmark = pytest.mark.gpu
N_, C_, LO, UP = G.OP_N, G.OP_C, G.FILL_LOWER, G.FILL_UPPER
SENTINEL = complex(-7.25, 3.5)
HERK = ("gemm_i8_herk_kernel", "gemm_i8_herk_onetile_kernel")

# n, k, N, uplo, trans, kwargs
CASES = [
    (200, 100, 12, LO, N_, dict(kernel=HERK[1])),                    # one ragged diagonal tile, 2 k-steps; gemm takes
                                                                     # the big-matrix geometry here
    (520, 448, 8, UP, C_, dict(pad=(5, 9), alpha=0.5, beta=-1.5)),   # 3 tile rows, 7 k-steps, clipped tile, conj on A
    (1300, 390, 14, LO, N_, dict(kernel=HERK[0])),                   # T = 6, 882 units: claims, clipped band
    (1300, 390, 14, UP, N_, dict(kernel=HERK[0], beta=1.0)),         # the swapped decode, persistent
    (300, 200, 2, LO, C_, {}),                                       # fewest moduli, one-level CRT
    (300, 200, 10, LO, N_, dict(dtype=torch.complex64)),             # f32 output path
    (300, 200, 10, UP, N_, dict(fast=False)),                        # accurate mode through gemm's split
    (260, 66000, 4, LO, N_, dict(not_herk=True)),                    # k_pad > 2^16: all tiles + triangular CRT
]


def _operand(rows, cols, ld, dtype, seed):
    """column-major rows x cols matrix with leading dimension ld: (flat buffer, (cols, rows) view)"""
    buf = torch.zeros(ld * cols, dtype=dtype, device="cuda")
    view = buf.view(cols, ld)[:, :rows]
    view.copy_(G.randmat(rows, cols, dtype, seed=seed))
    return buf, view


@pytest.mark.parametrize("n,k,N,uplo,trans,kw", CASES)
def test_herk_matches_gemm_triangle(n, k, N, uplo, trans, kw):
    dtype, fast = kw.get("dtype", torch.complex128), kw.get("fast", True)
    alpha, beta = kw.get("alpha", 1.0), kw.get("beta", 0.0)
    dlda, dldc = kw.get("pad", (0, 0))
    ra, ca = (n, k) if trans == N_ else (k, n)
    lda, ldc = ra + dlda, n + dldc
    bufA, Av = _operand(ra, ca, lda, dtype, 100)
    view = lambda buf: buf[:ldc * n].view(n, ldc)[:, :n]  # [col, row]
    ones = torch.ones(n, n, dtype=torch.bool, device="cuda")
    tri = torch.triu(ones) if uplo == LO else torch.tril(ones)  # in the [col, row] view: lower = row >= col
    strict = tri & ~torch.eye(n, dtype=torch.bool, device="cuda")
    C0 = torch.full((ldc * n + 3,), SENTINEL, dtype=dtype, device="cuda")
    view(C0)[tri] = G.randmat(n, n, dtype, seed=900)[tri]
    view(C0).diagonal().imag.zero_()
    inside = torch.zeros_like(C0, dtype=torch.bool)
    view(inside)[tri] = True
    Cs, Cg = C0.clone(), C0.clone()
    work = torch.full((G.workSize_herk(n, k, N),), 0xA5, dtype=torch.uint8, device="cuda")
    G.herk(uplo, trans, n, k, alpha, bufA, lda, beta, Cs, ldc, N, fast, work)
    kernel = G.last_products_kernel()
    ct = G.COMPLEX_KARATSUBA_MULT
    G.gemm(trans, C_ if trans == N_ else N_, n, n, k, alpha, bufA, lda, bufA, lda, beta, Cg, ldc, N, fast,
           G.alloc_work(n, n, k, N, ct), ct)
    torch.cuda.synchronize()

    u8 = lambda x: x.contiguous().view(torch.uint8)
    diag = lambda buf: torch.view_as_real(view(buf).diagonal())
    assert u8(view(Cs)[strict]).equal(u8(view(Cg)[strict]))          # 1. gemm's bits in the strict triangle ...
    assert u8(diag(Cs)[:, 0]).equal(u8(diag(Cg)[:, 0]))              # ... and in the diagonal's real part
    assert not u8(diag(Cs)[:, 1]).any()                              # 2. diagonal imaginary parts: +0.0
    assert u8(Cs[~inside]).equal(u8(C0[~inside]))                    # 3. nothing else touched
    # 4. error against the complex128 product no larger than gemm's; X = op(A), n x k
    X = (Av.t() if trans == N_ else Av.conj()).to(torch.complex128)
    ref = (X @ X.conj().t()).t()[tri]                                # [col, row] like the views
    err = [((((view(c)[tri] - beta * view(C0)[tri]) / alpha).to(torch.complex128) - ref).abs().max() /
            ref.abs().max()).item() for c in (Cs, Cg)]
    print(f"max rel err herk {err[0]:.3e} gemm {err[1]:.3e}, products: {kernel}")
    assert err[0] <= err[1]
    assert "kernel" not in kw or kernel == kw["kernel"]              # 5. the products kernel
    assert not (kw.get("not_herk") and kernel in HERK)
