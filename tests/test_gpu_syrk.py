"""syrk against gemm(A, A^T): the triangle carries gemm's bits, nothing outside it is touched, lower is the
transpose of upper, and the error against the double-double product is no larger than gemm's."""
import pytest
import torch

import gemmul8 as G

pytestmark = pytest.mark.gpu
N_, T_, LO, UP = G.OP_N, G.OP_T, G.FILL_LOWER, G.FILL_UPPER
SENTINEL = -7.25

# n, k, N, uplo, trans, kwargs
CASES = [
    (200, 100, 14, LO, N_, dict(kernel="gemm_i8_syrk_onetile_kernel")),  # one diagonal tile, ragged, 2 k-steps
    (520, 448, 8, UP, T_, dict(pad=(5, 9), alpha=0.5, beta=-1.5)),       # 3 tile rows, 7 k-steps, clipped last tile
    (2600, 390, 14, LO, N_, dict(kernel="gemm_i8_syrk_kernel")),         # 924 units: claims, clipped last band
    (2600, 390, 14, UP, N_, dict(kernel="gemm_i8_syrk_kernel", beta=1.0)),  # the swapped decode, persistent
    (300, 200, 2, LO, T_, {}),                                           # fewest moduli
    (300, 200, 10, LO, N_, dict(dtype=torch.float32)),                   # f32 in and out
    (300, 200, 10, UP, N_, dict(fast=False)),                            # accurate: two-operand split
    (260, 66000, 14, LO, N_, dict(kernel="gemm_i8_kernel")),             # k_pad > 2^16: all tiles + triangular CRT
]


def _operand(rows, cols, ld, dtype, seed):
    """column-major rows x cols matrix with leading dimension ld: (flat buffer, (cols, rows) view)"""
    buf = torch.zeros(ld * cols, dtype=dtype, device="cuda")
    view = buf.view(cols, ld)[:, :rows]
    view.copy_(G.randmat(rows, cols, dtype, seed=seed))
    return buf, view


@pytest.mark.parametrize("n,k,N,uplo,trans,kw", CASES)
def test_syrk_matches_gemm_triangle(n, k, N, uplo, trans, kw):
    dtype, fast = kw.get("dtype", torch.float64), kw.get("fast", True)
    alpha, beta = kw.get("alpha", 1.0), kw.get("beta", 0.0)
    dlda, dldc = kw.get("pad", (0, 0))
    ra, ca = (n, k) if trans == N_ else (k, n)
    lda, ldc = ra + dlda, n + dldc
    bufA, Av = _operand(ra, ca, lda, dtype, 100)
    view = lambda buf: buf[:ldc * n].view(n, ldc)[:, :n]  # [col, row]
    # triangle masks in the [col, row] view: lower = row >= col
    ones = torch.ones(n, n, dtype=torch.bool, device="cuda")
    tri = {LO: torch.triu(ones), UP: torch.tril(ones)}
    other = UP if uplo == LO else LO
    Cin = G.randmat(n, n, dtype, seed=900)

    def c0_for(ul, vals):
        buf = torch.full((ldc * n + 3,), SENTINEL, dtype=dtype, device="cuda")
        view(buf)[tri[ul]] = vals[tri[ul]]
        inside = torch.zeros_like(buf, dtype=torch.bool)
        view(inside)[tri[ul]] = True
        return buf, inside

    C0, inside = c0_for(uplo, Cin)
    C0t, _ = c0_for(other, Cin.t())
    Cs, Cg, Ct = C0.clone(), C0.clone(), C0t.clone()
    works = [torch.full((G.workSize_syrk(n, k, N),), 0xA5, dtype=torch.uint8, device="cuda") for _ in range(2)]
    G.syrk(uplo, trans, n, k, alpha, bufA, lda, beta, Cs, ldc, N, fast, works[0])
    kernel = G.last_products_kernel()
    G.syrk(other, trans, n, k, alpha, bufA, lda, beta, Ct, ldc, N, fast, works[1])
    G.gemm(trans, T_ if trans == N_ else N_, n, n, k, alpha, bufA, lda, bufA, lda, beta, Cg, ldc, N, fast,
           G.alloc_work(n, n, k, N))
    torch.cuda.synchronize()

    u8 = lambda x: x.contiguous().view(torch.uint8)
    assert u8(Cs[inside]).equal(u8(Cg[inside]))                        # 1. gemm's bits in the triangle
    assert u8(Cs[~inside]).equal(u8(C0[~inside]))                      # 2. nothing else touched
    assert u8(view(Cs)[tri[uplo]]).equal(u8(view(Ct).t()[tri[uplo]]))  # 3. the other uplo is the transpose
    # 4. error against the double-double product no larger than gemm's
    X = (Av if trans == N_ else Av.t()).double().contiguous()          # op(A), column-major n x k
    C1, C2 = G.dd_gemm(X, X.t().contiguous(), n, n, k)
    m = tri[uplo]
    err = [G.relerr_dd(((view(c)[m].double() - beta * view(C0)[m].double()) / alpha).contiguous(), C1[m].contiguous(),
                       C2[m].contiguous())[0] for c in (Cs, Cg)]
    print(f"max rel err syrk {err[0]:.3e} gemm {err[1]:.3e}, products: {kernel}")
    assert err[0] <= err[1]
    assert "kernel" not in kw or kernel == kw["kernel"]                # 5. the products kernel
