"""Complex trmm against gemm on the explicit dense form of the triangle: C carries gemm's bits although the
unreferenced part of A holds NaN in both parts, nothing outside C is touched, in place equals out of place, and the
error against the complex128 product is no larger than gemm's."""
import pytest
import torch

import gemmul8 as G

pytestmark = pytest.mark.gpu
N_, T_, C_, LO, UP, L_, R_, NU, UN = G.OP_N, G.OP_T, G.OP_C, G.FILL_LOWER, G.FILL_UPPER, G.SIDE_LEFT, G.SIDE_RIGHT, 0, 1
SENTINEL = complex(-7.25, 3.5)
KARA = ("gemm_i8_trmm_kara_kernel", "gemm_i8_trmm_kara_onetile_kernel")

# side, uplo, trans, diag, m, n, N, kwargs
CASES = [
    (L_, LO, N_, NU, 200, 130, 12, dict(kernel=KARA[1])),        # one ragged tile, 4 k-steps; gemm itself takes the
                                                                 # big-matrix geometry here
    (L_, UP, C_, UN, 520, 300, 8, dict(alpha=0.5 - 0.25j, pad=(5, 9))),  # conj + transpose decode, unit diagonal,
                                                                 # k <= t: 4 / 8 / 9 steps
    (L_, UP, T_, NU, 520, 300, 14, {}),                          # plain transpose of a complex triangle, k >= t
    (R_, LO, N_, UN, 300, 520, 14, {}),                          # the clip on tn, triangle in the B role
    (R_, UP, C_, NU, 300, 520, 14, {}),
    (L_, LO, N_, NU, 1300, 1000, 14, dict(kernel=KARA[0])),      # 6 x 4 tiles x 42 planes = 1008 units, 21 k-steps:
                                                                 # claims, widened units, band order over 3 N planes
    (L_, UP, N_, NU, 1300, 1000, 14, dict(kernel=KARA[0])),      # kbeg > 0 through the cursor jump
    (L_, LO, N_, NU, 300, 300, 10, dict(dtype=torch.complex64)),  # complex64 in and out
    (L_, LO, C_, NU, 300, 300, 10, dict(fast=False)),            # accurate: masked magnitudes in the bound product
    (L_, LO, N_, NU, 520, 300, 14, dict(inplace=True)),          # C is B
    (L_, LO, N_, NU, 520, 300, 14, dict(flat=True)),             # all-tiles fallback over the same layout
]


@pytest.mark.parametrize("side,uplo,trans,diag,m,n,N,kw", CASES)
def test_ctrmm_matches_gemm_on_the_dense_triangle(side, uplo, trans, diag, m, n, N, kw, monkeypatch):
    dtype, fast, alpha = kw.get("dtype", torch.complex128), kw.get("fast", True), kw.get("alpha", 1.0)
    if kw.get("flat"):
        monkeypatch.setenv("GEMMUL8_FORCE_FLAT_DMA", "1")  # read per call
    dlda, dld = kw.get("pad", (0, 0))
    na = m if side == L_ else n
    lda, ld = na + dlda, m + dld  # ldb == ldc
    # A: NaN + NaN i wherever trmm must not look (the other triangle, a unit diagonal, the lda padding); views are
    # [col, row]
    ones = torch.ones(na, na, dtype=torch.bool, device="cuda")
    keep = torch.triu(ones, diag) if uplo == LO else torch.tril(ones, -diag)
    Ad = G.randmat(na, na, dtype, seed=100) * keep  # the dense form, column-major na x na
    if diag == UN:
        Ad.fill_diagonal_(1.0)
    bufA = torch.full((lda * na,), complex(float("nan"), float("nan")), dtype=dtype, device="cuda")
    bufA.view(na, lda)[:, :na][keep] = Ad[keep]
    view = lambda buf: buf[:ld * n].view(n, ld)[:, :m]
    bufB = torch.full((ld * n + 3,), SENTINEL, dtype=dtype, device="cuda")
    view(bufB).copy_(G.randmat(m, n, dtype, seed=200))
    inside = torch.zeros_like(bufB, dtype=torch.bool)
    view(inside)[:] = True
    Ct, Cg = (torch.full_like(bufB, SENTINEL) for _ in range(2))
    work = torch.full((G.workSize_trmm(side, m, n, N, dtype),), 0xA5, dtype=torch.uint8, device="cuda")

    G.trmm(side, uplo, trans, diag, m, n, alpha, bufA, lda, bufB, ld, Ct, ld, N, fast, work)
    kernel = G.last_products_kernel()
    ct = G.COMPLEX_KARATSUBA_MULT
    if side == L_:
        G.gemm(trans, N_, m, n, m, alpha, Ad, na, bufB, ld, 0.0, Cg, ld, N, fast, G.alloc_work(m, n, m, N, ct), ct)
    else:
        G.gemm(N_, trans, m, n, n, alpha, bufB, ld, Ad, na, 0.0, Cg, ld, N, fast, G.alloc_work(m, n, n, N, ct), ct)
    torch.cuda.synchronize()

    u8 = lambda x: x.contiguous().view(torch.uint8)
    assert u8(Ct[inside]).equal(u8(Cg[inside]))             # 1. gemm's bits (so no NaN leaked)
    assert bool((Ct[~inside] == SENTINEL).all())            # 2. ldc padding and the tail untouched
    # 3. error against the complex128 product no larger than gemm's; the views are the transposes
    At = Ad.to(torch.complex128)
    X = {N_: At.t(), T_: At, C_: At.conj()}[trans]          # op(A)
    Bd = view(bufB).to(torch.complex128).t()
    ref = (X @ Bd if side == L_ else Bd @ X).t()
    err = [((view(c).to(torch.complex128) / alpha - ref).abs().max() / ref.abs().max()).item() for c in (Ct, Cg)]
    print(f"max rel err trmm {err[0]:.3e} gemm {err[1]:.3e}, products: {kernel}")
    assert err[0] <= err[1]
    assert "kernel" not in kw or kernel == kw["kernel"]    # 4. the products kernel
    assert not (kw.get("flat") and kernel in KARA)
    if kw.get("inplace"):                                   # 5. C is B: the out-of-place bytes
        G.trmm(side, uplo, trans, diag, m, n, alpha, bufA, lda, bufB, ld, bufB, ld, N, fast, work)
        torch.cuda.synchronize()
        assert u8(bufB).equal(u8(Ct))
