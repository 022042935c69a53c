"""gemm_strided_batched against gemm element by element: same bits, no larger error, nothing written outside C."""
import pytest
import torch

import gemmul8 as G

pytestmark = pytest.mark.gpu
N_, T_ = G.OP_N, G.OP_T
SENTINEL = -7.25

# m, n, k, batch, N, opA, opB, kwargs
CASES = [
    (200, 136, 100, 3, 14, N_, N_, {}),                                     # ragged, 2 k-steps: one-unit launch
    (300, 520, 448, 2, 8, T_, N_, dict(pad=(5, 9, 1000, 777), alpha=0.5, beta=-1.5)),  # tiles, strided A, padding
    (256, 256, 384, 56, 14, N_, T_, dict(kernel="gemm_i8_batched_kernel")),  # 784 units: rounds of the queues
    (130, 260, 390, 64, 14, N_, N_, dict(kernel="gemm_i8_batched_kernel")),  # mostly-empty quadrants
    (256, 256, 448, 5, 14, N_, N_, dict(share_a=True)),                     # stride_a = 0
    (200, 136, 100, 1, 2, N_, N_, {}),                                      # batch 1, fewest moduli
    (150, 100, 2100, 2, 14, N_, N_, {}),                                    # k beyond the hot path: host loop
    (150, 100, 200, 2, 10, N_, N_, dict(dtype=torch.float32, fast=False)),  # f32, accurate: host loop
]


def _operand(rows, cols, ld, stride, count, dtype, seed):
    """`count` column-major rows x cols matrices, leading dimension ld, `stride` elements apart"""
    buf = torch.zeros(max(count - 1, 0) * stride + ld * cols, dtype=dtype, device="cuda")
    views = [buf[b * stride:b * stride + ld * cols].view(cols, ld)[:, :rows] for b in range(count)]
    for b, v in enumerate(views):
        v.copy_(G.randmat(rows, cols, dtype, seed=seed + b))
    return buf, views


@pytest.mark.parametrize("m,n,k,batch,N,opA,opB,kw", CASES)
def test_batched_matches_per_element(m, n, k, batch, N, opA, opB, kw):
    dtype, fast = kw.get("dtype", torch.float64), kw.get("fast", True)
    alpha, beta = kw.get("alpha", 1.0), kw.get("beta", 0.0)
    dlda, dldc, dsa, dsc = kw.get("pad", (0, 0, 0, 0))
    ra, ca = (m, k) if opA == N_ else (k, m)
    rb, cb = (k, n) if opB == N_ else (n, k)
    lda, ldb, ldc = ra + dlda, rb, m + dldc
    sa = 0 if kw.get("share_a") else lda * ca + dsa
    sb, sc = ldb * cb, ldc * n + dsc
    bufA, Av = _operand(ra, ca, lda, sa, 1 if sa == 0 else batch, dtype, 100)
    bufB, Bv = _operand(rb, cb, ldb, sb, batch, dtype, 500)
    C0 = torch.full(((batch - 1) * sc + ldc * n + 3,), SENTINEL, dtype=dtype, device="cuda")
    inside = torch.zeros_like(C0, dtype=torch.bool)
    Cv = lambda buf: [buf[b * sc:b * sc + ldc * n].view(n, ldc)[:, :m] for b in range(batch)]
    for b, v in enumerate(Cv(C0)):
        v.copy_(G.randmat(m, n, dtype, seed=900 + b))
    for v in Cv(inside):
        v.fill_(True)

    Cb, Ce = C0.clone(), C0.clone()
    work = torch.empty(G.workSize_strided_batched(m, n, k, N, batch), dtype=torch.uint8, device="cuda")
    G.gemm_strided_batched(opA, opB, m, n, k, alpha, bufA, lda, sa, bufB, ldb, sb, beta, Cb, ldc, sc, batch, N, fast, work)
    kernel = G.last_products_kernel()
    w1 = G.alloc_work(m, n, k, N)
    for b in range(batch):
        G.gemm(opA, opB, m, n, k, alpha, bufA[b * sa:], lda, bufB[b * sb:], ldb, beta, Ce[b * sc:], ldc, N, fast, w1)
    torch.cuda.synchronize()

    assert "kernel" not in kw or kernel == kw["kernel"]
    # 3. every element outside the m x n blocks keeps its sentinel
    assert torch.equal(Cb[~inside].view(torch.uint8), C0[~inside].view(torch.uint8))
    for b, (cb_, ce_, c0_) in enumerate(zip(Cv(Cb), Cv(Ce), Cv(C0))):
        # 1. the same bits as gemm on element b
        assert torch.equal(cb_.contiguous().view(torch.uint8), ce_.contiguous().view(torch.uint8)), f"element {b}"
        # 2. error against the double-double product no larger than the per-element call's
        a_ = Av[0 if sa == 0 else b]
        opa = (a_ if opA == N_ else a_.t()).double().contiguous()  # column-major m x k as a (k, m) tensor
        opb = (Bv[b] if opB == N_ else Bv[b].t()).double().contiguous()
        C1, C2 = G.dd_gemm(opa, opb, m, n, k)
        err = [G.relerr_dd(((c.double() - beta * c0_.double()) / alpha).contiguous(), C1, C2)[0] for c in (cb_, ce_)]
        print(f"element {b}: max rel err batched {err[0]:.3e} per-element {err[1]:.3e}")
        assert err[0] <= err[1]


def test_bmm_matches_matmul():
    A = torch.randn(3, 70, 90, dtype=torch.float64, device="cuda")
    B = torch.randn(3, 90, 50, dtype=torch.float64, device="cuda")
    C = G.bmm(A, B)
    for b in range(3):
        assert torch.equal(C[b], G.matmul(A[b], B[b]))
