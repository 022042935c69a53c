"""Host-only checks of the strided-batched entry points: exports, workspace size, argument errors."""
import pytest

import gemmul8 as G

E_MODULI, E_SIZE = -1, -4


def _call(m=8, n=8, k=8, lda=8, ldc=8, stride_c=64, batch=2, N=14):
    # null device pointers: every case below returns before anything could touch them
    return G.lib.gemmul8_gemm_strided_batched(None, 0, 0, m, n, k, 0, 0, 0, None, None, lda, 64, None, 8, 64, None, None,
                                              ldc, stride_c, batch, N, 1, None, 0, None)


def test_exports():
    assert G.lib.gemmul8_work_size_strided_batched and G.lib.gemmul8_gemm_strided_batched
    assert callable(G.gemm_strided_batched) and callable(G.workSize_strided_batched) and callable(G.bmm)


@pytest.mark.parametrize("m,n,k,N", [(200, 136, 100, 14), (1024, 1024, 1024, 8), (130, 260, 2100, 2)])
def test_work_size_linear_in_batch(m, n, k, N):
    w = [G.workSize_strided_batched(m, n, k, N, b) for b in (1, 2, 3, 64)]
    assert w[0] >= G.workSize(m, n, k, N)
    step = w[1] - w[0]
    assert step > 0 and w[2] == w[0] + 2 * step and w[3] == w[0] + 63 * step


def test_argument_errors_enqueue_nothing():
    assert _call(stride_c=63) == E_SIZE           # stride_c < ldc * n with batch > 1
    assert _call(lda=7) == E_SIZE and _call(ldc=7) == E_SIZE  # prepare()'s checks
    assert _call(N=1) == E_MODULI
    assert _call(batch=0) == 0                    # nothing to do
    assert _call(stride_c=63, batch=0) == 0
