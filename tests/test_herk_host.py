"""Host-only checks of the HERK entry points: exports, workspace size, argument errors."""
import pytest

import gemmul8 as G

E_MODULI, E_TYPES, E_OP, E_SIZE = -1, -2, -3, -4


def _call(uplo=0, trans=0, n=8, k=8, ta=G.C_64F, tc=G.C_64F, lda=8, ldc=8, N=12):
    # null device pointers: every case below returns before anything could touch them
    return G.lib.gemmul8_herk(None, uplo, trans, n, k, ta, tc, None, None, lda, None, None, ldc, N, 1, None, None)


def test_exports():
    assert G.lib.gemmul8_work_size_herk and G.lib.gemmul8_herk
    assert callable(G.herk) and callable(G.workSize_herk)


@pytest.mark.parametrize("n,k,N", [(200, 100, 12), (1300, 390, 14), (260, 66000, 4)])
def test_work_size_positive(n, k, N):
    assert G.workSize_herk(n, k, N) > 0


def test_work_size_is_the_karatsuba_gemms():
    # gemm itself takes the Karatsuba geometry from k = 3072, m = 1024; herk takes it at every shape
    assert G.layout(1024, 1024, 3072, 12, G.COMPLEX_KARATSUBA_MULT)["nsub"] == 3
    assert G.workSize_herk(1024, 3072, 12) == G.workSize(1024, 1024, 3072, 12, G.COMPLEX_KARATSUBA_MULT)


def test_argument_errors_enqueue_nothing():
    assert _call(ta=G.R_64F) == E_TYPES and _call(tc=G.R_32F) == E_TYPES
    assert _call(trans=G.OP_T) == E_OP and _call(uplo=2) == E_OP
    assert _call(N=1) == E_MODULI and _call(N=21) == E_MODULI
    assert _call(lda=7) == E_SIZE and _call(ldc=7) == E_SIZE
    assert _call(trans=G.OP_C, n=16, k=8, lda=7, ldc=16) == E_SIZE  # k x n operand: lda >= k
    assert _call(trans=G.OP_C, n=16, k=8, lda=8, ldc=15) == E_SIZE
    assert _call(n=0, lda=1, ldc=1) == 0          # nothing to do
