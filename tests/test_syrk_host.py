"""Host-only checks of the SYRK entry points: exports, workspace size, argument errors."""
import pytest

import gemmul8 as G

E_MODULI, E_TYPES, E_OP, E_SIZE = -1, -2, -3, -4


def _call(uplo=0, trans=0, n=8, k=8, ta=0, tc=0, lda=8, ldc=8, N=14):
    # null device pointers: every case below returns before anything could touch them
    return G.lib.gemmul8_syrk(None, uplo, trans, n, k, ta, tc, None, None, lda, None, None, ldc, N, 1, None, None)


def test_exports():
    assert G.lib.gemmul8_work_size_syrk and G.lib.gemmul8_syrk
    assert callable(G.syrk) and callable(G.workSize_syrk) and (G.FILL_LOWER, G.FILL_UPPER) == (0, 1)


@pytest.mark.parametrize("n,k,N", [(200, 100, 14), (2600, 390, 8), (260, 66000, 2)])
def test_work_size_is_the_square_gemms(n, k, N):
    assert G.workSize_syrk(n, k, N) == G.workSize(n, n, k, N) > 0


def test_argument_errors_enqueue_nothing():
    assert _call(ta=G.C_64F) == E_TYPES and _call(tc=G.C_32F) == E_TYPES
    assert _call(trans=G.OP_C) == E_OP and _call(uplo=2) == E_OP
    assert _call(N=1) == E_MODULI and _call(N=21) == E_MODULI
    assert _call(lda=7) == E_SIZE and _call(ldc=7) == E_SIZE
    assert _call(trans=G.OP_T, n=16, k=8, lda=7, ldc=16) == E_SIZE  # k x n operand: lda >= k
    assert _call(n=0, lda=1, ldc=1) == 0          # nothing to do
