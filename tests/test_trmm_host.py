"""Host-only checks of the TRMM entry points: exports, workspace size, argument errors."""
import pytest

import gemmul8 as G

E_MODULI, E_TYPES, E_OP, E_SIZE = -1, -2, -3, -4


def _call(side=0, uplo=0, trans=0, diag=0, m=8, n=4, ta=0, tb=0, tc=0, lda=8, ldb=8, ldc=8, N=14):
    # null device pointers: every case below returns before anything could touch them
    return G.lib.gemmul8_trmm(None, side, uplo, trans, diag, m, n, ta, tb, tc, None, None, lda, None, ldb, None, ldc,
                              N, 1, None, None)


def test_exports():
    assert G.lib.gemmul8_work_size_trmm and G.lib.gemmul8_trmm
    assert callable(G.trmm) and callable(G.workSize_trmm)
    assert (G.SIDE_LEFT, G.SIDE_RIGHT, G.DIAG_NON_UNIT, G.DIAG_UNIT) == (0, 1, 0, 1)


@pytest.mark.parametrize("m,n,N", [(200, 130, 14), (2600, 1300, 8), (300, 520, 2)])
def test_work_size_is_the_equivalent_gemms(m, n, N):
    assert G.workSize_trmm(G.SIDE_LEFT, m, n, N) == G.workSize(m, n, m, N) > 0
    assert G.workSize_trmm(G.SIDE_RIGHT, m, n, N) == G.workSize(m, n, n, N) > 0


def test_argument_errors_enqueue_nothing():
    assert _call(ta=G.C_64F) == E_TYPES and _call(tb=G.C_32F) == E_TYPES and _call(tc=G.C_64F) == E_TYPES
    assert _call(trans=G.OP_C) == E_OP and _call(side=2) == E_OP and _call(uplo=2) == E_OP and _call(diag=2) == E_OP
    assert _call(N=1) == E_MODULI and _call(N=21) == E_MODULI
    assert _call(lda=7) == E_SIZE and _call(ldb=7) == E_SIZE and _call(ldc=7) == E_SIZE
    assert _call(side=1, lda=3, ldb=8, ldc=8) == E_SIZE                  # side right: A is n x n, lda >= n
    assert _call(m=0, lda=1, ldb=1, ldc=1) == 0 and _call(n=0) == 0      # nothing to do
