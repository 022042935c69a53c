"""Host-only checks of the complex TRMM entry points: workspace size, argument errors."""
import pytest
import torch

import gemmul8 as G

E_TYPES, E_OP, E_SIZE = -2, -3, -4
Z, D = G.C_64F, G.R_64F


def _call(trans=0, m=8, n=4, ta=Z, tb=Z, tc=Z, lda=8, ldb=8, ldc=8):
    # null device pointers: every case below returns before anything could touch them
    return G.lib.gemmul8_trmm(None, 0, 0, trans, 0, m, n, ta, tb, tc, None, None, lda, None, ldb, None, ldc, 14, 1,
                              None, None)


@pytest.mark.parametrize("m,n,N", [(200, 130, 12), (1300, 1000, 14), (300, 520, 2), (3072, 3072, 12), (4096, 4096, 8)])
def test_work_size(m, n, N):
    ct = G.COMPLEX_KARATSUBA_MULT
    for side, ka in ((G.SIDE_LEFT, m), (G.SIDE_RIGHT, n)):
        assert G.workSize_trmm(side, m, n, N, torch.complex128) == G.workSize_trmm(side, m, n, N, torch.complex64) > 0
        assert G.workSize_trmm(side, m, n, N) == G.workSize(m, n, ka, N)     # the real form is unchanged
        if G.layout(m, n, ka, N, ct)["nsub"] == 3:                            # gemm itself takes the Karatsuba geometry
            assert G.workSize_trmm(side, m, n, N, torch.complex128) == G.workSize(m, n, ka, N, ct)
    assert G.layout(m, n, m, N, ct)["nsub"] == (3 if m >= 3072 else 1)        # both branches above are taken


def test_argument_checks_enqueue_nothing():
    assert _call(trans=G.OP_C, m=0, lda=1, ldb=1, ldc=1) == 0               # complex, op C, nothing to do
    assert _call(tb=D, tc=D) == E_TYPES and _call(ta=D) == E_TYPES and _call(tc=G.R_32F) == E_TYPES
    assert _call(trans=G.OP_C, ta=D, tb=D, tc=D) == E_OP                    # op C stays complex-only
    assert _call(lda=7) == E_SIZE and _call(trans=G.OP_C, ldc=7) == E_SIZE
