#!/usr/bin/env python3
"""A/B of the triangular matrix multiply: in one process, alternating per round, event-timed after warm-up,
  trmm      gemmul8.trmm (lower, op N, non-unit): the triangle's half of the split, the k-clipped products, gemm's CRT
  gemm      gemmul8.gemm on the explicitly masked dense A into a scratch C (what a caller had before the entry
            point, without the masking pass that caller also paid)
  dtrmm     hipblasDtrmm / hipblasZtrmm (out of place) through ctypes, where hipBLAS loads; reported, not gated
--dtype complex128: the complex form (Karatsuba k-clipped products) against gemm under COMPLEX_KARATSUBA_MULT, rows to
profiles/trmm/ab_complex.jsonl.
N = 14; fast mode except the shapes marked accurate; side left except the shape marked right.  One JSON line per shape
and round to profiles/trmm/ab.jsonl (or --out) with both calls' phase times; the spread of a variant over the rounds
is the margin a difference has to beat.  products_ratio = trmm products / gemm products, beside the unit-work ratio
sum_t min(4 (t + 1), K) / (T K).

  python tools/probes/trmm_ab.py [--rounds 5] [--iters 20] [--dtype float64|complex128] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "mixed-gemmul8_amd"))
import gemmul8 as G  # noqa: E402

# m, n, side, fast
SHAPES = [(1024, 1024, G.SIDE_LEFT, True), (2048, 2048, G.SIDE_LEFT, True), (4096, 4096, G.SIDE_LEFT, True),
          (8192, 8192, G.SIDE_LEFT, True), (8192, 1024, G.SIDE_LEFT, True), (1024, 8192, G.SIDE_RIGHT, True),
          (4096, 4096, G.SIDE_LEFT, False)]
N = 14


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters  # us per call


def vendor_dtrmm(cplx):
    """hipblasDtrmm / hipblasZtrmm(lower, op N, non-unit; the out-of-place form) as a callable
    (side, m, n, A, lda, B, C), or None where hipBLAS does not load"""
    hb = None
    for name in ("libhipblas.so", "/opt/rocm/lib/libhipblas.so"):
        try:
            hb = ctypes.CDLL(name)
            break
        except OSError:
            pass
    handle = ctypes.c_void_p()
    if hb is None or hb.hipblasCreate(ctypes.byref(handle)) != 0:
        return None
    one = (ctypes.c_double * 2)(1.0, 0.0)
    fn = hb.hipblasZtrmm if cplx else hb.hipblasDtrmm
    HIPBLAS_SIDE = {G.SIDE_LEFT: 141, G.SIDE_RIGHT: 142}
    HIPBLAS_FILL_MODE_LOWER, HIPBLAS_OP_N, HIPBLAS_DIAG_NON_UNIT = 122, 111, 131

    def call(side, m, n, A, lda, B, C):
        hb.hipblasSetStream(handle, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        rc = fn(handle, HIPBLAS_SIDE[side], HIPBLAS_FILL_MODE_LOWER, HIPBLAS_OP_N, HIPBLAS_DIAG_NON_UNIT, m, n,
                ctypes.byref(one), ctypes.c_void_p(A.data_ptr()), lda, ctypes.c_void_p(B.data_ptr()), m,
                ctypes.c_void_p(C.data_ptr()), m)
        assert rc == 0, rc
    return call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--dtype", choices=("float64", "complex128"), default="float64")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "trmm_ab needs a GPU"
    cplx = a.dtype == "complex128"
    dtype = torch.complex128 if cplx else torch.float64
    ct = G.COMPLEX_KARATSUBA_MULT if cplx else G.REAL_DEFAULT
    a.out = a.out or os.path.join(ROOT, "profiles", "trmm", "ab_complex.jsonl" if cplx else "ab.jsonl")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    dtrmm = vendor_dtrmm(cplx)
    with open(a.out, "w") as out:
        for m, n, side, fast in SHAPES:
            na = m if side == G.SIDE_LEFT else n
            # column-major lower triangle = upper triangle of the [col, row] view; Ad is the masked dense form
            Ad = torch.triu(G.randmat(na, na, dtype, seed=10))
            B = G.randmat(m, n, dtype, seed=11)
            C, Cs = (torch.zeros((n, m), dtype=dtype, device="cuda") for _ in range(2))
            wt = torch.empty(G.workSize_trmm(side, m, n, N, dtype), dtype=torch.uint8, device="cuda")
            wg = G.alloc_work(m, n, na, N, ct)
            iters = a.iters if m * n < 8192 * 8192 else max(3, a.iters // 4)

            def trmm(pt=False):
                return G.trmm(side, G.FILL_LOWER, G.OP_N, G.DIAG_NON_UNIT, m, n, 1.0, Ad, na, B, m, C, m, N, fast, wt,
                              phase_times=pt)

            def gemm(pt=False):
                if side == G.SIDE_LEFT:
                    return G.gemm(G.OP_N, G.OP_N, m, n, m, 1.0, Ad, na, B, m, 0.0, Cs, m, N, fast, wg, ct,
                                  phase_times=pt)
                return G.gemm(G.OP_N, G.OP_N, m, n, n, 1.0, B, m, Ad, na, 0.0, Cs, m, N, fast, wg, ct, phase_times=pt)

            for _ in range(2):
                trmm(), gemm()
            torch.cuda.synchronize()
            same = bool(C.view(torch.uint8).equal(Cs.view(torch.uint8)))
            T, K = (na + 255) // 256, (na + 63) // 64
            for r in range(a.rounds):
                row = {"m": m, "n": n, "dtype": a.dtype, "side": "right" if side == G.SIDE_RIGHT else "left", "N": N,
                       "fast": fast,
                       "round": r, "same_bits": same, "trmm_us": timed(trmm, iters), "gemm_us": timed(gemm, iters)}
                if dtrmm:
                    row["hipblas_dtrmm_us"] = timed(lambda: dtrmm(side, m, n, Ad, na, B, Cs), iters)
                row["trmm_phase_ns"] = trmm(True)
                row["products_kernel"] = G.last_products_kernel()
                row["gemm_phase_ns"] = gemm(True)
                row["products_ratio"] = row["trmm_phase_ns"][1] / row["gemm_phase_ns"][1]
                row["unit_work_ratio"] = sum(min(4 * (t + 1), K) for t in range(T)) / (T * K)
                line = json.dumps(row)
                print(line, flush=True)
                out.write(line + "\n")
                out.flush()


if __name__ == "__main__":
    main()
