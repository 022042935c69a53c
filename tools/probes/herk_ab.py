#!/usr/bin/env python3
"""A/B of the Hermitian rank-k update: in one process, alternating per round, event-timed after warm-up,
  herk      gemmul8.herk (lower, op N): gemm's split over the Karatsuba geometry, the triangle's tiles of the three
            sub-products, the triangular complex CRT
  gemm      gemmul8.gemm(N, C, A, A) into a scratch C (what a caller had before the entry point)
  zherk     hipblasZherk (lower, op N) through ctypes, where hipBLAS loads; reported, not gated
N = 12, complex128; fast mode except the shapes marked accurate.  One JSON line per shape and round to
profiles/herk/ab.jsonl (or --out) with both calls' phase times; the spread of a variant over the rounds is the margin
a difference has to beat.  products_ratio = herk products / gemm products, beside the unit-count ratio (T + 1) / 2T
(gemm multiplies 3 T^2 Karatsuba or 4 T^2 big-matrix tiles per modulus: "gemm_kara" says which).

  python tools/probes/herk_ab.py [--rounds 5] [--iters 20] [--out FILE]
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

# n, k, fast
SHAPES = [(1024, 1024, True), (2048, 2048, True), (4096, 4096, True), (8192, 1024, True), (4096, 4096, False)]
N = 12
CT = G.COMPLEX_KARATSUBA_MULT


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


def vendor_zherk():
    """hipblasZherk(lower, op N) as a callable (n, k, A, C), or None where hipBLAS does not load"""
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
    one, zero = ctypes.c_double(1.0), ctypes.c_double(0.0)
    HIPBLAS_FILL_MODE_LOWER, HIPBLAS_OP_N = 122, 111

    def call(n, k, A, C):
        hb.hipblasSetStream(handle, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        rc = hb.hipblasZherk(handle, HIPBLAS_FILL_MODE_LOWER, HIPBLAS_OP_N, n, k, ctypes.byref(one),
                             ctypes.c_void_p(A.data_ptr()), n, ctypes.byref(zero), ctypes.c_void_p(C.data_ptr()), n)
        assert rc == 0, rc
    return call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "herk", "ab.jsonl"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "herk_ab needs a GPU"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    zherk = vendor_zherk()
    with open(a.out, "w") as out:
        for n, k, fast in SHAPES:
            A = G.randmat(n, k, torch.complex128, seed=10)  # column-major n x k
            C, Cs = (torch.zeros((n, n), dtype=torch.complex128, device="cuda") for _ in range(2))
            wh = torch.empty(G.workSize_herk(n, k, N), dtype=torch.uint8, device="cuda")
            wg = G.alloc_work(n, n, k, N, CT)

            def herk(pt=False):
                return G.herk(G.FILL_LOWER, G.OP_N, n, k, 1.0, A, n, 0.0, C, n, N, fast, wh, phase_times=pt)

            def gemm(pt=False):
                return G.gemm(G.OP_N, G.OP_C, n, n, k, 1.0, A, n, A, n, 0.0, Cs, n, N, fast, wg, CT, phase_times=pt)

            for _ in range(2):
                herk(), gemm()
            T = (n + 255) // 256
            for r in range(a.rounds):
                row = {"n": n, "k": k, "N": N, "fast": fast, "round": r, "herk_us": timed(herk, a.iters),
                       "gemm_us": timed(gemm, a.iters)}
                if zherk:
                    row["hipblas_zherk_us"] = timed(lambda: zherk(n, k, A, Cs), a.iters)
                row["herk_phase_ns"] = herk(True)
                row["products_kernel"] = G.last_products_kernel()
                row["gemm_phase_ns"] = gemm(True)
                row["gemm_kara"] = G.layout(n, n, k, N, CT)["nsub"] == 3
                row["products_ratio"] = row["herk_phase_ns"][1] / row["gemm_phase_ns"][1]
                row["unit_ratio"] = (T + 1) / (2 * T)
                line = json.dumps(row)
                print(line, flush=True)
                out.write(line + "\n")
                out.flush()


if __name__ == "__main__":
    main()
