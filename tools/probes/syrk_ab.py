#!/usr/bin/env python3
"""A/B of the symmetric rank-k update: in one process, alternating per round, event-timed after warm-up,
  syrk      gemmul8.syrk (lower, op N): one split of A, the triangle's tiles, the triangular CRT
  gemm      gemmul8.gemm(N, T, A, A) into a scratch C (what a caller had before the entry point)
  dsyrk     hipblasDsyrk (lower, op N) through ctypes, where hipBLAS loads; reported, not gated
N = 14; fast mode except the shapes marked accurate.  One JSON line per shape and round to profiles/syrk/ab.jsonl
(or --out) with both calls' phase times; the spread of a variant over the rounds is the margin a difference has
to beat.  products_ratio = syrk products / gemm products, beside the unit-count ratio (T + 1) / 2T.

  python tools/probes/syrk_ab.py [--rounds 5] [--iters 20] [--out FILE]
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
SHAPES = [(1024, 1024, True), (2048, 2048, True), (4096, 4096, True), (8192, 8192, True), (8192, 1024, True),
          (4096, 4096, False)]
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


def vendor_dsyrk():
    """hipblasDsyrk(lower, op N) as a callable (n, k, A, C), or None where hipBLAS does not load"""
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
        rc = hb.hipblasDsyrk(handle, HIPBLAS_FILL_MODE_LOWER, HIPBLAS_OP_N, n, k, ctypes.byref(one),
                             ctypes.c_void_p(A.data_ptr()), n, ctypes.byref(zero), ctypes.c_void_p(C.data_ptr()), n)
        assert rc == 0, rc
    return call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "syrk", "ab.jsonl"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "syrk_ab needs a GPU"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    dsyrk = vendor_dsyrk()
    with open(a.out, "w") as out:
        for n, k, fast in SHAPES:
            A = G.randmat(n, k, seed=10)  # column-major n x k
            C, Cs = (torch.zeros((n, n), dtype=torch.float64, device="cuda") for _ in range(2))
            ws, wg = G.alloc_work(n, n, k, N), G.alloc_work(n, n, k, N)
            iters = a.iters if n < 8192 or k < 8192 else max(3, a.iters // 4)

            def syrk(pt=False):
                return G.syrk(G.FILL_LOWER, G.OP_N, n, k, 1.0, A, n, 0.0, C, n, N, fast, ws, phase_times=pt)

            def gemm(pt=False):
                return G.gemm(G.OP_N, G.OP_T, n, n, k, 1.0, A, n, A, n, 0.0, Cs, n, N, fast, wg, phase_times=pt)

            for _ in range(2):
                syrk(), gemm()
            T = (n + 255) // 256
            for r in range(a.rounds):
                row = {"n": n, "k": k, "N": N, "fast": fast, "round": r, "syrk_us": timed(syrk, iters),
                       "gemm_us": timed(gemm, iters)}
                if dsyrk:
                    row["hipblas_dsyrk_us"] = timed(lambda: dsyrk(n, k, A, Cs), iters)
                row["syrk_phase_ns"] = syrk(True)
                row["products_kernel"] = G.last_products_kernel()
                row["gemm_phase_ns"] = gemm(True)
                row["products_ratio"] = row["syrk_phase_ns"][1] / row["gemm_phase_ns"][1]
                row["unit_ratio"] = (T + 1) / (2 * T)
                line = json.dumps(row)
                print(line, flush=True)
                out.write(line + "\n")
                out.flush()


if __name__ == "__main__":
    main()
