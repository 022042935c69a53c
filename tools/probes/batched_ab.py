#!/usr/bin/env python3
"""A/B of the strided-batched call: in one process, alternating per round, event-timed after warm-up,
  batched   gemmul8.gemm_strided_batched (one split, product and CRT launch per batch)
  loop      gemmul8.gemm per element (what a caller had before the batched entry point)
  bmm       torch.bmm on float64 (vendor path, no interposer)
N = 14, fast mode.  One JSON line per shape and round to profiles/batched/ab.jsonl (or --out); the spread of a
variant over the rounds is the margin a difference has to beat.

  python tools/probes/batched_ab.py [--rounds 5] [--iters 20] [--out FILE]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "mixed-gemmul8_amd"))
import gemmul8 as G  # noqa: E402

SHAPES = [(256, 256, 256, 256), (384, 384, 512, 128), (512, 512, 512, 64), (1024, 1024, 1024, 8), (130, 260, 390, 256)]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batched", "ab.jsonl"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "batched_ab needs a GPU"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as out:
        for m, n, k, batch in SHAPES:
            A = torch.stack([G.randmat(m, k, seed=10 + b) for b in range(batch)])  # [batch] column-major m x k
            B = torch.stack([G.randmat(k, n, seed=9000 + b) for b in range(batch)])
            C = torch.zeros((batch, n, m), dtype=torch.float64, device="cuda")
            wb = torch.empty(G.workSize_strided_batched(m, n, k, N, batch), dtype=torch.uint8, device="cuda")
            w1 = G.alloc_work(m, n, k, N)
            At, Bt = A.transpose(1, 2), B.transpose(1, 2)  # row-major views for torch.bmm: (B^T A^T)^T = A B

            def batched(pt=False):
                return G.gemm_strided_batched(G.OP_N, G.OP_N, m, n, k, 1.0, A, m, m * k, B, k, k * n, 0.0, C, m, m * n,
                                              batch, N, True, wb, phase_times=pt)

            def loop():
                for b in range(batch):
                    G.gemm(G.OP_N, G.OP_N, m, n, k, 1.0, A[b], m, B[b], k, 0.0, C[b], m, N, True, w1)

            def bmm():
                torch.bmm(At, Bt)

            for _ in range(3):
                batched(), loop(), bmm()
            for r in range(a.rounds):
                row = {"m": m, "n": n, "k": k, "batch": batch, "N": N, "round": r,
                       "batched_us": timed(batched, a.iters), "loop_us": timed(loop, max(1, a.iters // 4)),
                       "bmm_f64_us": timed(bmm, a.iters), "phase_ns": batched(True),
                       "products_kernel": G.last_products_kernel()}
                line = json.dumps(row)
                print(line, flush=True)
                out.write(line + "\n")


if __name__ == "__main__":
    main()
