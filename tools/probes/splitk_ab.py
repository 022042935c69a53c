#!/usr/bin/env python3
"""A/B of the split-K products (few output tiles, long k): in one process, alternating per round, event-timed
after warm-up,
  gemm      gemmul8.gemm, whose products run as gemm_i8_splitk_kernel inside the rule's domain
  nosplit   the same call with the floor on k-steps per split raised beyond any k (GEMMUL8_SPLITK_MIN_STEPS, read
            per call): the one-tile or k-chunked products
  phases    gemmul8.split + products + recombine on the same operands and workspace (they never split k)
  vendor    the hipBLAS GEMM of the shape (gemmul8.time_vendor_gemm)
with the products phase of gemm and of nosplit from the call's own phase times.  The headline shapes run with the
built floor; the edge shapes (k = 2 and 4 floors deep) run once per candidate floor.  One JSON line per shape, floor
and round to profiles/splitk/ab.jsonl (or --out); the min-max of `phases_us` and `nosplit_us` over the rounds is
the spread a difference has to beat.

  python tools/probes/splitk_ab.py [--rounds 5] [--iters 10] [--out FILE]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "mixed-gemmul8_amd"))
import gemmul8 as G  # noqa: E402

ENV, NEVER = "GEMMUL8_SPLITK_MIN_STEPS", str(1 << 30)
# m, n, k, N, fast, floor (None: the built one)
HEADLINE = [(256, 256, 1 << 16, 14, True), (256, 256, 1 << 18, 14, True), (512, 512, 1 << 17, 14, True),
            (512, 512, 1 << 20, 14, True), (768, 768, 1 << 16, 14, True), (512, 512, 1 << 17, 14, False)]
FLOORS = (32, 64, 128, 256)
EDGE = sorted({(mn, mn, d * f * 64, 14, True, f) for mn in (256, 512) for f in FLOORS for d in (2, 4)})


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
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "splitk", "ab.jsonl"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "splitk_ab needs a GPU"
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as out:
        for m, n, k, N, fast, floor in [s + (None,) for s in HEADLINE] + EDGE:
            A, B = G.randmat(m, k, seed=10), G.randmat(k, n, seed=9000)
            C = torch.zeros((n, m), dtype=torch.float64, device="cuda")
            W = G.alloc_work(m, n, k, N)
            iters = max(2, min(a.iters, (a.iters << 16) // k))  # the long shapes take tens of ms per call

            def setenv(v):
                os.environ.pop(ENV, None)
                if v is not None:
                    os.environ[ENV] = str(v)

            def gemm(pt=False):
                return G.gemm(G.OP_N, G.OP_N, m, n, k, 1.0, A, m, B, k, 0.0, C, m, N, fast, W, phase_times=pt)

            def phases():
                G.split(G.OP_N, G.OP_N, m, n, k, A, m, B, k, N, fast, W, torch.float64)
                G.products(m, n, k, N, W)
                G.recombine(m, n, k, N, 1.0, 0.0, C, m, W)

            gemm(), phases()
            vendor = G.time_vendor_gemm(m, n, k, A, B, C, iters) * 1e6
            for r in range(a.rounds):
                row = {"m": m, "n": n, "k": k, "N": N, "fast": fast, "floor": floor, "round": r, "iters": iters}
                setenv(floor)
                row["gemm_us"] = timed(gemm, iters)
                row["gemm_products_us"] = gemm(True)[1] * 1e-3
                row["gemm_kernel"] = G.last_products_kernel()
                setenv(NEVER)
                row["nosplit_us"] = timed(gemm, iters)
                row["nosplit_products_us"] = gemm(True)[1] * 1e-3
                row["nosplit_kernel"] = G.last_products_kernel()
                row["phases_us"] = timed(phases, iters)
                row["phases_products_us"] = timed(lambda: G.products(m, n, k, N, W), iters)
                row["vendor_us"] = vendor if r == 0 else G.time_vendor_gemm(m, n, k, A, B, C, iters) * 1e6
                setenv(None)
                line = json.dumps(row)
                print(line, flush=True)
                out.write(line + "\n")
            del A, B, C, W
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
