#!/usr/bin/env python3
"""Where the head's backward on the HIP path (ctc_amd_head_backward) beats the torch arithmetic it replaces, and where not.

Runs a train-mode ``head_forward`` once per shape and then times the backward two ways in ONE process on the same saved
tensors: the torch arithmetic (``producer._head_backward_torch``: elementwise kernels and two rocBLAS GEMMs, what
``_HeadFn.backward`` runs outside the gate) and the new call (``producer.head_backward``).  The two alternate inside each
round; a round is `--calls` backward passes between two device synchronisations (host clock, no profiler attached), reported
per call in microseconds as median [min .. max] over the rounds.  The results are compared first.

    python tools/head_backward_bench.py [--rounds 9] [--calls 100]

``producer.HEAD_BACKWARD_MAX_ROWS`` holds the largest measured T B up to which the new call's median is below the minimum
of the torch arithmetic's rounds at every B and C measured, with and without d_feat (profiles/r14_head_backward.md)."""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from ctc_amd import producer  # noqa: E402

K = 1024
SHAPES = [(T, B, C) for T in (10, 40, 150) for B in (10, 64, 256) for C in (33, 158)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--calls", type=int, default=100)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    print("| T | B | C | T B | d_feat | torch arithmetic, us | head_backward, us | new / torch | new median < torch min |")
    print("|---|---|---|---|---|---|---|---|---|")
    for (T, B, C) in SHAPES:
        torch.manual_seed(T + B + C)
        feat = torch.randn(T, B, K, device=dev)
        w, b = torch.randn(C, K, device=dev) * 0.03, torch.randn(C, device=dev) * 0.1
        gamma, beta = torch.rand(C, device=dev) + 0.5, torch.randn(C, device=dev) * 0.2
        mask = torch.nn.functional.dropout(torch.ones(T, B, C, device=dev), 0.3, True)
        _, lin, mean, _, inv = producer.head_forward(feat, w, b, gamma, beta, mask=mask, want_backward_state=True)
        d_out = torch.randn(T, B, C, device=dev)
        for need in (True, False):
            paths = {
                "torch": lambda: producer._head_backward_torch(d_out, feat, w, gamma, beta, lin, mean, inv, mask, True, need),
                "hip": lambda: producer.head_backward(d_out, feat, w, gamma, beta, lin, mean, inv, None, None, 1e-5, mask, need),
            }

            def run(fn, calls):
                out = None
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(calls):
                    out = fn()
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) / calls * 1e6, out

            ref, got = run(paths["torch"], 10)[1], run(paths["hip"], 10)[1]          # warm-up of both paths at this shape
            for x, y in zip(ref, got):
                if x is not None:
                    assert float((x - y).abs().max()) <= 1e-3 * max(1.0, float(x.abs().max())), (T, B, C)
            times = {k: [] for k in paths}
            for _ in range(a.rounds):
                for k, fn in paths.items():
                    times[k].append(run(fn, a.calls)[0])
            fmt = lambda v: "%.1f [%.1f .. %.1f]" % (statistics.median(v), min(v), max(v))      # noqa: E731
            med = statistics.median(times["hip"])
            print("| %d | %d | %d | %d | %s | %s | %s | %.2f | %s |" % (
                T, B, C, T * B, "yes" if need else "no", fmt(times["torch"]), fmt(times["hip"]),
                med / statistics.median(times["torch"]), "yes" if med < min(times["torch"]) else "no"), flush=True)


if __name__ == "__main__":
    main()
