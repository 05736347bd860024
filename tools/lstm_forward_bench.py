#!/usr/bin/env python3
"""Where the one-launch eval forward (ctc_amd_lstm_forward) beats the two launches it replaces, and where it stops.

Times eval-mode ``LSTM_cell.forward`` under ``torch.no_grad()`` two ways in ONE process on the same module and inputs: the
two-launch path (head_forward + lstm_series: the gate closed) and the one-launch path (the gate open).  The two are
timed in alternating rounds; a round is `--calls` forwards between two device synchronisations (host clock), reported
per call in microseconds as median [min .. max] over the rounds.  The outputs are compared bit for bit first.

    python tools/lstm_forward_bench.py [--rounds 9] [--calls 200]

A workgroup does the head of its own four samples for all T frames: the largest 4 T at which the one-launch path is no
slower is what ``producer.FUSED_FORWARD_MAX_WG_ROWS`` holds (profiles/r13_lstm_forward.md)."""
import argparse
import os
import statistics
import sys
import time
import types

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from ctc_amd import producer  # noqa: E402

SHAPES = [(10, 10, 33), (10, 64, 33), (10, 256, 33), (150, 10, 33), (150, 64, 33), (150, 256, 33), (150, 256, 38),
          # between the reference's T = 10 and the benchmark's T = 150: where the crossover lies
          (12, 10, 33), (12, 256, 33), (16, 10, 33), (16, 256, 33), (20, 10, 33), (20, 256, 33), (28, 10, 33), (28, 256, 33),
          (40, 10, 33), (40, 256, 33)]
K = 1024


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--calls", type=int, default=200)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    print("| T | B | C | 4 T | two launches, us | one launch, us | one / two |")
    print("|---|---|---|---|---|---|---|")
    for (T, B, C) in SHAPES:
        torch.manual_seed(T + B + C)
        m = producer.LSTM_cell(types.SimpleNamespace(extract_feat_dim=K, v_class=C, batch_size=B, temporal=T)).to(dev).eval()
        with torch.no_grad():
            m.v.layers[1].running_mean.normal_(0.0, 0.3)
            m.v.layers[1].running_var.uniform_(0.5, 1.5)
        feat = torch.randn(T, B, K, device=dev)
        h0, c0 = 0.1 * torch.randn(B, C, device=dev), 0.1 * torch.randn(B, C, device=dev)

        def run(gate, calls):
            producer.FUSED_FORWARD_MAX_WG_ROWS = gate
            out = None
            with torch.no_grad():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(calls):
                    out = m(feat, h0, c0)
                torch.cuda.synchronize()
            return (time.perf_counter() - t0) / calls * 1e6, out

        shipped = producer.FUSED_FORWARD_MAX_WG_ROWS
        try:
            (_, two), (_, one) = run(0, 20), run(1 << 30, 20)                # warm-up of both paths at this shape
            assert torch.equal(one, two), "the one-launch path differs from the two launches at %s" % ((T, B, C),)
            times = {0: [], 1 << 30: []}
            for _ in range(a.rounds):
                for gate in times:
                    times[gate].append(run(gate, a.calls)[0])
        finally:
            producer.FUSED_FORWARD_MAX_WG_ROWS = shipped
        fmt = lambda v: "%.1f [%.1f .. %.1f]" % (statistics.median(v), min(v), max(v))      # noqa: E731
        two_t, one_t = times[0], times[1 << 30]
        print("| %d | %d | %d | %d | %s | %s | %.2f |" % (T, B, C, 4 * T, fmt(two_t), fmt(one_t),
                                                          statistics.median(one_t) / statistics.median(two_t)), flush=True)


if __name__ == "__main__":
    main()
