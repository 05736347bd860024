#!/usr/bin/env python3
"""What the beam search launch (ctc_amd.blank_beam_search / ctc_amd.noblank_beam_search) costs, beside what a
user does without it: ``.cpu()`` and Python loops over the [T, C] rows of every sample (tests/beam_ref.py, the float64
restatement of the same rules).

Per shape: the launch is captured (``torch.cuda.graph``) after a warm-up on the capture stream; a round is at least
`--calls` replays and at least `--window` seconds of them between two device synchronisations (host clock, no profiler
attached), reported per replay in microseconds as median [min .. max] over the rounds.  The host path is timed on the first
`--host-samples` samples of the batch, the copy of the whole batch included, and scaled to the batch (it is a loop over
samples).  Those samples are compared first -- tokens and lengths equal, the largest score error printed -- where the
restatement's own scores are no near-ties (tests/test_beam_search_gpu.py states the rule).  There is no gate: nothing
chooses between these paths (profiles/r22_beam_search.md).

    python tools/beam_bench.py [--rounds 7] [--calls 10] [--window 0.2] [--host-samples 2]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import ctc_amd  # noqa: E402
from tests.beam_ref import beam_search_ref  # noqa: E402
from tools.head_wide_bench import captured, fmt, timed  # noqa: E402

# (T, B, C, lattice): the flagship no-blank batch, the long blank-CTC batch; each at W = 16, K = 16
SHAPES = [(150, 256, 158, "noblank"), (2000, 64, 1000, "blank")]
W, K, NBEST = 16, 16, 4
GAP, RTOL = 1e-3, 1e-5


def inputs(T, B, C, lattice, seed=0):
    """logits as a trained model's look: unit noise, each label of a transcript held for 3-9 frames and raised by 10 (blank
    runs between the labels on the blank lattice); the blank lattice gets their log-softmax"""
    rng = np.random.default_rng(seed + T + B)
    x = rng.standard_normal((T, B, C)).astype(np.float32)
    for b in range(B):
        t, prev, k = 0, -1, 0
        while t < T:
            n = int(rng.integers(3, 10))
            c = int(rng.integers(1, C))
            while c == prev:
                c = int(rng.integers(1, C))
            if lattice == "blank" and k % 2:
                c = 0
            else:
                prev = c
            x[t:t + n, b, c] += 10.0
            t, k = t + n, k + 1
    xt = torch.from_numpy(x)
    return torch.log_softmax(xt.double(), -1).float() if lattice == "blank" else xt


def sweep(a, dev):
    print("| T | B | C | lattice | W | K | what | us per call: median [min .. max] |")
    print("|---|---|---|---|---|---|---|---|")
    for (T, B, C, lattice) in SHAPES:
        x = inputs(T, B, C, lattice).to(dev)
        il = torch.full((B,), T, dtype=torch.int64, device=dev)
        blank = 0 if lattice == "blank" else -1

        def launch():
            if lattice == "blank":
                return ctc_amd.blank_beam_search(x, il, beam_width=W, nbest=NBEST, top_classes=K)
            return ctc_amd.noblank_beam_search(x, il, beam_width=W, nbest=NBEST, top_classes=K)

        def host(n):
            xh, ih = x.cpu().numpy(), il.cpu().numpy()
            return beam_search_ref(xh[:, :n], ih[:n], W, K, 5, T, blank, np.float64)

        got = launch()
        torch.cuda.synchronize()
        n = min(a.host_samples, B)
        rt, rl, rs, rc = host(n)
        tokens, lengths, scores = got.tokens.cpu().numpy(), got.lengths.cpu().numpy(), got.scores.cpu().numpy()
        counted, worst = 0, 0.0
        for b in range(n):
            s = rs[b, :min(int(rc[b]), 5)]
            if not np.all(s[:-1] - s[1:] > GAP):
                continue
            counted += 1
            m = min(int(rc[b]), NBEST)
            assert (tokens[b, :m] == rt[b, :m]).all() and (lengths[b, :m] == rl[b, :m]).all(), "launch against the host loops"
            worst = max(worst, max(abs(float(scores[b, k]) - rs[b, k]) / max(1.0, abs(rs[b, k])) for k in range(m)))
        graph, _ = captured(launch)
        calls = max(a.calls, int(a.window * 1e6 / timed(graph.replay, 3)) + 1)
        dev_times = [timed(graph.replay, calls) for _ in range(a.rounds)]
        ht = []
        for _ in range(a.host_reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            host(n)
            ht.append((time.perf_counter() - t0) * 1e6 * B / n)
        head = "| %d | %d | %d | %s | %d | %d |" % (T, B, C, lattice, W, K)
        print("%s launch (graph replay) | %s |" % (head, fmt(dev_times)))
        print("%s host: .cpu() + Python loops (%d samples, scaled to %d) | %s |" % (head, n, B, fmt(ht)), flush=True)
        print("(T=%d B=%d %s: %.2f us per frame of a replay; launch / host = %.6f on the medians; %d of %d compared samples "
              "counted, largest score error %.3g relative to max(1, |score|), bound %.0e)" % (
                  T, B, lattice, statistics.median(dev_times) / T, statistics.median(dev_times) / statistics.median(ht),
                  counted, n, worst, RTOL), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--window", type=float, default=0.2)
    ap.add_argument("--host-samples", type=int, default=2)
    ap.add_argument("--host-reps", type=int, default=2)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    print("device: %s" % torch.cuda.get_device_name(dev), flush=True)
    sweep(a, dev)


if __name__ == "__main__":
    main()
