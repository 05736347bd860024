#!/usr/bin/env python3
"""What reading bf16 logits natively (the *_typed read-out entries of the no-blank and the binary lattice) buys over
the cast it replaces.

Each of the six functions -- ``noblank_`` / ``binary_`` ``best_path``, ``posteriors``, ``token_spans`` -- on bf16 logits, two
ways in ONE process on the same tensors: native path off (``functional._LOWP_READOUT`` emptied: ``logits.float()``, then the
fp32 entry -- the only route there was before the typed entries) and on (the typed entry reads the logits as they lie).  The
outputs are compared first, bitwise.  Every body is captured (``torch.cuda.graph``) after a warm-up on the capture stream;
the two alternate inside each round; a round is at least `--calls` replays and at least `--window` seconds of them between two
device synchronisations (host clock, no profiler attached), reported per replay in microseconds as median [min .. max] over
the rounds.  The queue settings of the process are left as they are.

    python tools/readout_typed_bench.py [--rounds 7] [--calls 10] [--window 0.1]

The rule (r13's, r19's): a function takes the native path by default only where its median is below the minimum of the cast
path's rounds at every measured shape; the tool prints the verdict per function (profiles/r20_readout_typed.md)."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import ctc_amd  # noqa: E402
from ctc_amd import functional  # noqa: E402
from tools.head_wide_bench import fmt, measure  # noqa: E402

# (T, B, C, S): the flagship batch, eight times it, and the reference's own sizes
SHAPES = [(150, 256, 158, 20), (150, 2048, 158, 20), (10, 10, 33, 5)]
NAMES = ["noblank_best_path", "noblank_posteriors", "noblank_token_spans",
         "binary_best_path", "binary_posteriors", "binary_token_spans"]
LOWP = dict(functional._LOWP_READOUT)


def typed(on):
    """the switch: with no 2-byte dtype known to ``_logits_call`` every read-out casts and takes the fp32 entry"""
    functional._LOWP_READOUT = dict(LOWP) if on else {}


def bits_equal(a, b):
    return all(x.dtype is y.dtype and torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32))
               for x, y in zip(a, b))


def inputs(T, B, C, S, lattice, dev):
    g = torch.Generator().manual_seed(T + B + C + S)
    x = (3 * torch.randn(T, B, C, generator=g)).to(torch.bfloat16).to(dev)
    L = torch.randint(1, S + 1, (B,), generator=g)
    Tb = torch.maximum(torch.randint(min(S, T), T + 1, (B,), generator=g), L)
    if lattice == "noblank":
        tg = torch.randint(0, C, (B, S), generator=g, dtype=torch.int32)
    else:
        tg = (torch.rand(B, S, C, generator=g) < 0.05).float()
    return x, tg.to(dev), Tb.long().to(dev), L.long().to(dev)


def sweep(a, dev):
    print("| function | T | B | C | S | cast path, us | native path, us | native / cast | native median < cast min | "
          "logit traffic, MB: cast -> native |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    verdict = {n: True for n in NAMES}
    for name in NAMES:
        fn = getattr(ctc_amd, name)
        for (T, B, C, S) in SHAPES:
            if name == "noblank_posteriors" and C % 2:
                C += 1                                                   # the typed entry's domain: C even
            x, tg, Tb, L = inputs(T, B, C, S, name.split("_")[0], dev)

            def run(on):
                typed(on)
                return fn(x, tg, Tb, L)

            new, old = run(True), run(False)
            torch.cuda.synchronize()
            assert bits_equal(new, old), (name, T, B, C, S)
            times, wins = measure(a, {"old": lambda: run(False), "new": lambda: run(True)})
            n = T * B * C / 1e6                                          # logits, in millions
            # cast path: the cast reads 2 and writes 4 bytes per logit, the launch reads 4; native: the launch reads 2
            print("| %s | %d | %d | %d | %d | %s | %s | %.3f | %s | %.1f -> %.1f |" % (
                name, T, B, C, S, fmt(times["old"]), fmt(times["new"]),
                statistics.median(times["new"]) / statistics.median(times["old"]), "yes" if wins else "no", 10 * n, 2 * n),
                flush=True)
            verdict[name] = verdict[name] and wins
            del x, tg, new, old
            torch.cuda.empty_cache()
    print()
    for name in NAMES:
        print("%s: %s" % (name, "native by default (wins at every measured shape)" if verdict[name]
                          else "keeps the cast by default (the native path does not win at every measured shape)"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--window", type=float, default=0.1)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    print("device: %s" % torch.cuda.get_device_name(dev), flush=True)
    try:
        sweep(a, dev)
    finally:
        typed(True)


if __name__ == "__main__":
    main()
