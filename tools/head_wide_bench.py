#!/usr/bin/env python3
"""Where the head for batches beyond 256 samples (ctc_amd_head_forward_wide / ctc_amd_head_backward_wide) beats the path it
replaces, and where not.

Forward: ``LSTM_cell._head`` itself, two ways in ONE process on the same tensors -- gate closed (``HEAD_WIDE_MAX_ROWS = 0``, the
parent's arithmetic: ``torch.stack([model.v(feat[t]) for t in range(T)])``, torch's four layers per frame) and gate open (the
mask draw, ``head_forward_wide`` and the closed-form update of the running statistics) -- in train mode (dropout p = 0.3,
gradients enabled: the state of the backward pass is saved on both sides) and in eval mode (no_grad).  Backward: on the state
a train-mode ``head_forward_wide`` saved, ``producer._head_backward_torch`` (what ``_HeadFn.backward`` runs outside its gate)
against ``producer.head_backward_wide``, with and without d_feat.  Every body is captured (``torch.cuda.graph``) after a
warm-up on the capture stream; the two alternate inside each round; a round is at least `--calls` replays and at least
`--window` seconds of them between two device synchronisations (host clock, no profiler attached), reported per replay in
microseconds as median [min .. max] over the rounds.  The results are compared first (eager calls): the forward with dropout
off (the two paths draw different masks otherwise), the backward without d_bias (identically 0 under batch statistics: the
rounding noise of an fp32 sum over up to 307200 rows on both sides), each to 1e-4 max(1, max|comparator|); the last column is
that figure (tests/test_head_wide_gpu.py holds the entries to 1e-4 of float64).

    python tools/head_wide_bench.py [--rounds 7] [--calls 10] [--window 0.15]

``producer.HEAD_WIDE_MAX_ROWS`` / ``producer.HEAD_WIDE_BACKWARD_MAX_ROWS`` hold the largest measured T B at which the new path's
median is below the minimum of the comparator's rounds at every B and C measured -- the forward in both modes, the backward
with and without d_feat (profiles/r18_head_wide.md); the tool prints both at the end."""
import argparse
import os
import statistics
import sys
import time
import types

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import ctc_amd  # noqa: E402
from ctc_amd import producer  # noqa: E402

K = 1024
SHAPES = [(T, B, C) for T in (10, 150) for B in (512, 1024, 2048) for C in (33, 158)]
OPEN = 1 << 30


def captured(fn):
    """fn warmed up on a side stream and captured there -> (graph, the captured call's outputs)"""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        out = fn()
    return graph, out


def timed(run, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        run()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls * 1e6


def fmt(v):
    return "%.1f [%.1f .. %.1f]" % (statistics.median(v), min(v), max(v))


def worst(xs, ys):
    return max(float((x - y).abs().max()) / max(1.0, float(y.abs().max())) for x, y in zip(xs, ys) if y is not None)


def measure(a, bodies):
    """bodies: {"old": fn, "new": fn} -> the two graphs timed alternately -> (times, new median < old minimum)"""
    graphs = {k: captured(fn) for k, fn in bodies.items()}
    calls = {k: max(a.calls, int(a.window * 1e6 / timed(g.replay, 3)) + 1) for k, (g, _) in graphs.items()}
    times = {k: [] for k in graphs}
    for _ in range(a.rounds):
        for k, (g, _) in graphs.items():
            times[k].append(timed(g.replay, calls[k]))
    del graphs
    return times, statistics.median(times["new"]) < min(times["old"])


def row(T, B, C, what, times, wins, dev_max):
    print("| %d | %d | %d | %d | %s | %s | %s | %.3f | %s | %.1e |" % (
        T, B, C, T * B, what, fmt(times["old"]), fmt(times["new"]),
        statistics.median(times["new"]) / statistics.median(times["old"]), "yes" if wins else "no", dev_max), flush=True)


def gate(results):
    """r13's rule: the largest measured T B at which the new path wins every measurement taken at that T B and at every
    smaller measured T B; 0 if there is none"""
    best = 0
    for rows in sorted({r for r, _ in results}):
        if not all(w for r, w in results if r == rows):
            break
        best = rows
    return best


def sweep(a, dev):
    print("| T | B | C | T B | what | comparator, us | wide path, us | wide / comparator | wide median < comparator min | result, wide against comparator |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    fwd, bwd = [], []
    for (T, B, C) in SHAPES:
        torch.manual_seed(T + B + C)
        args = types.SimpleNamespace(extract_feat_dim=K, v_class=C, batch_size=B, temporal=T)
        model = ctc_amd.LSTM_cell(args).to(dev)
        feat = torch.randn(T, B, K, device=dev)

        def head(gate_rows):
            producer.HEAD_WIDE_MAX_ROWS = gate_rows
            return model._head(feat)

        for mode in ("train", "eval"):
            model.train(mode == "train")
            grad = torch.enable_grad if mode == "train" else torch.no_grad
            with grad():
                model.v.layers[3].p = 0.0                                # the comparison: the same mask (none) on both sides
                dev_max = worst([head(OPEN).detach()], [head(0).detach()])
                assert dev_max <= 1e-4, (T, B, C, mode, dev_max)
                model.v.layers[3].p = 0.3
                times, wins = measure(a, {"old": lambda: head(0), "new": lambda: head(OPEN)})
            row(T, B, C, "forward, %s" % mode, times, wins, dev_max)
            fwd.append((T * B, wins))
        # the backward on the state of one train-mode forward
        lin, bn = model.v.layers[0], model.v.layers[1]
        w, gamma, beta = lin.weight.detach(), bn.weight.detach(), bn.bias.detach()
        mask = torch.nn.functional.dropout(torch.ones(T, B, C, device=dev), 0.3, True)
        _, lo, mean, _, inv = producer.head_forward_wide(feat, w, lin.bias.detach(), gamma, beta, mask=mask, want_backward_state=True)
        d_out = torch.randn(T, B, C, device=dev)
        for need in (True, False):
            bodies = {
                "old": lambda: producer._head_backward_torch(d_out, feat, w, gamma, beta, lo, mean, inv, mask, True, need),
                "new": lambda: producer.head_backward_wide(d_out, feat, w, gamma, beta, lo, mean, inv, None, None, 1e-5, mask, need),
            }
            new, old = bodies["new"](), bodies["old"]()
            dev_max = worst(new[:2] + new[3:], old[:2] + old[3:])             # (d_feat, d_weight, d_bn_weight, d_bn_bias)
            assert dev_max <= 1e-4, (T, B, C, need, dev_max)
            times, wins = measure(a, bodies)
            row(T, B, C, "backward, %s d_feat" % ("with" if need else "no"), times, wins, dev_max)
            bwd.append((T * B, wins))
        del model, feat, lo, mask, d_out
        torch.cuda.empty_cache()
    print()
    print("HEAD_WIDE_MAX_ROWS = %d, HEAD_WIDE_BACKWARD_MAX_ROWS = %d by the rule" % (gate(fwd), gate(bwd)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--window", type=float, default=0.15)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    print("device: %s" % torch.cuda.get_device_name(dev), flush=True)
    saved = producer.HEAD_WIDE_MAX_ROWS
    try:
        sweep(a, dev)
    finally:
        producer.HEAD_WIDE_MAX_ROWS = saved


if __name__ == "__main__":
    main()
