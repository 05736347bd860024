#!/usr/bin/env python3
"""Where the wide recurrence (ctc_amd_lstm_series_wide / ctc_amd_lstm_series_backward_wide, up to 160 classes) beats the path
it replaces, and where not.

Times ``_SeriesFn.forward`` and ``_SeriesFn.backward`` themselves (called on a stand-in for the autograd context, everything
needing a gradient) two ways in ONE process on the same tensors: gate closed (``SERIES_WIDE_MAX_ROWS = 0``, the parent's
arithmetic: T launches of ``ctc_amd_lstm_cell_step``, then the BPTT loop of torch kernels) and gate open (the wide forward
entry, then the wide backward recurrence with ``_series_backward_torch``'s three GEMMs and the HIP column sum behind it).
Forward, backward, and forward + backward in one graph are each captured (``torch.cuda.graph``) after a warm-up on the
capture stream; closed and open alternate inside each round; a round is at least `--calls` replays and at least `--window`
seconds of them between two device synchronisations (host clock, no profiler attached), reported per replay in microseconds
as median [min .. max] over the rounds.  The results are compared first: v_series bit for bit, the gradients to 1e-4 max(1, max|closed|)
(eager calls; the parameters are drawn like nn.LSTMCell's initialisation); the last column is what one replay of the graphs
gives against the eager calls, held to the same 1e-4.

    python tools/lstm_wide_bench.py [--rounds 7] [--calls 20] [--window 0.25]

``producer.SERIES_WIDE_MAX_ROWS`` holds the largest measured T B up to which the open path's forward + backward median is
below the minimum of the closed path's rounds at every B and H measured (profiles/r16_lstm_wide.md)."""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import ctc_amd  # noqa: E402,F401
from ctc_amd import producer  # noqa: E402

SHAPES = [(T, B, C, C) for (T, B) in ((10, 10), (10, 64), (150, 10), (10, 256), (150, 64), (150, 256)) for C in (158, 96)]
GATE = {"closed": 0, "open": 1 << 30}


class Ctx:
    """what _SeriesFn.forward and .backward need of an autograd context"""
    needs_input_grad = (True,) * 7 + (False, False)

    def save_for_backward(self, *tensors):
        self.saved_tensors = tensors


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


def sweep(a, dev):
    print("| T | B | I = H | T B | what | gate closed, us | gate open, us | open / closed | open median < closed min | gradients, open against closed | replay against eager, closed / open |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    for (T, B, I, H) in SHAPES:
        torch.manual_seed(T + B + H)
        rnd = lambda *s: torch.rand(*s, device=dev) * 2 - 1          # noqa: E731
        v_all, h0, c0 = rnd(T, B, I), rnd(B, H), rnd(B, H)
        k0 = H ** -0.5                                               # nn.LSTMCell's own initialisation: uniform(-1 / sqrt(H), 1 / sqrt(H))
        w_ih, w_hh, b_ih, b_hh = rnd(4 * H, I) * k0, rnd(4 * H, H) * k0, rnd(4 * H) * k0, rnd(4 * H) * k0
        cols = H + 1 if H % 2 else H
        up = rnd(T, B, cols)
        graphs, eager, held = {}, {}, {}
        for k, gate in GATE.items():
            producer.SERIES_WIDE_MAX_ROWS = gate                     # (read in forward only: the context carries the choice)

            def forward(ctx):
                return producer._SeriesFn.forward(ctx, v_all, h0, c0, w_ih, w_hh, b_ih, b_hh, cols, producer.PAD_LOGIT)

            def both():
                ctx = Ctx()
                series = forward(ctx)
                return (series,) + tuple(producer._SeriesFn.backward(ctx, up)[:7])

            ctx = held[k] = Ctx()                                    # (kept: a graph holds no reference to what it reads)
            forward(ctx)                                             # the saved state the backward-only graph reads
            assert bool(getattr(ctx, "wide", False)) == (k == "open") and not ctx.one_launch, (k, T, B, H)
            eager[k] = [t.clone() for t in both()]
            graphs[k] = {"forward": captured(lambda: forward(Ctx())),
                         "backward": captured(lambda ctx=ctx: producer._SeriesFn.backward(ctx, up)[:7]),
                         "forward + backward": captured(both)}
        torch.cuda.synchronize()
        worst = lambda xs, ys: max(float((x - y).abs().max()) / max(1.0, float(y.abs().max())) for x, y in zip(xs, ys))   # noqa: E731
        assert torch.equal(eager["closed"][0], eager["open"][0]), (T, B, H)
        dev_max = worst(eager["open"][1:], eager["closed"][1:])
        assert dev_max <= 1e-4, (T, B, H, [worst([x], [y]) for x, y in zip(eager["open"][1:], eager["closed"][1:])])
        rep = {}
        for k in graphs:                                             # what a replay gives against what the eager call gave
            for g, _ in graphs[k].values():
                g.replay()
            torch.cuda.synchronize()
            rep[k] = max(worst([graphs[k]["forward"][1]], eager[k][:1]), worst(graphs[k]["backward"][1], eager[k][1:]),
                         worst(graphs[k]["forward + backward"][1], eager[k]))
            if rep[k] > 1e-4:                                        # reported per output, then the tool fails
                print("replay against eager, %s, per output (v_series, d_x, dh0, dc0, d_w_ih, d_w_hh, d_b_ih, d_b_hh): %s" % (
                    k, " ".join("%.1e" % worst([x], [y]) for x, y in zip(graphs[k]["forward + backward"][1], eager[k]))))
        assert max(rep.values()) <= 1e-4, (T, B, H, rep)
        for what in ("forward", "backward", "forward + backward"):
            times = {k: [] for k in graphs}
            calls = {}
            for k in graphs:                                         # warm-up of the replays; the size of a timed window
                calls[k] = max(a.calls, int(a.window * 1e6 / timed(graphs[k][what][0].replay, 5)) + 1)
            for _ in range(a.rounds):
                for k in graphs:
                    times[k].append(timed(graphs[k][what][0].replay, calls[k]))
            med = statistics.median(times["open"])
            print("| %d | %d | %d | %d | %s | %s | %s | %.3f | %s | %.1e | %.1e / %.1e |" % (
                T, B, H, T * B, what, fmt(times["closed"]), fmt(times["open"]), med / statistics.median(times["closed"]),
                "yes" if med < min(times["closed"]) else "no", dev_max, rep["closed"], rep["open"]), flush=True)
        del graphs, eager, held


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--window", type=float, default=0.25)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    print("device: %s" % torch.cuda.get_device_name(dev), flush=True)
    saved = producer.SERIES_WIDE_MAX_ROWS
    try:
        sweep(a, dev)
    finally:
        producer.SERIES_WIDE_MAX_ROWS = saved


if __name__ == "__main__":
    main()
