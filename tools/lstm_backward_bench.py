#!/usr/bin/env python3
"""Where the recurrence's backward on the HIP path, whole (ctc_amd_lstm_backward) beats the path it replaces, and where not.

Runs ``lstm_series`` once per shape and then times ``_SeriesFn.backward`` itself (called on a stand-in for the autograd
context that holds what ``_SeriesFn.forward`` saves) two ways in ONE process on the same tensors: gate closed (the body
runs ``producer._series_backward_torch``: the recurrence launch, three rocBLAS GEMMs, a column sum and a clone -- the
parent's arithmetic) and gate open (the body runs ``producer.lstm_backward``: one call of ``ctc_amd_lstm_backward``).  A
third column is the recurrence launch alone (``producer.lstm_series_backward``), which both bodies start with: what is
left of either column after it is the remainder this tool is about.  Each is captured into a graph (``torch.cuda.graph``)
after a warm-up on the capture stream; the three alternate inside each round; a round is at least `--calls` replays and
at least `--window` seconds of them between two device synchronisations (host clock, no profiler attached), reported per
replay in microseconds as median [min .. max] over the rounds.  The results are compared first.  The ``torch.cat`` of h0
and v_series that the closed gate pays in every training FORWARD is not in its column.

    python tools/lstm_backward_bench.py [--rounds 9] [--calls 200] [--window 0.25] [--e2e]

``--e2e`` adds one end-to-end figure: a train-mode ``LSTM_cell`` forward and backward (eager, host clock) at T = 10, B = 10,
K = 1024, C = 33 with ``SERIES_BACKWARD_MAX_ROWS`` open against closed.

``producer.SERIES_BACKWARD_MAX_ROWS`` holds the largest measured T B up to which the new call's median is below the minimum of
the comparator's rounds at every B and (I, H) measured, with and without d_x (profiles/r15_lstm_backward.md)."""
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

SHAPES = [(T, B, C, C) for (T, B) in ((10, 10), (10, 64), (150, 10), (10, 256), (150, 64), (150, 256)) for C in (33, 38)]


def captured(fn):
    """fn warmed up on a side stream and captured there -> (graph, the captured call's outputs)"""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
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
    producer.SERIES_BACKWARD_MAX_ROWS = 1 << 30                      # (the open context's body looks at it again)
    print("| T | B | I = H | T B | d_x | recurrence launch alone, us | gate closed, us | gate open, us | open / closed "
          "| open median < closed min |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for (T, B, I, H) in SHAPES:
        torch.manual_seed(T + B + H)
        rnd = lambda *s: torch.rand(*s, device=dev) * 2 - 1          # noqa: E731
        v_all, h0, c0 = rnd(T, B, I), rnd(B, H), rnd(B, H)
        w_ih, w_hh, b_ih, b_hh = rnd(4 * H, I) * 0.3, rnd(4 * H, H) * 0.3, rnd(4 * H) * 0.1, rnd(4 * H) * 0.1
        cols = H + 1 if H % 2 else H
        series, gates, cells = producer.lstm_series(v_all, h0, c0, w_ih, w_hh, b_ih, b_hh, cols, want_backward_state=True)
        hs = torch.cat([h0.unsqueeze(0), series[:, :, :H]])          # (what the parent's forward saved)
        up = rnd(T, B, cols)
        for need in (True, False):
            ctx = {                                                  # what _SeriesFn.forward leaves on its context
                "closed": types.SimpleNamespace(H=H, in_place=False, one_launch=True, needs_input_grad=(need,) + (True,) * 6,
                                                saved_tensors=(v_all, w_ih, w_hh, hs, cells, gates)),
                "open": types.SimpleNamespace(H=H, in_place=True, one_launch=True, needs_input_grad=(need,) + (True,) * 6,
                                              saved_tensors=(v_all, w_ih, w_hh, h0, cells, gates, series)),
            }
            paths = {
                "recurrence": lambda: producer.lstm_series_backward(up, gates, cells, w_hh),
                "closed": lambda: producer._SeriesFn.backward(ctx["closed"], up)[:7],
                "open": lambda: producer._SeriesFn.backward(ctx["open"], up)[:7],
            }
            graphs = {k: captured(fn) for k, fn in paths.items()}
            for g, _ in graphs.values():
                g.replay()
            torch.cuda.synchronize()
            for x, y in zip(graphs["closed"][1], graphs["open"][1]):
                if y is not None:
                    assert float((x - y).abs().max()) <= 1e-4 * max(1.0, float(x.abs().max())), (T, B, H)
            times = {k: [] for k in paths}
            calls = {}
            for k, (g, _) in graphs.items():                         # warm-up of the replays; the size of a timed window
                calls[k] = max(a.calls, int(a.window * 1e6 / timed(g.replay, 50)) + 1)
            for _ in range(a.rounds):
                for k, (g, _) in graphs.items():
                    times[k].append(timed(g.replay, calls[k]))
            med = statistics.median(times["open"])
            print("| %d | %d | %d | %d | %s | %s | %s | %s | %.2f | %s |" % (
                T, B, H, T * B, "yes" if need else "no", fmt(times["recurrence"]), fmt(times["closed"]), fmt(times["open"]),
                med / statistics.median(times["closed"]), "yes" if med < min(times["closed"]) else "no"), flush=True)


def end_to_end(a, dev):
    T, B, K, C = 10, 10, 1024, 33
    torch.manual_seed(1)
    model = ctc_amd.LSTM_cell(types.SimpleNamespace(extract_feat_dim=K, v_class=C, batch_size=B, temporal=T)).to(dev).train()
    feat, h0, c0, up = (torch.randn(*s, device=dev) for s in ((T, B, K), (B, C), (B, C), (T, B, C)))
    saved = producer.SERIES_BACKWARD_MAX_ROWS

    def step():
        model.zero_grad(set_to_none=True)
        (model(feat, h0, c0) * up).sum().backward()

    times = {"closed": [], "open": []}
    gate = {"closed": 0, "open": 1 << 30}
    calls = {}
    for k in times:
        producer.SERIES_BACKWARD_MAX_ROWS = gate[k]
        calls[k] = max(a.calls, int(a.window * 1e6 / timed(step, 50)) + 1)
    for _ in range(a.rounds):
        for k in times:
            producer.SERIES_BACKWARD_MAX_ROWS = gate[k]
            times[k].append(timed(step, calls[k]))
    producer.SERIES_BACKWARD_MAX_ROWS = saved
    print("\ntrain-mode LSTM_cell forward + backward, T = %d, B = %d, K = %d, C = %d (eager, us per step):" % (T, B, K, C))
    print("  SERIES_BACKWARD_MAX_ROWS closed: %s" % fmt(times["closed"]))
    print("  SERIES_BACKWARD_MAX_ROWS open:   %s" % fmt(times["open"]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--window", type=float, default=0.25)
    ap.add_argument("--e2e", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    print("device: %s" % torch.cuda.get_device_name(dev), flush=True)
    sweep(a, dev)
    if a.e2e:
        end_to_end(a, dev)


if __name__ == "__main__":
    main()
