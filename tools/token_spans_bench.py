"""Token spans in one call against the route a caller composes from the best path and the posteriors, on the same
inputs, in the same process; --family chooses the lattice (blank, the default; noblank; binary).

    python tools/token_spans_bench.py [--family blank] [--shapes 2000x64x1000x100 150x256x158x20 1250x16x64x1023]
                                      [--reps 9] [--per-graph 5] [--eager] [--routes spans composed_b1 composed_b2]
                                      [--out FILE]

Routes of --family noblank / binary, per shape T x B x C x S (synth_noblank / synth_binary inputs, full-length samples;
default shapes 10x10x33x5 and 150x256x158x20):
    spans        (a)  ctc_amd.noblank_token_spans / binary_token_spans: ONE launch
    composed_b1  (b1) *_best_path + *_posteriors: path, score, gamma [B,T,S], nll (two launches)
    composed_b2  (b2) b1, then torch.gather(gamma, 2, path) and the mask of the frames behind T_b: the composition that
                      yields frame_conf.  The float32 per-label loop that a caller would run on the host for start / end /
                      conf is in NEITHER timed region.
Routes of --family blank, per shape T x B x C x S (synth_blank inputs, full-length samples):
    spans        (a)  ctc_amd.blank_token_spans: start, end, conf [B,S], frame_conf, path [B,T], score, nll [B]
    composed_b1  (b1) ctc_amd.blank_best_path + ctc_amd.blank_posteriors: path, score, gamma [B,T,2S+1], nll
    composed_b2  (b2) b1, then torch.gather(gamma, 2, path) and a merge of equal states in torch without a host loop
                      (scatter_reduce amin / amax for the boundaries, scatter_add for the sums, one division)
Each route is captured into a hipGraph of --per-graph back-to-back calls (no host launch cost in the number; the outputs
come from the graph's memory pool); after a warm-up the routes' graphs are replayed in turn, --reps rounds, and the MEDIAN
per call is reported (device events), with min and max.  --eager issues the same calls without a graph, --per-graph x --reps times per route
(for a rocprofv3 --kernel-trace run, which then times the kernels themselves).
Peak bytes: torch.cuda.max_memory_allocated over ONE eager call of the route, above what was allocated before it (the
inputs and the hidden workspace, which all routes share); (a) allocates B (2T + 3S + 2) x 4 bytes of outputs, (b) at least
B T (2S+1) x 4 more for gamma.
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import ctc_amd  # noqa: E402
from tests.helpers import synth_binary, synth_blank, synth_noblank  # noqa: E402


def torch_merge(path, gamma, S):
    """what a caller writes today: per-frame confidence at the path, then one record per label, all on the device"""
    B, T = path.shape
    st = path.long()
    fc = torch.gather(gamma, 2, st.clamp(min=0).unsqueeze(2)).squeeze(2)
    fc = torch.where(st >= 0, fc, torch.zeros_like(fc))
    label = (st > 0) & ((st & 1) == 1)
    col = torch.where(label, (st - 1) >> 1, torch.full_like(st, S))          # other frames go to a spare column
    t = torch.arange(T, device=path.device).expand(B, T)
    first = torch.full((B, S + 1), T, dtype=torch.int64, device=path.device).scatter_reduce_(1, col, t, "amin")
    last = torch.full((B, S + 1), -1, dtype=torch.int64, device=path.device).scatter_reduce_(1, col, t, "amax")
    total = torch.zeros((B, S + 1), device=path.device).scatter_add_(1, col, fc)
    seen = last[:, :S] >= 0
    start = torch.where(seen, first[:, :S], torch.full_like(first[:, :S], -1)).int()
    end = torch.where(seen, last[:, :S] + 1, torch.full_like(last[:, :S], -1)).int()
    conf = torch.where(seen, total[:, :S] / (end - start).clamp(min=1).float(), torch.zeros_like(total[:, :S]))
    return start, end, conf, fc


def lattice_routes(family, T, B, C, S, dev):
    """the no-blank / binary lattice: the new call and what a caller composes today, on the same device tensors"""
    if family == "noblank":
        x, tgt, Tb, L = synth_noblank(0, T, B, C, S)
        spans_fn, path_fn, post_fn = ctc_amd.noblank_token_spans, ctc_amd.noblank_best_path, ctc_amd.noblank_posteriors
    else:
        x, tgt, Tb, L = synth_binary(0, T, B, C, S, density=0.2)
        spans_fn, path_fn, post_fn = ctc_amd.binary_token_spans, ctc_amd.binary_best_path, ctc_amd.binary_posteriors
    args = (x.to(dev), tgt.to(dev), Tb.to(dev), L.to(dev))

    def spans():
        return spans_fn(*args)

    def composed_b1():
        path, score = path_fn(*args)
        gamma, nll = post_fn(*args)
        return path, score, gamma, nll

    def composed_b2():
        path, score, gamma, nll = composed_b1()
        fc = torch.gather(gamma, 2, path.clamp(min=0).long().unsqueeze(2)).squeeze(2)
        fc = torch.where(path >= 0, fc, torch.zeros_like(fc))
        return fc, path, score, nll

    return {"spans": spans, "composed_b1": composed_b1, "composed_b2": composed_b2}


def routes(T, B, C, S, dev, family="blank"):
    if family != "blank":
        return lattice_routes(family, T, B, C, S, dev)
    lp, tgt, Tb, L = synth_blank(0, T, B, C, S)
    args = (lp.to(dev), tgt.to(dev), Tb.to(dev), L.to(dev))

    def spans():
        return ctc_amd.blank_token_spans(*args)

    def composed_b1():
        path, score = ctc_amd.blank_best_path(*args)
        gamma, nll = ctc_amd.blank_posteriors(*args)
        return path, score, gamma, nll

    def composed_b2():
        path, score, gamma, nll = composed_b1()
        return torch_merge(path, gamma, S) + (path, score, nll)

    return {"spans": spans, "composed_b1": composed_b1, "composed_b2": composed_b2}


def peak_bytes(fn):
    fn()                                                 # (the current stream's hidden workspace is allocated here, once)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak


def capture(fn, reps, per_graph, eager):
    """warm-up on a stream of its own, then a hipGraph of per_graph calls (None with --eager: the calls are issued plainly)"""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):                               # warm-up (this stream's workspace; a failing call raises)
            fn()
    torch.cuda.synchronize()
    if eager:
        with torch.cuda.stream(s):
            for _ in range(reps * per_graph):
                fn()
        torch.cuda.synchronize()
        return None
    g = torch.cuda.CUDAGraph()
    keep = []
    with torch.cuda.graph(g, stream=s):
        for _ in range(per_graph):
            keep.append(fn())
    for _ in range(2):
        g.replay()
    torch.cuda.synchronize()
    return g, keep


def time_graphs(graphs, reps, per_graph):
    """the routes' graphs replayed in turn, reps rounds: what disturbs one route in a round disturbs its neighbours too"""
    out = {name: [] for name in graphs}
    for _ in range(reps):
        for name, (g, _keep) in graphs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            g.replay()
            e1.record()
            torch.cuda.synchronize()
            out[name].append(e0.elapsed_time(e1) * 1e3 / per_graph)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--family", choices=["blank", "noblank", "binary"], default="blank")
    ap.add_argument("--shapes", nargs="+")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--per-graph", type=int, default=5)
    ap.add_argument("--eager", action="store_true")
    ap.add_argument("--routes", nargs="+", default=["spans", "composed_b1", "composed_b2"])
    ap.add_argument("--out")
    a = ap.parse_args()
    if not a.shapes:
        a.shapes = (["2000x64x1000x100", "150x256x158x20", "1250x16x64x1023"] if a.family == "blank"
                    else ["10x10x33x5", "150x256x158x20"])
    dev = torch.device("cuda:0")
    lines = ["| T x B x C x S | route | median us | min | max | vs composed_b1 | peak MB of one call |",
             "|---|---|---|---|---|---|---|"]
    for shape in a.shapes:
        T, B, C, S = (int(v) for v in shape.split("x"))
        res, peak, graphs = {}, {}, {}
        fns = {name: fn for name, fn in routes(T, B, C, S, dev, a.family).items() if name in a.routes}
        for name, fn in fns.items():
            g = capture(fn, a.reps, a.per_graph, a.eager)
            if g is not None:
                graphs[name] = g
        for name, t in time_graphs(graphs, a.reps, a.per_graph).items():
            res[name] = (statistics.median(t), min(t), max(t))
        graphs.clear()
        for name in res:
            peak[name] = peak_bytes(fns[name])
        torch.cuda.empty_cache()
        for name, (med, lo, hi) in res.items():
            rel = "%.3f" % (med / res["composed_b1"][0]) if "composed_b1" in res else ""
            lines.append("| %s | %s | %.1f | %.1f | %.1f | %s | %.1f |" % (shape, name, med, lo, hi, rel, peak[name] / 1e6))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
