"""Blank-CTC best path (forced alignment) and state posteriors against the blank loss + gradient on the same inputs, in
the same process.

    python tools/align_bench.py [--shapes 2000x64x1000x100 150x256x158x20] [--reps 9] [--per-graph 10] [--eager]
                                [--routes best_path posteriors loss_grad] [--out FILE]

Routes, per shape T x B x C x S (synth_blank inputs, full-length samples):
    best_path   ctc_amd_blank_best_path (S <= 255) or ctc_amd_blank_best_path_wide (256 <= S <= 1023): path [B,T] int32
                + score [B]
    posteriors  ctc_amd_blank_posteriors (S <= 255) or ctc_amd_blank_posteriors_wide (256 <= S <= 1023): gamma
                [B,T,2S+1] fp32 + nll [B]
    loss_grad   ctc_amd_blank_loss_grad: nll, loss and the whole input gradient (the library's own schedule)
Each route is captured into a hipGraph of --per-graph back-to-back calls (no host launch cost in the number); after a
warm-up the graph is replayed --reps times and the MEDIAN per call is reported (device events), with min and max.
--eager issues the same calls without a graph, --per-graph x --reps times per route (for a rocprofv3 --kernel-trace
run, which then times the kernels themselves).  Algorithmic bytes of the best path: every log_probs row read once
plus the path written (T B C + T B) x 4; of the posteriors: every log_probs row read once plus gamma written
(T B C + T B (2S+1)) x 4.
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from ctc_amd import _lib  # noqa: E402
from tests.helpers import synth_blank  # noqa: E402


def routes(T, B, C, S, dev, lib):
    lp, tgt, Tb, L = synth_blank(0, T, B, C, S)
    lp, tgt, Tb, L = lp.to(dev), tgt.to(dev), Tb.to(dev), L.to(dev)
    need = lib.ctc_amd_workspace_bytes(_lib.BLANK, T, B, C, S)
    ws_a = torch.zeros(need, dtype=torch.uint8, device=dev)
    narrow = S <= 255                                    # the narrow entries stop there
    ws_p = torch.zeros(need, dtype=torch.uint8, device=dev)
    gamma = torch.empty((B, T, 2 * S + 1), device=dev)
    pnll = torch.empty(B, device=dev)
    ws_l = torch.zeros(need, dtype=torch.uint8, device=dev)
    path = torch.empty((B, T), dtype=torch.int32, device=dev)
    score = torch.empty(B, device=dev)
    nll = torch.empty(B, device=dev)
    loss = torch.empty((), device=dev)
    grad = torch.empty_like(lp)
    st, sb = lp.stride(0), lp.stride(1)
    sc = 1.0 / B

    entry = lib.ctc_amd_blank_best_path if narrow else lib.ctc_amd_blank_best_path_wide

    def best_path(stream):
        return entry(lp.data_ptr(), st, sb, tgt.data_ptr(), 1, Tb.data_ptr(), L.data_ptr(),
                     T, B, C, S, 0, path.data_ptr(), score.data_ptr(), ws_a.data_ptr(), stream)

    pentry = lib.ctc_amd_blank_posteriors if narrow else lib.ctc_amd_blank_posteriors_wide

    def posteriors(stream):
        return pentry(lp.data_ptr(), st, sb, tgt.data_ptr(), 1, Tb.data_ptr(), L.data_ptr(),
                      T, B, C, S, 0, pnll.data_ptr(), gamma.data_ptr(), ws_p.data_ptr(), stream)

    def loss_grad(stream):
        return lib.ctc_amd_blank_loss_grad(lp.data_ptr(), st, sb, tgt.data_ptr(), 1, Tb.data_ptr(), L.data_ptr(),
                                           T, B, C, S, 0, sc, sc, nll.data_ptr(), loss.data_ptr(), grad.data_ptr(),
                                           ws_l.data_ptr(), stream)

    return {"best_path": best_path, "posteriors": posteriors, "loss_grad": loss_grad}


def time_route(fn, reps, per_graph, eager):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):                               # warm-up (and the argument check: a failing call raises)
            _lib.check(fn(s.cuda_stream), "launch")
    torch.cuda.synchronize()
    if eager:
        with torch.cuda.stream(s):
            for _ in range(reps * per_graph):
                fn(s.cuda_stream)
        torch.cuda.synchronize()
        return None
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        for _ in range(per_graph):
            fn(s.cuda_stream)
    for _ in range(2):
        g.replay()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / per_graph)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["2000x64x1000x100", "150x256x158x20"])
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--per-graph", type=int, default=10)
    ap.add_argument("--eager", action="store_true")
    ap.add_argument("--routes", nargs="+", default=["best_path", "posteriors", "loss_grad"])
    ap.add_argument("--out")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = _lib.load()
    lines = ["| T x B x C x S | route | median us | min | max | vs loss_grad | GB/s (algorithmic) |",
             "|---|---|---|---|---|---|---|"]
    for shape in a.shapes:
        T, B, C, S = (int(v) for v in shape.split("x"))
        res = {}
        for name, fn in routes(T, B, C, S, dev, lib).items():
            if name not in a.routes and name != "loss_grad":
                continue
            t = time_route(fn, a.reps, a.per_graph, a.eager)
            if t is not None:
                res[name] = (statistics.median(t), min(t), max(t))
        nbytes = {"best_path": (T * B * C + T * B) * 4, "posteriors": (T * B * C + T * B * (2 * S + 1)) * 4}
        for name, (med, lo, hi) in res.items():
            rate = "%.0f" % (nbytes[name] / med / 1e3) if name in nbytes else ""
            lines.append("| %s | %s | %.1f | %.1f | %.1f | %.3f | %s |" % (
                shape, name, med, lo, hi, med / res["loss_grad"][0], rate))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
