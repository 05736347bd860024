"""bf16 / fp16 logits in the no-blank loss against the fp32 launch and the cast route a user has without them.

    python tools/lowp_bench.py [--B 256 2048] [--reps 9] [--per-graph 20] [--eager] [--out FILE]

Routes, per batch size (T = 150, C = 158, S = 20: BASELINE config 2 and its B = 2048 neighbour), each the loss AND the
whole input gradient:
    fp32   ctc_amd_noblank_loss_grad on fp32 logits
    bf16   ctc_amd_noblank_loss_grad_typed on bf16 logits (bf16 gradient)
    fp16   the same on fp16 logits
    cast   what bf16 logits cost without the typed entry: x.float(), the fp32 launch, grad.to(bfloat16)
Each route is captured into a hipGraph of --per-graph back-to-back repetitions (no host launch cost in the number);
after a warm-up the graph is replayed --reps times and the MEDIAN per repetition is reported, with min and max.
--eager issues the same calls without a graph, --per-graph x --reps times per route (for a rocprofv3 --kernel-trace
run, which then times the kernels themselves).
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from ctc_amd import _lib  # noqa: E402
from tests.helpers import synth_noblank  # noqa: E402

T, C, S = 150, 158, 20


def routes(B, dev, lib):
    x, lab, Tb, L = synth_noblank(0, T, B, C, S, var_T=True)
    x32 = x.to(dev)
    xb, xh = x32.to(torch.bfloat16), x32.to(torch.float16)
    lab, Tb, L = lab.to(dev), Tb.to(dev), L.to(dev)
    ws = torch.zeros(lib.ctc_amd_workspace_bytes(_lib.NOBLANK, T, B, C, S), dtype=torch.uint8, device=dev)
    nll = torch.empty(B, device=dev)
    loss = torch.empty((), device=dev)
    g32 = torch.empty_like(x32)
    gb, gh = torch.empty_like(xb), torch.empty_like(xh)
    xf = torch.empty_like(x32)                           # the cast route's fp32 copy of the bf16 logits
    st, sb = x32.stride(0), x32.stride(1)
    sc = 1.0 / B

    def fp32(stream):
        return lib.ctc_amd_noblank_loss_grad(x32.data_ptr(), st, sb, lab.data_ptr(), 0, Tb.data_ptr(), L.data_ptr(),
                                             T, B, C, S, sc, sc, nll.data_ptr(), loss.data_ptr(), g32.data_ptr(),
                                             ws.data_ptr(), stream)

    def typed(xx, gg, code):
        def run(stream):
            return lib.ctc_amd_noblank_loss_grad_typed(xx.data_ptr(), code, st, sb, lab.data_ptr(), 0, Tb.data_ptr(),
                                                       L.data_ptr(), T, B, C, S, -1.0, sc, sc, nll.data_ptr(),
                                                       loss.data_ptr(), gg.data_ptr(), ws.data_ptr(), stream)
        return run

    def cast(stream):
        xf.copy_(xb)                                     # x.float()
        rc = lib.ctc_amd_noblank_loss_grad(xf.data_ptr(), st, sb, lab.data_ptr(), 0, Tb.data_ptr(), L.data_ptr(),
                                           T, B, C, S, sc, sc, nll.data_ptr(), loss.data_ptr(), g32.data_ptr(),
                                           ws.data_ptr(), stream)
        gb.copy_(g32)                                    # grad.to(bfloat16)
        return rc

    return {"fp32": fp32, "bf16": typed(xb, gb, _lib.BF16), "fp16": typed(xh, gh, _lib.F16), "cast": cast}


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
    for _ in range(3):
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
    ap.add_argument("--B", type=int, nargs="+", default=[256, 2048])
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--per-graph", type=int, default=20)
    ap.add_argument("--eager", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = _lib.load()
    lines = ["| B | route | median us | min | max | vs fp32 | vs cast |", "|---|---|---|---|---|---|---|"]
    for B in a.B:
        res = {}
        for name, fn in routes(B, dev, lib).items():
            t = time_route(fn, a.reps, a.per_graph, a.eager)
            if t is not None:
                res[name] = (statistics.median(t), min(t), max(t))
        for name, (med, lo, hi) in res.items():
            lines.append("| %d | %s | %.2f | %.2f | %.2f | %.3f | %.3f |" % (
                B, name, med, lo, hi, med / res["fp32"][0], med / res["cast"][0]))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
