"""Blank-CTC loss + gradient on wide lattices (S > 255 labels) against torch's own GPU kernel on the same device tensors.

    python tools/blank_wide_bench.py [--shapes 2000x32x64x600 2400x16x32x1023 2000x32x64x255] [--window 0.5]
                                     [--eager N] [--routes ctc_amd torch] [--out FILE]

Routes, per shape T x B x C x S (synth_blank inputs, full-length samples and full-length targets: L_b = S):
    ctc_amd  ctc_amd_blank_loss_grad: nll, loss and the whole input gradient in one call (C ABI, no autograd)
    torch    torch.nn.functional.ctc_loss(reduction="mean") + backward on the same tensors -- what a user of targets
             beyond 255 labels falls back to without the wide path
After a warm-up each route is timed per call with device events around a batch of back-to-back calls, the batch sized
for a window of at least --window seconds; the mean per call over the window is reported (one window: state the number
as that).  --eager N issues N calls of each route and times nothing (for a `rocprofv3 --kernel-trace --stats` run, which
then times the kernels themselves).  Algorithmic bytes of the three launches at padded width NSP: the gather reads
log_probs once and writes the emission table (T B C + T B NSP) x 4; each chain reads the table and writes its lattice,
two chains: 4 T B NSP x 4; the gradient rows read three lattices and log_probs and write the gradient
(3 T B NSP + 2 T B C) x 4.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from ctc_amd import _lib  # noqa: E402
from tests.helpers import synth_blank  # noqa: E402


def routes(T, B, C, S, dev, lib):
    lp, tgt, Tb, _ = synth_blank(0, T, B, C, S)
    L = torch.full((B,), S, dtype=torch.int64)
    lp, tgt, Tb, L = lp.to(dev), tgt.to(dev), Tb.to(dev), L.to(dev)
    ws = torch.zeros(lib.ctc_amd_workspace_bytes(_lib.BLANK, T, B, C, S), dtype=torch.uint8, device=dev)
    nll = torch.empty(B, device=dev)
    loss = torch.empty((), device=dev)
    grad = torch.empty_like(lp)
    st, sb = lp.stride(0), lp.stride(1)
    sc = 1.0 / B
    stream = torch.cuda.current_stream().cuda_stream

    def ours():
        _lib.check(lib.ctc_amd_blank_loss_grad(lp.data_ptr(), st, sb, tgt.data_ptr(), 1, Tb.data_ptr(), L.data_ptr(),
                                               T, B, C, S, 0, sc, sc, nll.data_ptr(), loss.data_ptr(), grad.data_ptr(),
                                               ws.data_ptr(), stream), "ctc_amd_blank_loss_grad")

    x = lp.clone().requires_grad_(True)

    def theirs():
        x.grad = None
        torch.nn.functional.ctc_loss(x, tgt, Tb, L, blank=0, reduction="mean").backward()

    return {"ctc_amd": ours, "torch": theirs}


def time_route(fn, window):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    n = max(5, int(window * 1e3 / max(e0.elapsed_time(e1), 1e-3)) + 1)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n, n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["2000x32x64x600", "2400x16x32x1023", "2000x32x64x255"])
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--eager", type=int, default=0)
    ap.add_argument("--routes", nargs="+", default=["ctc_amd", "torch"])
    ap.add_argument("--out")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = _lib.load()
    lines = ["| T x B x C x S | NSP | route | us per call (mean) | calls | vs torch | GB (algorithmic) | share of 8 TB/s |",
             "|---|---|---|---|---|---|---|---|"]
    for shape in a.shapes:
        T, B, C, S = (int(v) for v in shape.split("x"))
        ns = 2 * S + 1
        nsp = 128 if ns <= 128 else 256 if ns <= 256 else (ns + 511) // 512 * 512
        gb = ((T * B * C + T * B * nsp) + 4 * T * B * nsp + (3 * T * B * nsp + 2 * T * B * C)) * 4 / 1e9
        res = {}
        for name, fn in routes(T, B, C, S, dev, lib).items():
            if name not in a.routes:
                continue
            if a.eager:
                for _ in range(a.eager):
                    fn()
                torch.cuda.synchronize()
            else:
                res[name] = time_route(fn, a.window)
        for name, (us, n) in res.items():
            vs = "%.2f" % (us / res["torch"][0]) if "torch" in res else ""
            traffic = ("%.2f" % gb, "%.1f %%" % (100 * gb * 1e9 / (us * 1e-6) / 8e12)) if name == "ctc_amd" else ("", "")
            lines.append("| %s | %d | %s | %.1f | %d | %s | %s | %s |" % (shape, nsp, name, us, n, vs, *traffic))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
