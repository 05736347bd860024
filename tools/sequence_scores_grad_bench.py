#!/usr/bin/env python3
"""What the gradient of the sequence scores costs (ctc_amd_sequence_scores_grad behind the autograd of
ctc_amd.blank_sequence_scores / ctc_amd.noblank_sequence_scores), beside the only composition the engine offered
before it: a loop of N loss calls, forward and backward (``blank_ctc_loss`` / ``noblank_ctc_loss`` with candidate column n as
the target), plus the torch arithmetic that recovers  sum_n w[b, n] d score[b, n] / d x  from their N gradients -- the
losses return a batch mean, so each gradient is unscaled per sample (B, and on the blank lattice the target length),
turned from the loss's convention into the score's, weighted and summed.  The losses are not the code under test, so the
loop is a fair yardstick.

Per shape the new call (forward launch + backward: scores, then the weighted gradient) and the loop are captured
(``torch.cuda.graph``) after a warm-up on the capture stream -- the loop twice, so that its run-to-run spread against
itself shows -- and replayed in turn; a round is at least `--calls` replays and at least `--window` seconds of them
between two device synchronisations (host clock, no profiler attached), reported per replay in microseconds as median
[min .. max] over the rounds.  The bar: the new call's MEDIAN below the loop's MINIMUM.  The two gradients are compared
first, on the occupancy scale (max |difference| / max_b sum_n |w[b, n]|).

    python tools/sequence_scores_grad_bench.py [--rounds 7] [--calls 10] [--window 0.2]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import ctc_amd  # noqa: E402
from tools.beam_bench import inputs  # noqa: E402
from tools.head_wide_bench import captured, fmt, timed  # noqa: E402
from tools.sequence_scores_bench import SHAPES, candidates  # noqa: E402

ATOL = 1e-3                                                    # two fp32 routes to the same occupancies: 5e-4 each


def sweep(a, dev):
    print("| use | lattice | T | B | C | N | what | us per call: median [min .. max] |")
    print("|---|---|---|---|---|---|---|---|")
    for (use, lattice, T, B, C, N, kind) in SHAPES:
        blank = lattice == "blank"
        x = inputs(T, B, C, lattice).to(dev).requires_grad_(True)
        il = torch.full((B,), T, dtype=torch.int64, device=dev)
        seqs, lens, counts = candidates(kind, x.detach(), il, lattice, N, dev)
        w = torch.randn(B, N, device=dev)
        torch.cuda.synchronize()
        score = ctc_amd.blank_sequence_scores if blank else ctc_amd.noblank_sequence_scores
        loss = ctc_amd.blank_ctc_loss if blank else ctc_amd.noblank_ctc_loss
        # the loop's targets, one [B,L] tensor per candidate column, made valid outside the timed region; a candidate the
        # launch does not score (beyond the count, empty, without an alignment) is given the weight 0 in BOTH
        full = seqs if seqs.dim() == 3 else seqs.unsqueeze(0).expand(B, -1, -1)
        full_len = lens if lens.dim() == 2 else lens.unsqueeze(0).expand(B, -1)
        with torch.no_grad():
            s0 = score(x, il, seqs, lens, counts=counts)
            w = torch.where(torch.isfinite(s0) & (full_len >= 1), w, torch.zeros_like(w))
        columns = [(full[:, n].clamp(min=1 if blank else 0).contiguous(),
                    full_len[:, n].clamp(min=1, max=full.shape[2]).contiguous()) for n in range(N)]
        unscale = [float(B) * tl.to(torch.float32) if blank else torch.full((B,), float(B), device=dev)
                   for _, tl in columns]
        p = x.detach().exp() if blank else None                 # (the loop's arithmetic needs it; made outside the loop)

        def launch():
            s = score(x, il, seqs, lens, counts=counts)
            (g,) = torch.autograd.grad(s, x, w)
            return g

        def loop():
            total = torch.zeros_like(x)
            for n, (tg, tl) in enumerate(columns):
                (g,) = torch.autograd.grad(loss(x, tg, il, tl)[0], x)
                wn = (w[:, n] * unscale[n])[None, :, None]
                # blank: d loss / d lp = (exp(lp) - occ) / (B L_b), the score's is occ;  no-blank: d score / d x = -B d loss / d x
                total = total + (w[:, n][None, :, None] * p - wn * g if blank else -wn * g)
            return total

        got, want = launch(), loop()
        torch.cuda.synchronize()
        scale = float(w.abs().sum(dim=1).max())
        worst = float((got - want).abs().max()) / max(scale, 1e-30)
        assert worst <= ATOL, "launch against the loop of losses: %g of sum |w|" % worst

        graphs = {"launch": captured(launch)[0], "loop": captured(loop)[0], "loop again": captured(loop)[0]}
        calls = {k: max(a.calls, int(a.window * 1e6 / timed(g.replay, 3)) + 1) for k, g in graphs.items()}
        times = {k: [] for k in graphs}
        for _ in range(a.rounds):
            for k, g in graphs.items():
                times[k].append(timed(g.replay, calls[k]))
        head = "| %s | %s | %d | %d | %d | %d |" % (use, lattice, T, B, C, N)
        print("%s scores + weighted gradient (graph replay) | %s |" % (head, fmt(times["launch"])))
        print("%s loop of %d losses, forward + backward, + arithmetic (graph replay) | %s |" % (head, N, fmt(times["loop"])))
        print("%s the same loop, captured again | %s |" % (head, fmt(times["loop again"])), flush=True)
        loop_min = min(times["loop"] + times["loop again"])
        med = statistics.median(times["launch"])
        live = (w != 0)
        print("(%s %s: median %.1f us against the loop's minimum %.1f us: %s, x%.2f; gradients differ by %.3g of "
              "sum |w|; %d candidates weighted, labels per candidate: mean %.1f, max %d)" % (
                  use, lattice, med, loop_min, "below" if med < loop_min else "NOT below", loop_min / med, worst,
                  int(live.sum()), float(full_len[live].float().mean()), int(full_len[live].max())), flush=True)
        del graphs
        ctc_amd.release_workspaces()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--window", type=float, default=0.2)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    print("device: %s" % torch.cuda.get_device_name(dev), flush=True)
    sweep(a, dev)


if __name__ == "__main__":
    main()
