#!/usr/bin/env python3
"""What the sequence-scores launch (ctc_amd.blank_sequence_scores / ctc_amd.noblank_sequence_scores) costs,
beside the only composition the engine offered before it: a loop of N forward-only loss calls (``blank_ctc_loss`` /
``noblank_ctc_loss`` under ``no_grad``), one per candidate column, on the same inputs.  The losses are not the code under
test, so the loop is a fair yardstick.

Per shape the launch and the loop are captured (``torch.cuda.graph``) after a warm-up on the capture stream -- the loop
twice, so that its run-to-run spread against itself shows -- and replayed in turn; a round is at least `--calls` replays and
at least `--window` seconds of them between two device synchronisations (host clock, no profiler attached), reported per
replay in microseconds as median [min .. max] over the rounds.  The bar: the launch's MEDIAN below the loop's MINIMUM.
The scores are compared first: the launch against ``-nll`` of the loop wherever that is finite.

    python tools/sequence_scores_bench.py [--rounds 7] [--calls 10] [--window 0.2]"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import ctc_amd  # noqa: E402
from tools.beam_bench import inputs  # noqa: E402
from tools.head_wide_bench import captured, fmt, timed  # noqa: E402

RTOL = 1e-5
MAX_TOKENS = 255                                               # the launch's limit on labels per candidate

# (use, lattice, T, B, C, N, candidates)
SHAPES = [("rescoring", "blank", 2000, 64, 1000, 4, "beam"),
          ("rescoring", "noblank", 150, 256, 158, 4, "beam"),
          ("retrieval", "noblank", 150, 256, 158, 64, "shared"),
          ("reference's size", "blank", 10, 10, 33, 4, "random"),
          ("reference's size", "noblank", 10, 10, 33, 4, "random")]


def random_transcripts(rng, N, L, C, lattice):
    """[N,L] int64 padded with -1 and [N] lengths: 1 .. L labels without equal neighbours, never the blank (class 0)"""
    seqs, lens = np.full((N, L), -1, np.int64), rng.integers(1, L + 1, N)
    for n in range(N):
        prev = -1
        for i in range(int(lens[n])):
            c = int(rng.integers(1 if lattice == "blank" else 0, C))
            while c == prev:
                c = int(rng.integers(1 if lattice == "blank" else 0, C))
            seqs[n, i] = prev = c
    return seqs, lens.astype(np.int64)


def candidates(kind, x, il, lattice, N, dev):
    """-> (sequences, lengths, counts) as the launch takes them"""
    T, B, C = x.shape
    if kind == "beam":                                          # an n-best list, as the beam search leaves it
        search = ctc_amd.blank_beam_search if lattice == "blank" else ctc_amd.noblank_beam_search
        hyp = search(x, il, beam_width=16, nbest=N, top_classes=16, max_tokens=min(T, MAX_TOKENS))
        return hyp.tokens, hyp.lengths, hyp.count
    rng = np.random.default_rng(T + N)
    if kind == "shared":                                        # known transcripts, one set for the batch
        seqs, lens = random_transcripts(rng, N, 20, C, lattice)
    else:
        seqs, lens = random_transcripts(rng, B * N, 4, C, lattice)
        seqs, lens = seqs.reshape(B, N, -1), lens.reshape(B, N)
    return torch.from_numpy(seqs).to(dev), torch.from_numpy(lens).to(dev), None


def sweep(a, dev):
    print("| use | lattice | T | B | C | N | what | us per call: median [min .. max] |")
    print("|---|---|---|---|---|---|---|---|")
    for (use, lattice, T, B, C, N, kind) in SHAPES:
        x = inputs(T, B, C, lattice).to(dev)
        il = torch.full((B,), T, dtype=torch.int64, device=dev)
        seqs, lens, counts = candidates(kind, x, il, lattice, N, dev)
        torch.cuda.synchronize()
        score = ctc_amd.blank_sequence_scores if lattice == "blank" else ctc_amd.noblank_sequence_scores
        loss = ctc_amd.blank_ctc_loss if lattice == "blank" else ctc_amd.noblank_ctc_loss
        # the loop's targets, one [B,L] tensor per candidate column, made valid outside the timed region
        full = seqs if seqs.dim() == 3 else seqs.unsqueeze(0).expand(B, -1, -1)
        full_len = lens if lens.dim() == 2 else lens.unsqueeze(0).expand(B, -1)
        columns = [(full[:, n].clamp(min=1 if lattice == "blank" else 0).contiguous(),
                    full_len[:, n].clamp(min=1, max=full.shape[2]).contiguous()) for n in range(N)]

        def launch():
            return score(x, il, seqs, lens, counts=counts)

        def loop():
            with torch.no_grad():
                return [loss(x, tg, il, tl)[1] for tg, tl in columns]

        got = launch().double().cpu().numpy()
        nll = np.stack([v.double().cpu().numpy() for v in loop()], axis=1)
        lens_h = full_len.cpu().numpy()
        exist = lens_h if counts is None else lens_h[np.arange(N)[None, :] < counts.cpu().numpy()[:, None]]
        comparable = np.isfinite(nll) & (nll < 1e12) & (lens_h >= 1) & (lens_h <= full.shape[2]) & np.isfinite(got)
        worst = float((np.abs(got + nll)[comparable] / np.maximum(1.0, np.abs(nll[comparable]))).max())
        assert comparable.sum() >= B and worst <= 2 * RTOL, "launch against the loop of losses: %g" % worst

        graphs = {"launch": captured(launch)[0], "loop": captured(loop)[0], "loop again": captured(loop)[0]}
        calls = {k: max(a.calls, int(a.window * 1e6 / timed(g.replay, 3)) + 1) for k, g in graphs.items()}
        times = {k: [] for k in graphs}
        for _ in range(a.rounds):
            for k, g in graphs.items():
                times[k].append(timed(g.replay, calls[k]))
        head = "| %s | %s | %d | %d | %d | %d |" % (use, lattice, T, B, C, N)
        print("%s one launch (graph replay) | %s |" % (head, fmt(times["launch"])))
        print("%s loop of %d forward-only losses (graph replay) | %s |" % (head, N, fmt(times["loop"])))
        print("%s the same loop, captured again | %s |" % (head, fmt(times["loop again"])), flush=True)
        loop_min = min(times["loop"] + times["loop again"])
        med = statistics.median(times["launch"])
        print("(%s %s: launch median %.1f us against the loop's minimum %.1f us: %s, x%.2f; %d scores compared with the "
              "loop, largest difference %.3g relative to max(1, |score|); labels per candidate: mean %.1f, max %d)" % (
                  use, lattice, med, loop_min, "below" if med < loop_min else "NOT below", loop_min / med,
                  int(comparable.sum()), worst, float(exist.mean()), int(exist.max())), flush=True)
        del graphs


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
