#!/usr/bin/env python3
"""What the evaluation kernels (ctc_amd.collapse_frames, ctc_amd.edit_distance) cost, beside what a user does
without them.

Per shape, on the same frames and transcripts, three ways to the same numbers:

* kernels:  ``collapse_frames`` (with frame confidences), then ``edit_distance`` of its tokens against the transcripts --
            two launches; timed together and each on its own;
* torch:    a torch-only composition, as far as one is expressible -- the collapse as masks, a cumsum and scatters
            (tokens, lengths, start, end; NOT conf: a sum in run order with the kernel's bits is not a torch op), the distance
            as the row recurrence with ``cummin``, one round of ops per hypothesis column, over no more columns than the
            longest hypothesis has (taken from the host here; a user pays a synchronisation for it);
* host:     ``.cpu()`` and the Python / numpy loops of tests/eval_ref.py -- what there was before.

The device bodies are captured (``torch.cuda.graph``) after a warm-up on the capture stream and alternate inside each round; a
round is at least `--calls` replays and at least `--window` seconds of them between two device synchronisations (host clock, no
profiler attached), reported per replay in microseconds as median [min .. max] over the rounds.  The host path is timed
`--host-reps` times with the host clock, the copy included.  All three are compared first, for equality.  There is no gate:
nothing chooses between these paths (profiles/r21_eval.md).

    python tools/eval_bench.py [--rounds 7] [--calls 10] [--window 0.1] [--host-reps 3]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import ctc_amd  # noqa: E402
from tests.eval_ref import collapse_ref, edit_distance_ref  # noqa: E402
from tools.head_wide_bench import captured, fmt, timed  # noqa: E402

# (T, B, S, blank, classes): the flagship no-blank batch, the long blank-CTC batch, the reference's own sizes
SHAPES = [(150, 256, 20, None, 158), (2000, 64, 100, 0, 1000), (10, 10, 5, None, 33)]


def inputs(T, B, S, blank, C, seed=0):
    """frames [B,T] as a trained model's greedy decision looks -- each label of the transcript held for a few frames (blank
    frames between them on the blank lattice), about one frame per eight labels replaced by another class -- with their
    transcripts"""
    rng = np.random.default_rng(seed + T + B)
    lo = 0 if blank is None else 1
    ref = rng.integers(lo, C, (B, S))
    ref_len = rng.integers(max(S // 2, 1), S + 1, B)
    in_len = np.empty(B, np.int64)
    frames = rng.integers(lo, C, (B, T))
    for b in range(B):
        t = 0
        for j in range(ref_len[b]):
            left = ref_len[b] - j
            hold = int(rng.integers(1, max(2, 2 * (T - t) // (left * (3 if blank is not None else 2)))))
            frames[b, t:t + hold] = ref[b, j]
            t += hold
            if blank is not None:
                gap = int(rng.integers(1, 3))
                frames[b, t:t + gap] = blank
                t += gap
            t = min(t, T)
        in_len[b] = max(t, 1)
        noise = rng.random(T) < ref_len[b] / (8 * T)
        frames[b, noise] = rng.integers(lo, C, int(noise.sum()))
    conf = rng.random((B, T), dtype=np.float32)
    return frames, in_len, conf, ref, ref_len


def torch_collapse(frames, in_len, blank):
    """tokens / lengths / start / end of collapse_frames from dense torch ops (no conf)"""
    B, T = frames.shape
    t = torch.arange(T, device=frames.device)
    valid = t[None, :] < in_len[:, None]
    differs = frames[:, 1:] != frames[:, :-1]
    one = torch.ones((B, 1), dtype=torch.bool, device=frames.device)
    keep = valid if blank is None else valid & (frames != blank)
    opens = keep & torch.cat([one, differs], 1)
    closes = keep & (torch.cat([differs, one], 1) | (t[None, :] == in_len[:, None] - 1))
    lengths = opens.sum(1)
    out = []
    for mask, values in ((opens, frames.to(torch.int32)), (opens, t.to(torch.int32).expand(B, T)),
                         (closes, t.to(torch.int32).expand(B, T))):
        slot = torch.where(mask, mask.cumsum(1) - 1, T)                        # (column T: the bin)
        out.append(torch.full((B, T + 1), -1, dtype=torch.int32, device=frames.device).scatter_(1, slot, values)[:, :T])
    return out[0], lengths, out[1], out[2]


def torch_edit_distance(hyp, hyp_len, ref, ref_len):
    """the row recurrence with the in-row dependency as a cummin, one round of dense ops per hypothesis column"""
    B, N = hyp.shape
    M = ref.shape[1]
    j = torch.arange(M + 1, device=hyp.device)
    d = j.expand(B, M + 1)
    res = ref_len.clone()
    for i in range(1, N + 1):
        t = torch.minimum(d[:, 1:] + 1, d[:, :-1] + (ref != hyp[:, i - 1:i]))
        t = torch.cat([torch.full((B, 1), i, device=hyp.device), t], 1)
        d = torch.cummin(t - j, 1).values + j
        res = torch.where(hyp_len == i, d.gather(1, ref_len[:, None]).squeeze(1), res)
    return res.to(torch.int32)


def measure(a, bodies):
    graphs = {k: captured(fn)[0] for k, fn in bodies.items()}
    calls = {k: max(a.calls, int(a.window * 1e6 / timed(g.replay, 3)) + 1) for k, g in graphs.items()}
    times = {k: [] for k in graphs}
    for _ in range(a.rounds):
        for k, g in graphs.items():
            times[k].append(timed(g.replay, calls[k]))
    return times


def sweep(a, dev):
    print("| T | B | S | blank | tokens per sample | what | us per call: median [min .. max] |")
    print("|---|---|---|---|---|---|---|")
    for (T, B, S, blank, C) in SHAPES:
        frames, in_len, conf, ref, ref_len = inputs(T, B, S, blank, C)
        fr, il, fc = torch.from_numpy(frames).to(dev), torch.from_numpy(in_len).to(dev), torch.from_numpy(conf).to(dev)
        rf, rl = torch.from_numpy(ref).to(dev), torch.from_numpy(ref_len).to(dev)

        def host():
            f, i, c, r, n = fr.cpu().numpy(), il.cpu().numpy(), fc.cpu().numpy(), rf.cpu().numpy(), rl.cpu().numpy()
            tokens, lengths, start, end, cf = collapse_ref(f, i, blank, c)
            return tokens, lengths, start, end, cf, edit_distance_ref(tokens, lengths, r, n)

        def kernels():
            c = ctc_amd.collapse_frames(fr, il, blank=blank, frame_conf=fc)
            return c, ctc_amd.edit_distance(c.tokens, c.lengths, rf, rl)

        want = host()
        n_max = max(int(want[1].max()), 1)                     # the longest hypothesis: known here, a synchronisation for a user

        def composed():
            tokens, lengths, start, end = torch_collapse(fr, il, blank)
            return tokens, lengths, start, end, torch_edit_distance(tokens[:, :n_max], lengths, rf, rl)

        c, dist = kernels()
        comp = composed()
        torch.cuda.synchronize()
        for got, w in zip((c.tokens, c.lengths, c.start, c.end, dist), want[:4] + (want[5],)):
            assert torch.equal(got.cpu(), torch.from_numpy(w)), "kernels against the host loops"
        assert torch.equal(c.conf.cpu().view(torch.int32), torch.from_numpy(want[4]).view(torch.int32))
        for got, w in zip(comp, want[:4] + (want[5],)):
            assert torch.equal(got.cpu(), torch.from_numpy(w)), "torch composition against the host loops"
        tok, ln = c.tokens, c.lengths
        times = measure(a, {
            "kernels: collapse_frames + edit_distance": kernels,
            "kernels: collapse_frames": lambda: ctc_amd.collapse_frames(fr, il, blank=blank, frame_conf=fc),
            "kernels: edit_distance": lambda: ctc_amd.edit_distance(tok, ln, rf, rl),
            "torch: collapse + edit distance": composed,
            "torch: collapse (no conf)": lambda: torch_collapse(fr, il, blank),
            "torch: edit distance": lambda: torch_edit_distance(tok[:, :n_max], ln, rf, rl),
        })
        ht = []
        for _ in range(a.host_reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            host()
            ht.append((time.perf_counter() - t0) * 1e6)
        times["host: .cpu() + Python / numpy loops"] = ht
        head = "| %d | %d | %d | %s | %.1f |" % (T, B, S, "none" if blank is None else str(blank), float(want[1].mean()))
        for what, v in times.items():
            print("%s %s | %s |" % (head, what, fmt(v)), flush=True)
        print("(T=%d B=%d: kernels / torch = %.4f, kernels / host = %.6f, on the medians of the whole evaluation)" % (
            T, B, statistics.median(times["kernels: collapse_frames + edit_distance"])
            / statistics.median(times["torch: collapse + edit distance"]),
            statistics.median(times["kernels: collapse_frames + edit_distance"]) / statistics.median(ht)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--window", type=float, default=0.1)
    ap.add_argument("--host-reps", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    print("device: %s" % torch.cuda.get_device_name(dev), flush=True)
    sweep(a, dev)


if __name__ == "__main__":
    main()
