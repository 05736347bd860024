#!/usr/bin/env python3
"""What the bigram table costs the beam search launch, and whether the plain launch is still the one it was.

Per shape of tools/beam_bench.py (the two the README quotes), W = 16, K = 16, nbest = 4:

    (a) the plain entry of the PARENT commit   ``--parent-lib``: a shared library built from the parent's
                                               ctc_amd/csrc/beam_search.hip alone (``git show <parent>:ctc_amd/csrc/
                                               beam_search.hip``, hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared
                                               -I ctc_amd/csrc), called through ctypes on the same tensors; captured TWICE
                                               (a1, a2): the difference of the two is the spread of one kernel against itself
    (b) the plain entry of this tree           ``ctc_amd.blank_beam_search`` / ``noblank_beam_search`` without ``lm``
    (c) the fused entry                        the same call with ``lm`` (log-softmax rows of 1.5 x unit noise, a tenth of
                                               the entries -inf), lm_weight 0.8, token_bonus 0.5

The method of tools/beam_bench.py: every launch is captured (``torch.cuda.graph``) after a warm-up on the capture stream; the
graphs ALTERNATE inside each round; a round is at least `--calls` replays and at least `--window` seconds of them between two
device synchronisations (host clock, no profiler attached); microseconds per replay, median [min .. max] over the rounds.
Before a shape is timed, (a) and (b) are compared bit for bit, and the first `--host-samples` samples of (c) with the float64
restatement (tests/beam_lm_ref.py) under the rule of tests/test_beam_lm_gpu.py.  Results: profiles/r23_beam_lm.md.

    python tools/beam_lm_bench.py [--parent-lib PATH] [--rounds 7] [--calls 10] [--window 0.2] [--host-samples 1]"""
import argparse
import ctypes
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import ctc_amd  # noqa: E402
from ctc_amd import _lib  # noqa: E402
from tests.beam_lm_ref import beam_lm_search_ref  # noqa: E402
from tools.beam_bench import GAP, K, NBEST, RTOL, SHAPES, W, inputs  # noqa: E402
from tools.head_wide_bench import captured, fmt, timed  # noqa: E402

ALPHA, BETA = 0.8, 0.5


def table(C, seed=0):
    rng = np.random.default_rng(seed + 1000)
    lm = torch.log_softmax(torch.from_numpy(rng.standard_normal((C + 1, C)) * 1.5), -1).float()
    lm[torch.from_numpy(rng.random((C + 1, C)) < 0.1)] = float("-inf")
    return lm


def parent_launcher(path, x, il, blank):
    """the parent's ctc_amd_beam_search on preallocated outputs -> (launch, outputs)"""
    lib = ctypes.CDLL(path)
    for name in ("ctc_amd_beam_search_scratch_bytes", "ctc_amd_beam_search"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.PROTOTYPES[name]
    T, B, C = x.shape
    dev = x.device
    tokens = torch.empty((B, NBEST, T), dtype=torch.int32, device=dev)
    lengths = torch.empty((B, NBEST), dtype=torch.int64, device=dev)
    scores = torch.empty((B, NBEST), dtype=torch.float32, device=dev)
    count = torch.empty(B, dtype=torch.int32, device=dev)
    need = lib.ctc_amd_beam_search_scratch_bytes(T, B, W)
    scratch = torch.empty(need, dtype=torch.uint8, device=dev)

    def launch():
        rc = lib.ctc_amd_beam_search(x.data_ptr(), x.stride(0), x.stride(1), il.data_ptr(), T, B, C, blank, W, K, NBEST, T,
                                     tokens.data_ptr(), lengths.data_ptr(), scores.data_ptr(), count.data_ptr(),
                                     scratch.data_ptr(), need, torch.cuda.current_stream(dev).cuda_stream)
        assert rc == 0, rc
        return tokens, lengths, scores, count

    return launch


def sweep(a, dev):
    print("| T | B | C | lattice | what | us per call: median [min .. max] |")
    print("|---|---|---|---|---|---|")
    for (T, B, C, lattice) in SHAPES:
        x = inputs(T, B, C, lattice).to(dev)
        il = torch.full((B,), T, dtype=torch.int64, device=dev)
        lm = table(C).to(dev)
        blank = 0 if lattice == "blank" else -1
        fn = ctc_amd.blank_beam_search if lattice == "blank" else ctc_amd.noblank_beam_search
        kw = dict(beam_width=W, nbest=NBEST, top_classes=K)
        bodies = {"(b) plain, this tree": lambda: fn(x, il, **kw),
                  "(c) fused, this tree": lambda: fn(x, il, lm=lm, lm_weight=ALPHA, token_bonus=BETA, **kw)}
        plain = bodies["(b) plain, this tree"]()
        fused = bodies["(c) fused, this tree"]()
        torch.cuda.synchronize()
        if a.parent_lib:
            parent = parent_launcher(a.parent_lib, x, il, blank)
            bodies = {"(a1) plain, parent": parent, **bodies, "(a2) plain, parent again": parent}
            old = parent()
            torch.cuda.synchronize()
            assert all(torch.equal(u, v) for u, v in zip(old, plain)), "the plain entry's bits changed"
        # (c) against the restatement
        n = min(a.host_samples, B)
        rt, rl, rs, rc, ra, rabs = beam_lm_search_ref(x[:, :n].cpu().numpy(), il[:n].cpu().numpy(), W, K, 5, T, blank,
                                                      lm.cpu().numpy(), ALPHA, BETA, np.float64)
        counted, worst = 0, 0.0
        for b in range(n):
            s = rs[b, :min(int(rc[b]), 5)]
            if not np.all(s[:-1] - s[1:] > GAP):
                continue
            counted += 1
            m = min(int(rc[b]), NBEST)
            assert (fused.tokens[b, :m].cpu().numpy() == rt[b, :m]).all(), "the fused launch against the host loops"
            for k in range(m):
                worst = max(worst, abs(float(fused.scores[b, k]) - rs[b, k]) / max(1.0, abs(ra[b, k]) + rabs[b, k]),
                            abs(float(fused.ctc_scores[b, k]) - ra[b, k]) / max(1.0, abs(ra[b, k])))
        differ = int((fused.tokens[:, 0] != plain.tokens[:, 0]).any(dim=1).sum())
        graphs = {k: captured(f)[0] for k, f in bodies.items()}
        calls = {k: max(a.calls, int(a.window * 1e6 / timed(g.replay, 3)) + 1) for k, g in graphs.items()}
        times = {k: [] for k in graphs}
        for _ in range(a.rounds):
            for k, g in graphs.items():
                times[k].append(timed(g.replay, calls[k]))
        for k in graphs:
            print("| %d | %d | %d | %s | %s | %s |" % (T, B, C, lattice, k, fmt(times[k])), flush=True)
        med = {k[:4].strip("() "): statistics.median(v) for k, v in times.items()}
        line = "(T=%d B=%d %s: fused / plain = %.4f on the medians, %.2f us per frame fused" % (
            T, B, lattice, med["c"] / med["b"], med["c"] / T)
        if a.parent_lib:
            line += "; parent against itself a2 / a1 = %.4f, this tree's plain against the parent b / a1 = %.4f, b / a2 = %.4f" % (
                med["a2"] / med["a1"], med["b"] / med["a1"], med["b"] / med["a2"])
        print(line + "; the best hypothesis differs from the plain search's in %d of %d samples; %d of %d compared samples "
              "counted, largest score error %.3g of its scale, bound %.0e)" % (differ, B, counted, n, worst, RTOL), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--window", type=float, default=0.2)
    ap.add_argument("--host-samples", type=int, default=1)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    print("device: %s" % torch.cuda.get_device_name(dev), flush=True)
    sweep(a, dev)


if __name__ == "__main__":
    main()
