#!/usr/bin/env python3
"""What reading bf16 features natively (the *_typed head entries) buys over the cast it replaces.

Forward: ``LSTM_cell._head`` itself on a bf16 ``feat``, two ways in ONE process on the same tensors -- typed path off (the
parent's behaviour: ``feat.float().contiguous()``, then the fp32 launch) and on (the typed launch reads ``feat`` as it lies) --
in train mode (dropout p = 0.3, gradients enabled) and in eval mode (no_grad).  Backward: ``_HeadFn.backward`` on the state a
train-mode forward saved (the bf16 ``feat`` among it, as ``_HeadFn`` saves it), the same two ways, with and without d_feat; only
at the T B inside ``HEAD_BACKWARD_MAX_ROWS`` / ``HEAD_WIDE_BACKWARD_MAX_ROWS``: beyond those gates both sides run
``_head_backward_torch``, the same code.  Every body is captured (``torch.cuda.graph``) after a warm-up on the capture stream;
the two alternate inside each round; a round is at least `--calls` replays and at least `--window` seconds of them between two
device synchronisations (host clock, no profiler attached), reported per replay in microseconds as median [min .. max] over
the rounds.  The results are compared first (eager calls, dropout off so that both sides see the same mask): bitwise, d_feat
against the cast path's fp32 d_feat rounded once to bf16.

    python tools/head_typed_bench.py [--rounds 7] [--calls 10] [--window 0.1]

The rule (r13's): the native path is taken wherever its median is below the minimum of the cast path's rounds at every measured
B and C; the tool prints the largest measured T B up to which that holds (profiles/r19_head_typed.md)."""
import argparse
import os
import statistics
import sys
import types

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import ctc_amd  # noqa: E402
from ctc_amd import producer  # noqa: E402
from tools.head_wide_bench import fmt, gate, measure  # noqa: E402

K = 1024
# the (T, B) points of profiles/r14_head_backward.md and r18_head_wide.md: T B = 100 ... 307200
SHAPES = [(T, B, C) for (T, B) in ((10, 10), (150, 10), (10, 256), (150, 256), (10, 512), (150, 512), (10, 2048), (150, 2048))
          for C in (33, 158)]
LOWP = dict(producer._LOWP_FEAT)


def typed(on):
    """the switch: with no 2-byte dtype known to ``_feat_call`` every entry point casts and takes the fp32 entry, as the parent"""
    producer._LOWP_FEAT = dict(LOWP) if on else {}


def bits_equal(a, b):
    return a.dtype is b.dtype and torch.equal(a.contiguous().view(torch.int16 if a.element_size() == 2 else torch.int32),
                                              b.contiguous().view(torch.int16 if b.element_size() == 2 else torch.int32))


def row(T, B, C, what, times, wins, mb):
    print("| %d | %d | %d | %d | %s | %s | %s | %.3f | %s | %.1f -> %.1f |" % (
        T, B, C, T * B, what, fmt(times["old"]), fmt(times["new"]),
        statistics.median(times["new"]) / statistics.median(times["old"]), "yes" if wins else "no", mb[0], mb[1]), flush=True)


def sweep(a, dev):
    print("| T | B | C | T B | what | cast path, us | native path, us | native / cast | native median < cast min | feat traffic, MB: cast -> native |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    results = []
    for (T, B, C) in SHAPES:
        torch.manual_seed(T + B + C)
        model = ctc_amd.LSTM_cell(types.SimpleNamespace(extract_feat_dim=K, v_class=C, batch_size=B, temporal=T)).to(dev)
        feat = torch.randn(T, B, K, device=dev).to(torch.bfloat16)
        n = T * B * K / 1e6                                              # features, in millions

        def head(on):
            typed(on)
            return model._head(feat)

        for mode in ("train", "eval"):
            model.train(mode == "train")
            grad = torch.enable_grad if mode == "train" else torch.no_grad
            with grad():
                model.v.layers[3].p = 0.0
                assert bits_equal(head(True).detach(), head(False).detach()), (T, B, C, mode)
                model.v.layers[3].p = 0.3
                times, wins = measure(a, {"old": lambda: head(False), "new": lambda: head(True)})
            # cast path: the cast reads 2 and writes 4 bytes per feature, the launch reads 4; native: the launch reads 2 (C <= 48
            # columns are one pass over feat; the wide entry reads it once per group of three column tiles -- not counted)
            row(T, B, C, "forward, %s" % mode, times, wins, (10 * n, 2 * n))
            results.append((T * B, wins))
        wide = B > 256
        if T * B > (producer.HEAD_WIDE_BACKWARD_MAX_ROWS if wide else producer.HEAD_BACKWARD_MAX_ROWS):
            continue
        # the backward on the state of one train-mode forward, as _HeadFn.backward finds it
        model.train(True)
        lin, bn = model.v.layers[0], model.v.layers[1]
        w, gamma, beta = lin.weight.detach(), bn.weight.detach(), bn.bias.detach()
        mask = torch.nn.functional.dropout(torch.ones(T, B, C, device=dev), 0.3, True)
        fwd = producer.head_forward_wide if wide else producer.head_forward
        _, lo, mean, _, inv = fwd(feat, w, lin.bias.detach(), gamma, beta, mask=mask, want_backward_state=True)
        d_out = torch.randn(T, B, C, device=dev)
        for need in (True, False):
            ctx = types.SimpleNamespace(saved_tensors=(feat, w, gamma, beta, lo, mean, inv, mask, None, None), wide=wide,
                                        train=True, eps=1e-5, needs_input_grad=(need, True, True, True, True))

            def backward(on):
                typed(on)
                return producer._HeadFn.backward(ctx, d_out)[:5]

            new, old = backward(True), backward(False)
            if need:
                assert new[0].dtype is torch.bfloat16 and bits_equal(new[0], old[0].to(torch.bfloat16)), (T, B, C)
            assert all(bits_equal(x, y) for x, y in zip(new[1:], old[1:])), (T, B, C, need)
            times, wins = measure(a, {"old": lambda: backward(False), "new": lambda: backward(True)})
            # cast path: the cast (2 + 4), d_weight's read (4), d_feat's write (4); native: 2 and 2
            row(T, B, C, "backward, %s d_feat" % ("with" if need else "no"), times, wins,
                ((14 if need else 10) * n, (4 if need else 2) * n))
            results.append((T * B, wins))
        del model, feat, lo, mask, d_out
        torch.cuda.empty_cache()
    print()
    best, top = gate(results), max(r for r, _ in results)
    print("the native path wins at every measured point up to T B = %d (largest measured: %d)%s"
          % (best, top, ": no gate" if best == top else ": HEAD_TYPED_MAX_ROWS = %d by the rule" % best))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--window", type=float, default=0.1)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    print("device: %s" % torch.cuda.get_device_name(dev), flush=True)
    try:
        sweep(a, dev)
    finally:
        typed(True)


if __name__ == "__main__":
    main()
