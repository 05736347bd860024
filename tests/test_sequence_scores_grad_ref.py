"""tests/sequence_scores_grad_ref.py, the float64 alpha / beta restatement the gradient of the sequence scores is held to,
against four independent yardsticks: central finite differences of tests/sequence_scores_ref.sequence_score, the derivative
of the sum over all alignments (tests/beam_ref.brute_force), torch's CPU ctc_loss autograd behind a float64 log_softmax, and
the oracle's no-blank loss gradient.  No device.

Bounds: 1e-9 absolute, float64 against float64, for the three closed-form yardsticks.  Central differences with step h have a
truncation error ~ h^2 f''' / 6 and a rounding error ~ 1e-16 |f| / h: at h = 1e-5 and |f| <= 30 that is 1e-10 + 3e-10, and
the bound for them is FD_TOL = 2e-8 (what finite differences force, nothing else)."""
import itertools

import numpy as np
import pytest

from oracle import ctc_numpy
from tests.sequence_scores_ref import NEG_INF, all_sequences, padded, sequence_score
from tests.sequence_scores_grad_ref import sequence_score_grad, sequence_scores_grad_ref

TOL = 1e-9
FD_TOL = 2e-8
FD_H = 1e-5


def rows(seed, T, C, lattice):
    x = np.random.default_rng(seed).standard_normal((T, C)) * 2.0
    if lattice == "blank":
        x = x - np.log(np.exp(x).sum(axis=1, keepdims=True))
    return x


CASES = [("blank", (1, 2)), ("blank", (1, 1)), ("blank", ()), ("blank", (2, 1, 2)), ("blank", (2, 2, 2)),
         ("noblank", (0, 1)), ("noblank", (1, 1, 2)), ("noblank", (2,)), ("noblank", (0, 1, 2, 0))]


@pytest.mark.parametrize("lattice,labels", CASES)
@pytest.mark.parametrize("Tb", [6, 5])
def test_against_central_differences(lattice, labels, Tb):
    blank = 0 if lattice == "blank" else -1
    x = rows(4, 6, 3, lattice)
    score, grad = sequence_score_grad(x, Tb, labels, blank)
    assert np.isfinite(score) and abs(score - sequence_score(x, Tb, labels, blank)) <= 1e-12
    assert np.all(grad[Tb:] == 0.0)
    worst = 0.0
    for t, c in itertools.product(range(6), range(3)):
        hi, lo = x.copy(), x.copy()
        hi[t, c] += FD_H
        lo[t, c] -= FD_H
        fd = (sequence_score(hi, Tb, labels, blank) - sequence_score(lo, Tb, labels, blank)) / (2 * FD_H)
        worst = max(worst, abs(fd - grad[t, c]))
    assert worst <= FD_TOL, worst


def brute_force_grad(x, Tb, labels, blank):
    """d log P(labels) / d x from the sum over all C^Tb alignments: every alignment of the labelling, weighted by its share
    of the total, gives 1 to the entries it passes (and, on the no-blank lattice, -softmax to its rows)"""
    T, C = x.shape
    lp = x[:Tb].astype(np.float64)
    if blank < 0:
        lp = lp - np.log(np.exp(lp).sum(axis=1, keepdims=True))
    paths, logps = [], []
    for path in itertools.product(range(C), repeat=Tb):
        lab = tuple(c for k, c in enumerate(path) if (k == 0 or c != path[k - 1]) and c != blank)
        if lab == tuple(labels):
            paths.append(path)
            logps.append(sum(lp[t, c] for t, c in enumerate(path)))
    grad = np.zeros((T, C))
    if not paths:
        return NEG_INF, grad
    logps = np.asarray(logps)
    total = logps.max() + np.log(np.exp(logps - logps.max()).sum())
    for path, lg in zip(paths, logps):
        for t, c in enumerate(path):
            grad[t, c] += np.exp(lg - total)
    if blank < 0:
        grad[:Tb] -= np.exp(lp)
    return float(total), grad


@pytest.mark.parametrize("lattice", ["blank", "noblank"])
@pytest.mark.parametrize("Tb", [5, 3, 1])
def test_against_the_derivative_of_the_sum_over_all_alignments(lattice, Tb):
    """T = 5, C = 3: every sequence the collapse can produce (on the no-blank lattice those without equal neighbours: with
    them the lattice is the loss's, not a collapse)"""
    blank = 0 if lattice == "blank" else -1
    x = rows(3, 5, 3, lattice)
    seqs = all_sequences((1, 2), 3) if lattice == "blank" else all_sequences((0, 1, 2), 4, min_len=1, equal_neighbours=False)
    seen = 0
    for s in seqs:
        want, wgrad = brute_force_grad(x, Tb, s, blank)
        score, grad = sequence_score_grad(x, Tb, s, blank)
        if want == NEG_INF:
            assert score == NEG_INF and not grad.any()
            continue
        seen += 1
        assert abs(score - want) <= TOL
        assert np.abs(grad - wgrad).max() <= TOL, s
    assert seen >= 3


def test_blank_lattice_behind_log_softmax_against_torch():
    import torch
    T, B, C, L = 14, 4, 6, 5
    rng = np.random.default_rng(9)
    logits = rng.standard_normal((T, B, C)) * 2.0
    in_len = np.array([14, 9, 14, 11])
    tgt = np.array([[1, 1, 2, 3, 0], [4, 5, 1, 0, 0], [0, 0, 0, 0, 0], [2, 3, 4, 5, 1]])
    tl = np.array([4, 3, 0, 5])
    w = rng.standard_normal(B)
    z = torch.tensor(logits, dtype=torch.float64, requires_grad=True)
    lp = torch.log_softmax(z, dim=2)
    nll = torch.nn.functional.ctc_loss(lp, torch.tensor(tgt), torch.tensor(in_len), torch.tensor(tl), blank=0,
                                       reduction="none")
    (-(nll * torch.tensor(w))).sum().backward()
    scores, g = sequence_scores_grad_ref(lp.detach().numpy(), in_len, tgt[:, None, :], tl[:, None], w[:, None], blank=0)
    assert np.abs(scores[:, 0] + nll.detach().numpy()).max() <= TOL
    # the free-input gradient, pulled back through the log_softmax: g - softmax * rowsum(g)
    p = np.exp(lp.detach().numpy())
    pulled = g - p * g.sum(axis=2, keepdims=True)
    assert np.abs(pulled - z.grad.numpy()).max() <= TOL
    # the occupancy of every live row sums to the sample's weight
    for b in range(B):
        assert np.abs(g[:in_len[b], b].sum(axis=1) - w[b]).max() <= TOL
        assert not g[in_len[b]:, b].any()


def test_noblank_lattice_against_the_oracle_gradient():
    T, B, C = 12, 4, 6
    rng = np.random.default_rng(7)
    x = rng.standard_normal((T, B, C)) * 2.0
    in_len = np.array([12, 9, 12, 5])
    lab = np.array([[1, 1, 2, 3, 0], [4, 5, 1, 0, 0], [0, 3, 0, 0, 0], [2, 3, 4, 5, 1]])
    nl = np.array([4, 3, 1, 5])
    ref = ctc_numpy.noblank_ctc(x, lab, in_len, nl, np.float64, scale=1.0)
    w = rng.standard_normal(B)
    scores, g = sequence_scores_grad_ref(x, in_len, lab[:, None, :], nl[:, None], w[:, None], blank=-1)
    assert np.all(ref["nll"] < 1e12) and np.abs(scores[:, 0] + ref["nll"]).max() <= TOL
    assert np.abs(g + ref["grad"] * w[None, :, None]).max() <= TOL


def test_special_cases():
    x = rows(2, 5, 3, "blank")[:, None, :].repeat(3, axis=1)    # [5, 3, 3]
    x[:, 2, 2] = NEG_INF                                        # sample 2: class 2 masked
    seqs, lens = padded([(1, 2), (1,), (2, 0), (1, 7), (2,), ()], L=2)
    lens[4] = 3
    w = np.array([[1.0, -2.0, np.nan, np.inf, np.nan, 0.5]] * 3)
    scores, g = sequence_scores_grad_ref(x, [5, 0, 5], seqs, lens, w, counts=[6, 6, 5], blank=0)
    assert not np.isnan(g).any()
    assert not g[:, 1].any()                                    # T_b = 0
    assert np.isneginf(scores[2, 0]) and np.isneginf(scores[2, 5])      # crosses the masked class; beyond the count
    assert not g[:, 2, 2].any()
    _, only = sequence_score_grad(x[:, 2], 5, (1,), 0)
    assert np.abs(g[:, 2] + 2.0 * only).max() <= TOL            # sample 2: candidate 1 alone is scored finite
    # the all-blank path: 1 on the blank column
    _, e = sequence_score_grad(x[:, 0], 4, (), 0)
    assert np.abs(e[:4, 0] - 1.0).max() <= TOL and not e[:, 1:].any() and not e[4:].any()
    # a sample none of whose candidates is scored: zeros
    _, z = sequence_scores_grad_ref(x, [5, 5, 5], seqs[2:5], lens[2:5], w[:, 2:5], blank=0)
    assert not z.any()
