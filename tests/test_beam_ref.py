"""tests/beam_ref.py, the yardstick of the beam search kernels, against the sum over all C^T alignments (no GPU): where every
prefix fits in the beam the search is exact, so the hypotheses are the labellings of non-zero probability and every score is
the labelling's log-probability.  Then hand-checked cases for the merge rule and the tie order."""
import math

import numpy as np
import pytest

from tests.beam_ref import beam_search_ref, beam_search_sample, brute_force

NEG_INF = float("-inf")


def _log_softmax(x):
    x = x.astype(np.float64)
    m = x.max(axis=-1, keepdims=True)
    return (x - (m + np.log(np.exp(x - m).sum(axis=-1, keepdims=True)))).astype(np.float32)


def _case(seed, blank):
    rng = np.random.default_rng(seed)
    T = 5 if blank >= 0 else 4
    x = (rng.standard_normal((T, 3)) * 2.0).astype(np.float32)
    if seed % 4 == 3:
        x[rng.integers(T), rng.integers(3)] = NEG_INF          # a cell of probability 0
    return (_log_softmax(x) if blank >= 0 else x), int(rng.integers(0, T + 1)) if seed % 5 else T


@pytest.mark.parametrize("blank", [0, 2, -1])
@pytest.mark.parametrize("seed", range(20))
def test_exact_where_every_prefix_fits(seed, blank):
    x, Tb = _case(seed + 100 * (blank + 1), blank)
    want = brute_force(x, Tb, blank)
    got = beam_search_sample(x, Tb, 64, 3, blank, np.float64)
    assert len(got) == len(set(h for h, _ in got)), "a labelling was returned twice"
    assert set(h for h, _ in got) == set(want)
    for toks, score in got:
        assert abs(score - want[toks]) <= 1e-9, (toks, score, want[toks])
    assert all(got[i][1] >= got[i + 1][1] for i in range(len(got) - 1))
    assert abs(sum(math.exp(s) for _, s in got) - 1.0) <= 1e-5  # the labellings share out the whole probability


def test_float32_arithmetic_stays_close():
    for blank in (0, -1):
        for seed in range(8):
            x, Tb = _case(seed, blank)
            want = brute_force(x, Tb, blank)
            for toks, score in beam_search_sample(x, Tb, 64, 3, blank, np.float32):
                assert abs(score - want[toks]) <= 1e-5 * max(1.0, abs(want[toks]))


def test_merge_rule_by_hand():
    """C = 2 (blank, a), every cell 1/2.  T = 2: `a` collects a-, -a and aa (a, then a again: the same prefix), 3/4.
    T = 3: `aa` is a-a alone (a, blank, a: a new token), 1/8; the empty labelling ---, 1/8; `a` the other six."""
    lp = np.full((3, 2), math.log(0.5), np.float32)
    got = dict(beam_search_sample(lp, 2, 8, 1, 0))
    assert set(got) == {(1,), ()}
    assert got[(1,)] == pytest.approx(math.log(0.75), abs=1e-7) and got[()] == pytest.approx(math.log(0.25), abs=1e-7)
    got = beam_search_sample(lp, 3, 8, 1, 0)
    assert [h for h, _ in got] == [(1,), (), (1, 1)]           # the tie of `` and `aa`: the stay comes first
    assert [s for _, s in got] == pytest.approx([math.log(0.75), math.log(0.125), math.log(0.125)], abs=1e-7)


def test_merge_needs_the_parent_in_the_beam_by_hand():
    """a at frame 0, then blank, then a: with W = 1 the beam holds `a` alone after frame 0, the extension of `a` by a is
    the new prefix `aa` only through the blank-ending part of `a`"""
    p = np.array([[0.1, 0.9], [0.6, 0.4], [0.2, 0.8]])
    lp = np.log(p).astype(np.float32)
    got = dict(beam_search_sample(lp, 3, 64, 1, 0))
    want = brute_force(lp, 3, 0)
    assert got[(1, 1)] == pytest.approx(math.log(0.9 * 0.6 * 0.8), abs=1e-6)
    assert set(got) == set(want) and all(got[k] == pytest.approx(want[k], abs=1e-9) for k in got)


def test_tie_order_by_hand():
    """no-blank lattice, C = 2, constant logits, T = 2: four labellings of probability 1/4 each.  Frame 0 keeps the
    extensions by class 0 and class 1 in that order (equal inputs: the lower class has the lower rank); frame 1 orders the
    ties stay before extension, then by slot."""
    x = np.zeros((2, 2), np.float32)
    got = beam_search_sample(x, 2, 8, 2, -1)
    assert [h for h, _ in got] == [(0,), (1,), (0, 1), (1, 0)]
    assert all(s == pytest.approx(math.log(0.25), abs=1e-7) for _, s in got)
    # the same under a beam of 3: the fourth is cut, not another one
    assert [h for h, _ in beam_search_sample(x, 2, 3, 2, -1)] == [(0,), (1,), (0, 1)]
    # class rank follows the input value first: class 1 now leads
    x[:, 1] = 0.5
    got = beam_search_sample(x, 1, 8, 2, -1)
    assert [h for h, _ in got] == [(1,), (0,)]


def test_batch_layout_padding_and_truncation():
    rng = np.random.default_rng(3)
    x = _log_softmax(rng.standard_normal((6, 3, 4)) * 3.0)
    tokens, lengths, scores, count = beam_search_ref(x, [6, 0, 9], W=4, K=9, N=3, L=2, blank=0)
    assert tokens.shape == (3, 3, 2) and lengths.shape == scores.shape == (3, 3) and count.tolist() == [3, 1, 3]
    assert lengths[1].tolist() == [0, 0, 0] and scores[1, 0] == 0.0 and (scores[1, 1:] == NEG_INF).all()
    assert (tokens[1] == -1).all()
    for b in (0, 2):
        full = beam_search_sample(x[:, b], 6, 4, 3, 0)
        for n in range(3):
            toks = full[n][0]
            assert lengths[b, n] == len(toks)                   # the true count, also beyond L
            assert tokens[b, n].tolist() == (list(toks[:2]) + [-1, -1])[:2]
