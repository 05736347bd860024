"""tests/beam_lm_ref.py, the yardstick of the fused beam search, without a GPU: with a table of zeros it is
tests/beam_ref.py; where every prefix fits in the beam the hypotheses are the labellings of non-zero probability without a
forbidden bigram, the acoustic score is the labelling's log-probability from the sum over all alignments, and the fused
score is that + g(labelling)."""
import numpy as np
import pytest

from tests.beam_lm_ref import beam_lm_search_ref, beam_lm_search_sample, lm_score
from tests.beam_ref import beam_search_sample, brute_force

NEG_INF = float("-inf")


def _log_softmax(x):
    x = x.astype(np.float64)
    m = x.max(axis=-1, keepdims=True)
    return (x - (m + np.log(np.exp(x - m).sum(axis=-1, keepdims=True)))).astype(np.float32)


def _table(rng, C, forbidden):
    lm = _log_softmax(rng.standard_normal((C + 1, C)) * 1.5)
    lm[rng.random((C + 1, C)) < forbidden] = NEG_INF
    return lm


def _case(seed, blank, T, C):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((T, C)) * 2.0).astype(np.float32)
    return (_log_softmax(x) if blank >= 0 else x), rng


@pytest.mark.parametrize("blank", [0, 3, -1])
@pytest.mark.parametrize("seed", range(6))
def test_zero_table_is_the_plain_search(seed, blank):
    """beam smaller than the set of prefixes, so pruning happens: the same list, bit for bit, whatever alpha is"""
    x, rng = _case(seed + 50 * (blank + 1), blank, 12, 6)
    want = beam_search_sample(x, 12, 5, 3, blank, np.float64)
    got = beam_lm_search_sample(x, 12, 5, 3, blank, np.zeros((7, 6), np.float32), 0.7, 0.0, np.float64)
    assert [(h, s) for h, s, _, _ in got] == want
    assert all(s == a and ab == 0.0 for _, s, a, ab in got)


@pytest.mark.parametrize("blank", [0, 2, -1])
@pytest.mark.parametrize("seed", range(12))
def test_exact_where_every_prefix_fits(seed, blank):
    T, C = (5 if blank >= 0 else 4), 3
    x, rng = _case(seed + 100 * (blank + 1), blank, T, C)
    Tb = int(rng.integers(0, T + 1)) if seed % 4 else T
    lm = _table(rng, C, 0.15)
    alpha, beta = 0.8, 0.4
    acoustic = brute_force(x, Tb, blank)
    want = {lab: (p, lm_score(lab, lm, alpha, beta)[0]) for lab, p in acoustic.items()}
    want = {lab: (p, g) for lab, (p, g) in want.items() if g > NEG_INF}
    got = beam_lm_search_sample(x, Tb, 64, 32, blank, lm, alpha, beta, np.float64)
    assert len(got) == len(set(h for h, _, _, _ in got)), "a labelling was returned twice"
    assert set(h for h, _, _, _ in got) == set(want)
    for toks, fused, ctc, ab in got:
        p, g = want[toks]
        assert abs(ctc - p) <= 1e-12, (toks, ctc, p)
        assert abs(fused - (p + g)) <= 1e-12, (toks, fused, p + g)
        assert ab == pytest.approx(lm_score(toks, lm, alpha, beta)[1], abs=1e-12)
    assert all(got[i][1] >= got[i + 1][1] for i in range(len(got) - 1))


def test_forbidden_whatever_the_weight():
    """alpha = 0: a finite table has no say, a -inf entry still forbids"""
    x, rng = _case(7, 0, 5, 3)
    lm = np.zeros((4, 3), np.float32)
    lm[1, 2] = lm[3, 2] = NEG_INF                              # 2 never follows 1 and never starts (class 0 is the blank)
    got = beam_lm_search_sample(x, 5, 64, 32, 0, lm, 0.0, 0.0, np.float64)
    want = {lab: p for lab, p in brute_force(x, 5, 0).items() if lm_score(lab, lm, 0.0, 0.0)[0] > NEG_INF}
    assert set(h for h, _, _, _ in got) == set(want) and len(want) < len(brute_force(x, 5, 0))
    assert all(lab[:1] != (2,) and (1, 2) not in zip(lab, lab[1:]) for lab in want)
    assert all(fused == ctc for _, fused, ctc, _ in got)


def test_the_table_changes_what_survives():
    """a beam of 2: the bonus keeps longer prefixes alive that the plain search prunes (so the prior cannot be applied to
    the plain search's n-best list afterwards)"""
    rng = np.random.default_rng(3)
    x = _log_softmax(rng.standard_normal((10, 5)) * 1.0)
    plain = [h for h, _ in beam_search_sample(x, 10, 2, 4, 0)]
    fused = [h for h, _, _, _ in beam_lm_search_sample(x, 10, 2, 4, 0, np.zeros((6, 5), np.float32), 1.0, 2.0)]
    assert set(fused) != set(plain) and max(map(len, fused)) > max(map(len, plain))


def test_start_row_forbidden():
    x, rng = _case(9, 0, 4, 3)
    lm = np.zeros((4, 3), np.float32)
    lm[3] = NEG_INF
    got = beam_lm_search_sample(x, 4, 8, 2, 0, lm, 1.0, 0.0)
    assert [h for h, _, _, _ in got] == [()] and got[0][1] == pytest.approx(float(x[:, 0].astype(np.float64).sum()), abs=1e-12)
    assert beam_lm_search_sample(x, 4, 8, 3, -1, lm, 1.0, 0.0) == []
    assert [h for h, _, _, _ in beam_lm_search_sample(x, 0, 8, 3, -1, lm, 1.0, 0.0)] == [()]


def test_batch_layout():
    rng = np.random.default_rng(4)
    x = _log_softmax(rng.standard_normal((6, 3, 4)) * 3.0)
    lm = _table(rng, 4, 0.1)
    tokens, lengths, scores, count, ctc, lm_abs = beam_lm_search_ref(x, [6, 0, 9], 4, 9, 3, 2, 0, lm, 0.8, 0.5)
    assert tokens.shape == (3, 3, 2) and lengths.shape == scores.shape == ctc.shape == lm_abs.shape == (3, 3)
    assert count[1] == 1 and scores[1, 0] == 0.0 and ctc[1, 0] == 0.0 and (scores[1, 1:] == NEG_INF).all()
    assert (ctc[1, 1:] == NEG_INF).all() and (tokens[1] == -1).all()
    for b in (0, 2):
        full = beam_lm_search_sample(x[:, b], 6, 4, 3, 0, lm, 0.8, 0.5)
        for n in range(int(count[b])):
            toks = full[n][0]
            assert lengths[b, n] == len(toks) and tokens[b, n].tolist() == (list(toks[:2]) + [-1, -1])[:2]
            assert (scores[b, n], ctc[b, n], lm_abs[b, n]) == full[n][1:]
