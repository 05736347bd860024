"""tests/sequence_scores_ref.py, the float64 restatement the sequence-score kernels are held to, against three independent
yardsticks: the sum over all C^T alignments (tests/beam_ref.brute_force), the oracle's losses (oracle/ctc_numpy), and the
invariant that the probabilities of ALL label sequences sum to 1.  No device."""
import numpy as np
import pytest

from oracle import ctc_numpy
from tests.beam_ref import brute_force
from tests.sequence_scores_ref import NEG_INF, all_sequences, padded, sequence_score, sequence_scores_ref

TOL = 1e-12                                                    # float64 against float64: sums in another order


def rows(seed, T, C, lattice, dtype=np.float32):
    x = np.random.default_rng(seed).standard_normal((T, C)) * 2.0
    if lattice == "blank":
        x = x - np.log(np.exp(x).sum(axis=1, keepdims=True))
    return x.astype(dtype)


def enumeration(lattice):
    """the complete sets of the invariant: blank lattice (blank 0, C = 3): all 63 sequences over {1, 2} of length <= 5;
    no-blank lattice (C = 3): all sequences over {0, 1, 2} without equal neighbours of length 1 .. 5"""
    if lattice == "blank":
        seqs = all_sequences((1, 2), 5)
        assert len(seqs) == 63
    else:
        seqs = all_sequences((0, 1, 2), 5, min_len=1, equal_neighbours=False)
        assert len(seqs) == 3 + 6 + 12 + 24 + 48
    return seqs


@pytest.mark.parametrize("lattice", ["blank", "noblank"])
@pytest.mark.parametrize("Tb", [5, 3, 1])
def test_against_the_sum_over_all_alignments(lattice, Tb):
    blank = 0 if lattice == "blank" else -1
    x = rows(3, 5, 3, lattice)
    bf = brute_force(x, Tb, blank)
    seqs = enumeration(lattice)
    assert set(bf) <= set(seqs)                                 # the enumeration is complete
    for s in bf:                                                # every key of the brute-force dict
        assert abs(sequence_score(x, Tb, s, blank) - bf[s]) <= TOL * max(1.0, abs(bf[s])), s
    for s in seqs:                                              # and every other enumerated sequence has no alignment
        if s not in bf:
            assert sequence_score(x, Tb, s, blank) == NEG_INF, s
    if lattice == "noblank":
        assert sequence_score(x, Tb, (), blank) == NEG_INF     # the empty sequence: only at T_b = 0
        assert sequence_score(x, Tb, (0, 1, 2, 0, 1, 2), blank) == NEG_INF
    assert sequence_score(x, 0, (), blank) == 0.0
    assert sequence_score(x, 0, (1,), blank) == NEG_INF


@pytest.mark.parametrize("lattice", ["blank", "noblank"])
@pytest.mark.parametrize("Tb", [5, 4, 2, 1])
def test_probabilities_of_all_sequences_sum_to_one(lattice, Tb):
    blank = 0 if lattice == "blank" else -1
    x = rows(11, 5, 3, lattice, np.float64)                     # (float32 log-probabilities are normalised to 1e-7 only)
    total = sum(np.exp(sequence_score(x, Tb, s, blank)) for s in enumeration(lattice))
    assert abs(total - 1.0) <= 1e-12


def test_masked_classes_and_the_all_blank_path():
    x = rows(5, 5, 3, "blank")
    assert abs(sequence_score(x, 5, (), 0) - float(x[:, 0].astype(np.float64).sum())) <= TOL
    x[:, 2] = NEG_INF                                           # a masked vocabulary entry
    assert sequence_score(x, 5, (1, 2), 0) == NEG_INF
    assert np.isfinite(sequence_score(x, 5, (1, 1), 0))
    assert sequence_score(x, 2, (1, 1), 0) == NEG_INF           # a repeat needs a blank: three frames
    assert np.isfinite(sequence_score(x, 3, (1, 1), 0))


def test_against_the_oracle_losses():
    T, B, C, S = 12, 4, 6, 5
    rng = np.random.default_rng(7)
    x = (rng.standard_normal((T, B, C)) * 2.0).astype(np.float32)
    lp = (x.astype(np.float64) - np.log(np.exp(x.astype(np.float64)).sum(axis=2, keepdims=True))).astype(np.float32)
    in_len = np.array([12, 9, 12, 5])
    # blank lattice (blank 0): a repeat, a plain one, the empty target, one as long as the clip allows
    tgt = np.array([[1, 1, 2, 3, 0], [4, 5, 1, 0, 0], [0, 0, 0, 0, 0], [2, 3, 4, 5, 1]])
    tl = np.array([4, 3, 0, 5])
    ref = ctc_numpy.blank_ctc(lp, tgt, in_len, tl, np.float64, blank=0, want_grad=False)["nll"]
    got = sequence_scores_ref(lp, in_len, tgt[:, None, :], tl[:, None], blank=0)[:, 0]
    assert np.all(np.isfinite(ref)) and np.abs(got + ref).max() <= 1e-10
    # blank 2
    tgt2 = np.array([[1, 1, 0, 3, 0], [4, 5, 1, 0, 0], [0, 0, 0, 0, 0], [0, 3, 4, 5, 1]])
    ref = ctc_numpy.blank_ctc(lp, tgt2, in_len, tl, np.float64, blank=2, want_grad=False)["nll"]
    got = sequence_scores_ref(lp, in_len, tgt2[:, None, :], tl[:, None], blank=2)[:, 0]
    assert np.abs(got + ref).max() <= 1e-10
    # no-blank lattice: a sequence with equal neighbours among them (two states of the loss's lattice)
    lab = np.array([[1, 1, 2, 3, 0], [4, 5, 1, 0, 0], [0, 3, 0, 0, 0], [2, 3, 4, 5, 1]])
    nl = np.array([4, 3, 1, 5])
    ref = ctc_numpy.noblank_ctc(x, lab, in_len, nl, np.float64, want_grad=False)["nll"]
    got = sequence_scores_ref(x, in_len, lab[:, None, :], nl[:, None], blank=-1)[:, 0]
    assert np.all(ref < 1e12) and np.abs(got + ref).max() <= 1e-10


def test_special_cases_in_their_order():
    x = rows(2, 5, 3, "blank")[:, None, :].repeat(2, axis=1)    # [5, 2, 3]
    seqs, lens = padded([(1, 2), (1,), (2, 0), (1, 7), (2,), (1,)], L=2)
    lens[4], lens[5] = 3, -1                                    # longer than the tensor is wide; negative
    got = sequence_scores_ref(x, [5, 0], seqs, lens, counts=[6, 1], blank=0)
    assert np.isfinite(got[0, :2]).all()
    assert np.isnan(got[0, 2:]).all()                           # the blank as a label, a label >= C, len > L, len < 0
    assert got[1, 0] == NEG_INF and np.all(got[1, 1:] == NEG_INF)   # T_b = 0; rows beyond the count, before anything else
    seqs3 = np.broadcast_to(seqs, (2,) + seqs.shape)
    same = sequence_scores_ref(x, [5, 0], seqs3, np.broadcast_to(lens, (2, 6)), counts=[6, 1], blank=0)
    assert np.array_equal(got, same, equal_nan=True)            # the shared form is the expanded one
    assert sequence_scores_ref(x, [0, 0], np.zeros((1, 1), int), [0], blank=-1)[0, 0] == 0.0
