"""The numpy restatements of the evaluation (tests/eval_ref.py) on hand-checked cases (runs without a GPU):
tests/test_eval_gpu.py holds the kernels to these restatements, this file holds the restatements to known answers."""
import numpy as np

from tests.eval_ref import collapse_ref, edit_distance_ref, label_error_rate_ref, levenshtein, levenshtein_table

A, Bk = 7, 0                                                   # a label and the blank


def word(s):
    return [ord(c) for c in s]


def test_levenshtein_known_answers():
    assert levenshtein(word("kitten"), word("sitting")) == 3
    assert levenshtein(word("sitting"), word("kitten")) == 3
    assert levenshtein([], []) == 0
    for n in (1, 5, 64):
        assert levenshtein([], list(range(n))) == n
        assert levenshtein(list(range(n)), []) == n
    assert levenshtein(word("flaw"), word("lawn")) == 2
    assert levenshtein([1, 2, 3], [1, 2, 3]) == 0
    assert levenshtein([1, 1, 1, 1], [1, 1]) == 2              # repeated tokens
    assert levenshtein([1, 2, 3], [4, 5, 6, 7, 8]) == 5        # disjoint alphabets: max(N, M)


def test_the_two_forms_of_the_recurrence_agree():
    rng = np.random.default_rng(5)
    assert levenshtein_table(word("kitten"), word("sitting")) == 3
    for n, m in [(0, 0), (0, 7), (7, 0), (1, 1), (5, 9), (30, 17), (64, 65), (40, 130)]:
        for alphabet in (2, 5):
            a, b = rng.integers(0, alphabet, n), rng.integers(0, alphabet, m)
            assert levenshtein_table(a, b) == levenshtein(a, b), (n, m, alphabet)


def test_edit_distance_ref_respects_lengths():
    hyp = np.array([word("kittenXX"), word("sittingQ")], np.int64)
    ref = np.array([word("sittingZ"), word("kittenYY")], np.int32)
    assert edit_distance_ref(hyp, [6, 7], ref, [7, 6]).tolist() == [3, 3]
    assert edit_distance_ref(hyp, [0, 0], ref, [0, 4]).tolist() == [0, 4]
    assert edit_distance_ref(hyp, [0, 0], ref, [0, 4]).dtype == np.int32


def test_label_error_rate_ref():
    hyp = np.array([word("kitten_"), word("sitting")], np.int64)
    ref = np.array([word("sitting"), word("sitting")], np.int64)
    ler, dist = label_error_rate_ref(hyp, [6, 7], ref, [7, 7])
    assert dist.tolist() == [3, 0] and ler == np.float32(3) / np.float32(14) and ler.dtype == np.float32
    ler, dist = label_error_rate_ref(hyp, [6, 2], ref, [0, 0])   # no reference label at all: sum(dist) / 1
    assert dist.tolist() == [6, 2] and ler == np.float32(8)


def test_collapse_known_answers():
    frames = np.array([[A, Bk, A, Bk, Bk, 9],                   # a blank a: two tokens (then a third)
                       [A, A, A, A, A, A],                      # a a ...: one
                       [Bk, Bk, Bk, Bk, Bk, Bk],                # all blank: none
                       [Bk, A, A, 3, 3, Bk],
                       [A, A, 9, 9, 9, 9]], np.int64)
    in_len = [3, 6, 6, 6, 0]
    tokens, lengths, start, end, conf = collapse_ref(frames, in_len, blank=Bk)
    assert conf is None and tokens.shape == (5, 6) and tokens.dtype == np.int32 and lengths.dtype == np.int64
    assert lengths.tolist() == [2, 1, 0, 2, 0]
    assert tokens[0].tolist() == [A, A, -1, -1, -1, -1] and start[0].tolist()[:2] == [0, 2] and end[0].tolist()[:2] == [0, 2]
    assert tokens[1].tolist() == [A, -1, -1, -1, -1, -1] and (start[1, 0], end[1, 0]) == (0, 5)
    assert (tokens[2] == -1).all() and (start[2] == -1).all() and (end[2] == -1).all()
    assert tokens[3].tolist()[:2] == [A, 3] and start[3].tolist()[:2] == [1, 3] and end[3].tolist()[:2] == [2, 4]
    assert (tokens[4] == -1).all()                              # T_b = 0: nothing is read


def test_collapse_without_blank_takes_labels_literally():
    frames = np.array([[0, 0, -1, -1, 0, 2]], np.int32)
    tokens, lengths, start, end, _ = collapse_ref(frames, [6], blank=None)
    assert lengths.tolist() == [4] and tokens[0].tolist() == [0, -1, 0, 2, -1, -1]
    assert start[0].tolist()[:4] == [0, 2, 4, 5] and end[0].tolist()[:4] == [1, 3, 4, 5]


def test_collapse_truncation_keeps_the_true_count():
    frames = np.array([[1, 2, 3, 4, 5, 5]], np.int64)
    tokens, lengths, start, end, _ = collapse_ref(frames, [6], blank=0, max_tokens=3)
    assert tokens.shape == (1, 3) and lengths.tolist() == [5] and tokens[0].tolist() == [1, 2, 3]
    assert start[0].tolist() == [0, 1, 2] and end[0].tolist() == [0, 1, 2]


def test_collapse_confidence_is_a_float32_loop():
    fc = np.array([[0.1, 0.7, 0.2, 0.9, 0.3, 0.6]], np.float32)
    frames = np.array([[4, 4, 4, 0, 5, 5]], np.int64)
    _, lengths, _, _, conf = collapse_ref(frames, [6], blank=0, frame_conf=fc)
    want0 = np.float32(np.float32(np.float32(np.float32(0.1) + np.float32(0.7)) + np.float32(0.2)) / np.float32(3))
    want1 = np.float32(np.float32(np.float32(0.3) + np.float32(0.6)) / np.float32(2))
    assert lengths.tolist() == [2] and conf.dtype == np.float32
    assert conf[0, 0] == want0 and conf[0, 1] == want1 and (conf[0, 2:] == 0).all()
