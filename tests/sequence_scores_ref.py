"""The sequence scores restated in plain float64 -- what ctc_amd.blank_sequence_scores and ctc_amd.noblank_sequence_scores are
held to (include/ctc_amd.h and DESIGN.md 3.15 state the rules; tests/test_sequence_scores_ref.py checks this restatement
against the sum over all alignments and against the oracle's losses).  Slow and literal on purpose.

    sequence_score(x, Tb, labels, blank)                                   one sample [T,C], one sequence
    sequence_scores_ref(x, in_len, seqs, seq_len, counts=None, blank=0)    the batch, in the layout of the functions

blank < 0: the no-blank lattice, x holds raw logits."""
import numpy as np

NEG_INF = float("-inf")
NAN = float("nan")


def _lse(*v):
    m = max(v)
    if m == NEG_INF:
        return NEG_INF
    return m + float(np.log(sum(np.exp(a - m) for a in v)))


def log_rows(x, blank):
    """the rows as the lattices see them, float64: x itself, or x - logsumexp(x) on the no-blank lattice"""
    lp = np.asarray(x, dtype=np.float64)
    if blank < 0:
        m = lp.max(axis=-1, keepdims=True)
        with np.errstate(invalid="ignore", divide="ignore"):
            lp = lp - (m + np.log(np.exp(lp - m).sum(axis=-1, keepdims=True)))
    return lp


def sequence_score(x, Tb, labels, blank):
    """log P(labels | the first Tb rows of x [T,C]), the sum over all alignments; -inf where there is none.  The labels
    are valid (inside [0, C), none equal to the blank)."""
    labels = np.asarray(labels, dtype=np.int64).reshape(-1)
    n = len(labels)
    if Tb == 0:
        return 0.0 if n == 0 else NEG_INF
    lp = log_rows(x[:Tb], blank)
    if blank >= 0:
        # states: blank, label 0, blank, label 1, ..., blank; stay, advance, and skip the blank between unequal labels
        ext = np.full(2 * n + 1, blank, np.int64)
        ext[1::2] = labels
        skip = np.zeros(2 * n + 1, bool)
        skip[3::2] = labels[1:] != labels[:-1]
        start = 2
    else:
        # states: the labels; stay and advance
        if n == 0:
            return NEG_INF
        ext, skip, start = labels, np.zeros(n, bool), 1
    S = len(ext)
    a = np.full(S, NEG_INF)
    a[:start] = lp[0, ext[:start]]
    for t in range(1, Tb):
        below = np.concatenate(([NEG_INF], a[:-1]))
        two_below = np.where(skip, np.concatenate(([NEG_INF, NEG_INF], a[:-2]))[:S], NEG_INF)
        a = np.logaddexp(np.logaddexp(a, below), two_below) + lp[t, ext]
    return float(_lse(a[S - 1], a[S - 2]) if blank >= 0 and S > 1 else a[S - 1])


def sequence_scores_ref(x, in_len, seqs, seq_len, counts=None, blank=0):
    """x [T,B,C]; seqs [B,N,L] or [N,L] (shared by the batch), seq_len [B,N] or [N]; counts [B] or None -> float64 [B,N].
    The special cases in the order of the rules: n >= counts[b]: -inf; a length < 0 or > L: NaN; a label among the first
    `len` outside [0, C) or equal to the blank: NaN; then the score."""
    x = np.asarray(x)
    T, B, C = x.shape
    seqs, seq_len = np.asarray(seqs), np.asarray(seq_len)
    if seqs.ndim == 2:
        seqs = np.broadcast_to(seqs, (B,) + seqs.shape)
        seq_len = np.broadcast_to(seq_len, (B,) + seq_len.shape)
    N, L = seqs.shape[1:]
    out = np.empty((B, N), np.float64)
    for b in range(B):
        Tb = min(max(int(in_len[b]), 0), T)
        for n in range(N):
            ln = int(seq_len[b, n])
            if counts is not None and n >= int(counts[b]):
                out[b, n] = NEG_INF
            elif ln < 0 or ln > L:
                out[b, n] = NAN
            elif any(c < 0 or c >= C or c == blank for c in seqs[b, n, :ln].tolist()):
                out[b, n] = NAN
            else:
                out[b, n] = sequence_score(x[:, b], Tb, seqs[b, n, :ln], blank)
    return out


def all_sequences(symbols, max_len, min_len=0, equal_neighbours=True):
    """every sequence over `symbols` of min_len .. max_len labels, shortest first"""
    out, level = [], [()]
    for n in range(max_len + 1):
        if n >= min_len:
            out.extend(level)
        level = [s + (c,) for s in level for c in symbols if equal_neighbours or not s or s[-1] != c]
    return out


def padded(seqs, L=None, pad=-1, dtype=np.int64):
    """a list of sequences -> ([N,L] array padded with `pad`, [N] lengths)"""
    L = max(1, max(len(s) for s in seqs)) if L is None else L
    arr = np.full((len(seqs), L), pad, dtype)
    for i, s in enumerate(seqs):
        arr[i, :len(s)] = s
    return arr, np.array([len(s) for s in seqs], np.int64)
