"""The gradient of the sequence scores restated in plain float64 -- what ctc_amd_sequence_scores_grad and the autograd of
ctc_amd.blank_sequence_scores / ctc_amd.noblank_sequence_scores are held to (include/ctc_amd.h and DESIGN.md 3.16 state the
rules; tests/test_sequence_scores_grad_ref.py checks this restatement against finite differences, the sum over all
alignments, torch's CPU ctc_loss and the oracle).  A literal alpha / beta pass, slow on purpose.

    sequence_score_grad(x, Tb, labels, blank)                      one sample [T,C], one sequence -> (score, d score / d x)
    sequence_scores_grad_ref(x, in_len, seqs, seq_len, w, counts=None, blank=0)
                                                                   the batch -> (scores [B,N], grad [T,B,C])

blank >= 0: x holds log-probabilities, taken as FREE inputs: d score / d x[t, c] is the occupancy of class c at frame t in
the sequence's own lattice (not torch's exp(x) - occupancy, which folds a log_softmax in).  blank < 0: x holds raw logits,
d score / d x[t, c] = occupancy - softmax(x_t)[c].  Rows t >= Tb are 0; where x is -inf the gradient is 0."""
import numpy as np

from tests.sequence_scores_ref import NEG_INF, log_rows, sequence_scores_ref


def _lattice(labels, blank):
    n = len(labels)
    if blank >= 0:
        ext = np.full(2 * n + 1, blank, np.int64)
        ext[1::2] = labels
        skip = np.zeros(2 * n + 1, bool)
        skip[3::2] = labels[1:] != labels[:-1]
        return ext, skip, 2
    return labels, np.zeros(n, bool), 1


def sequence_score_grad(x, Tb, labels, blank):
    """-> (score, grad [T,C] float64).  The labels are valid.  A score of -inf comes with a gradient of zeros."""
    x = np.asarray(x, dtype=np.float64)
    T, C = x.shape
    labels = np.asarray(labels, dtype=np.int64).reshape(-1)
    grad = np.zeros((T, C))
    if Tb == 0:
        return (0.0 if len(labels) == 0 else NEG_INF), grad
    if blank < 0 and len(labels) == 0:
        return NEG_INF, grad
    lp = log_rows(x[:Tb], blank)
    ext, skip, start = _lattice(labels, blank)
    S = len(ext)
    final = [S - 1, S - 2] if blank >= 0 and S > 1 else [S - 1]
    with np.errstate(invalid="ignore"):
        alpha = np.full((Tb, S), NEG_INF)
        alpha[0, :start] = lp[0, ext[:start]]
        for t in range(1, Tb):
            a = alpha[t - 1]
            below = np.concatenate(([NEG_INF], a[:-1]))
            two_below = np.where(skip, np.concatenate(([NEG_INF, NEG_INF], a[:-2]))[:S], NEG_INF)
            alpha[t] = np.logaddexp(np.logaddexp(a, below), two_below) + lp[t, ext]
        score = float(np.logaddexp.reduce(alpha[Tb - 1, final]))
        if score == NEG_INF:
            return NEG_INF, grad
        # beta WITHOUT the frame's own emission: the log-mass of the ways from (t, s) to the end, frames t + 1 .. Tb - 1
        beta = np.full((Tb, S), NEG_INF)
        beta[Tb - 1, final] = 0.0
        for t in range(Tb - 2, -1, -1):
            nb = beta[t + 1] + lp[t + 1, ext]
            above = np.concatenate((nb[1:], [NEG_INF]))
            # s -> s + 2 is allowed where the state s + 2 may be entered by a skip
            two_above = np.where(np.concatenate((skip[2:], [False, False]))[:S],
                                 np.concatenate((nb[2:], [NEG_INF, NEG_INF]))[:S], NEG_INF)
            beta[t] = np.logaddexp(np.logaddexp(nb, above), two_above)
        gamma = np.exp(alpha + beta - score)                   # (-inf + -inf = -inf: 0; never +inf)
    for s in range(S):
        grad[:Tb, ext[s]] += gamma[:, s]
    if blank < 0:
        grad[:Tb] -= np.exp(lp)
    grad[:Tb][np.isneginf(x[:Tb])] = 0.0
    return score, grad


def sequence_scores_grad_ref(x, in_len, seqs, seq_len, w, counts=None, blank=0):
    """x [T,B,C]; seqs [B,N,L] or [N,L], seq_len [B,N] or [N]; w [B,N]; counts [B] or None -> (scores [B,N] float64 by the
    rules of sequence_scores_ref, grad [T,B,C] float64 = sum over the candidates scored finite of w[b,n] d score / d x).
    A candidate that is not scored finite gives nothing, whatever its w holds."""
    x = np.asarray(x)
    T, B, C = x.shape
    scores = sequence_scores_ref(x, in_len, seqs, seq_len, counts, blank)
    seqs, seq_len, w = np.asarray(seqs), np.asarray(seq_len), np.asarray(w, dtype=np.float64)
    if seqs.ndim == 2:
        seqs = np.broadcast_to(seqs, (B,) + seqs.shape)
        seq_len = np.broadcast_to(seq_len, (B,) + seq_len.shape)
    grad = np.zeros((T, B, C))
    for b in range(B):
        Tb = min(max(int(in_len[b]), 0), T)
        for n in range(seqs.shape[1]):
            if not np.isfinite(scores[b, n]):
                continue
            s, g = sequence_score_grad(x[:, b], Tb, seqs[b, n, :int(seq_len[b, n])], blank)
            assert abs(s - scores[b, n]) <= 1e-9 * max(1.0, abs(s))
            grad[:, b] += w[b, n] * g
    return scores, grad
