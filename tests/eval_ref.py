"""CTC evaluation restated in plain Python / numpy -- what ctc_amd.collapse_frames, ctc_amd.edit_distance and
ctc_amd.label_error_rate are held to, bit for bit (tests/test_eval_ref.py checks these restatements on hand-checked cases,
tests/test_eval_gpu.py the kernels against them).  This is also what a user does today after `.cpu()`."""
import numpy as np


def collapse_ref(frames, in_len, blank=None, frame_conf=None, max_tokens=None):
    """frames [B,T] integers, in_len [B] -> (tokens [B,W] int32, lengths [B] int64, start [B,W] int32, end [B,W] int32,
    conf [B,W] float32 or None): maximal runs of equal labels merged, runs of `blank` dropped (None: every run is a token),
    start / end the first and last frame of the run (inclusive), conf the float32 sum of frame_conf over the run in
    ascending t divided (in float32) by the frame count; -1 / -1 / -1 / 0 beyond the count; lengths is the true count even
    beyond W = max_tokens (default T).  Labels are compared and stored through their low 32 bits."""
    frames = np.asarray(frames).astype(np.int64).astype(np.int32)           # (wraps: the low 32 bits)
    B, T = frames.shape
    W = T if max_tokens is None else int(max_tokens)
    tokens = np.full((B, W), -1, np.int32)
    start = np.full((B, W), -1, np.int32)
    end = np.full((B, W), -1, np.int32)
    conf = None if frame_conf is None else np.zeros((B, W), np.float32)
    lengths = np.zeros(B, np.int64)
    for b in range(B):
        Tb, n, t = int(in_len[b]), 0, 0
        while t < Tb:
            e = t
            while e + 1 < Tb and frames[b, e + 1] == frames[b, t]:
                e += 1
            if blank is None or frames[b, t] != blank:
                if n < W:
                    tokens[b, n], start[b, n], end[b, n] = frames[b, t], t, e
                    if conf is not None:
                        acc = np.float32(0.0)
                        for u in range(t, e + 1):
                            acc = np.float32(acc + np.float32(frame_conf[b, u]))
                        conf[b, n] = np.float32(acc / np.float32(e - t + 1))
                n += 1
            t = e + 1
        lengths[b] = n
    return tokens, lengths, start, end, conf


def levenshtein(a, b):
    """the textbook O(NM) recurrence, unit costs"""
    a, b = [int(v) for v in a], [int(v) for v in b]
    row = list(range(len(b) + 1))
    for i in range(1, len(a) + 1):
        new = [i] + [0] * len(b)
        for j in range(1, len(b) + 1):
            new[j] = min(row[j] + 1, new[j - 1] + 1, row[j - 1] + (a[i - 1] != b[j - 1]))
        row = new
    return row[len(b)]


def levenshtein_table(a, b):
    """the same recurrence filled in anti-diagonal by anti-diagonal (every cell of one depends on the two before it only),
    one numpy statement per anti-diagonal: for the long sequences, where the Python loop above takes seconds"""
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    N, M = len(a), len(b)
    D = np.zeros((N + 1, M + 1), np.int64)
    D[:, 0] = np.arange(N + 1)
    D[0, :] = np.arange(M + 1)
    for k in range(2, N + M + 1):
        i = np.arange(max(1, k - M), min(N, k - 1) + 1)
        j = k - i
        D[i, j] = np.minimum(np.minimum(D[i - 1, j] + 1, D[i, j - 1] + 1), D[i - 1, j - 1] + (a[i - 1] != b[j - 1]))
    return int(D[N, M])


def _low32(x):
    return np.asarray(x).astype(np.int64).astype(np.int32)


def edit_distance_ref(hyp, hyp_len, ref, ref_len):
    """hyp [B,N], ref [B,M] integers -> dist [B] int32 between hyp[b,:hyp_len[b]] and ref[b,:ref_len[b]]"""
    hyp, ref = _low32(hyp), _low32(ref)
    out = []
    for b in range(hyp.shape[0]):
        h, r = hyp[b, :int(hyp_len[b])], ref[b, :int(ref_len[b])]
        out.append(levenshtein(h, r) if len(h) * len(r) <= 20000 else levenshtein_table(h, r))
    return np.array(out, np.int32)


def label_error_rate_ref(hyp, hyp_len, ref, ref_len):
    """-> (ler float32 = sum(dist) / max(sum(ref_len), 1), dist [B] int32)"""
    dist = edit_distance_ref(hyp, hyp_len, ref, ref_len)
    total = max(int(np.asarray(ref_len).astype(np.int64).sum()), 1)
    return np.float32(np.float32(int(dist.astype(np.int64).sum())) / np.float32(total)), dist
