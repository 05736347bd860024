"""CTC prefix beam search restated in plain Python -- what ctc_amd.blank_beam_search and ctc_amd.noblank_beam_search are
held to (DESIGN.md 3.13 states the rules; tests/test_beam_ref.py checks this restatement against the sum over all
alignments).  Slow and literal on purpose: lists, one candidate at a time, a trie of two lists.

    beam_search_ref(x, in_len, W, K, N, L, blank, dtype)     blank < 0: the no-blank lattice, x holds raw logits

`dtype` is the arithmetic of the probabilities (numpy.float64: the yardstick; numpy.float32: what the kernel's precision
can be expected to give).  The class candidates are always ordered on the raw float32 input, as in the kernel."""
import itertools

import numpy as np

NEG_INF = float("-inf")


def _lae(a, b, dtype):
    """logaddexp in `dtype`: m + log1p(exp(-|a - b|)); -inf where both are"""
    m = a if a > b else b
    if m == NEG_INF:
        return dtype(NEG_INF)
    return dtype(m + np.log1p(np.exp(dtype(-abs(dtype(a - b))))))


def _score_order(c):
    # score descending, then stay before extension, then beam slot ascending, then class rank ascending
    return (-c[0], c[1], c[2], c[3])


def beam_search_sample(x, Tb, W, K, blank, dtype=np.float64):
    """One sample.  x [T,C] float32 (log-probabilities, or raw logits when blank < 0) -> the final beam, best first: a
    list of (tokens tuple, score)."""
    C = x.shape[1]
    ninf = dtype(NEG_INF)
    parent, token = [-1], [-1]                                  # the trie; node 0 is the empty prefix
    # a beam: [pb, pnb, last, node]
    beams = [[dtype(0.0), ninf, -1, 0]]
    for t in range(Tb):
        row = x[t]
        if blank >= 0:
            lp = row.astype(dtype)
            lp_blank = lp[blank]
        else:
            r = row.astype(dtype)
            m = r.max()
            lp = r - (m + np.log(np.exp(r - m).sum(dtype=dtype))) if m > NEG_INF else r
            lp_blank = ninf
        # 1. the K non-blank classes of the largest INPUT values, ties to the lower index, -inf left out
        classes = [c for c in range(C) if c != blank and row[c] > NEG_INF]
        classes.sort(key=lambda c: (-float(row[c]), c))
        classes = classes[:K]
        # 2. stay candidates
        tot = [_lae(pb, pnb, dtype) for pb, pnb, _, _ in beams]
        stay = []
        for i, (pb, pnb, last, node) in enumerate(beams):
            stay.append([dtype(tot[i] + lp_blank), dtype(pnb + lp[last]) if last >= 0 else ninf])
        # 3. extensions: into the stay of the beam that already is this prefix, or a candidate of their own
        cands = []
        is_beam = {(parent[bj[3]], bj[2]): j for j, bj in enumerate(beams)}      # (parent prefix, last token) -> its beam
        for i, (pb, pnb, last, node) in enumerate(beams):
            for rank, c in enumerate(classes):
                if blank < 0 and c == last:
                    continue                                    # (the stay term covers it)
                v = dtype(lp[c] + (pb if c == last else tot[i]))
                j = is_beam.get((node, c))
                if j is not None:
                    stay[j][1] = _lae(stay[j][1], v, dtype)
                else:
                    cands.append((v, 1, i, rank, c))
        for i in range(len(beams)):
            cands.append((_lae(stay[i][0], stay[i][1], dtype), 0, i, 0, -1))
        # 4. selection
        cands = [c for c in cands if c[0] > NEG_INF]
        cands.sort(key=_score_order)
        new = []
        for slot, (score, is_ext, i, rank, c) in enumerate(cands[:W]):
            if is_ext:
                node = 1 + t * W + slot
                while len(parent) <= node:
                    parent.append(-1)
                    token.append(-1)
                parent[node], token[node] = beams[i][3], c
                new.append([ninf, score, c, node])
            else:
                new.append([stay[i][0], stay[i][1], beams[i][2], beams[i][3]])
        beams = new
    final = [(_lae(pb, pnb, dtype), 0, i, 0) for i, (pb, pnb, _, _) in enumerate(beams)]
    final.sort(key=_score_order)
    out = []
    for score, _, i, _ in final:
        toks, node = [], beams[i][3]
        while node > 0:
            toks.append(token[node])
            node = parent[node]
        out.append((tuple(reversed(toks)), float(score)))
    return out


def beam_search_ref(x, in_len, W, K, N, L, blank, dtype=np.float64):
    """The whole batch in the layout of BeamHypotheses.  x [T,B,C] float32 array -> (tokens [B,N,L] int32, lengths [B,N]
    int64, scores [B,N] float32-or-`dtype` as float64 array, count [B] int32)."""
    x = np.asarray(x, dtype=np.float32)
    T, B, C = x.shape
    K = min(K, C - 1 if blank >= 0 else C)
    tokens = np.full((B, N, L), -1, np.int32)
    lengths = np.zeros((B, N), np.int64)
    scores = np.full((B, N), NEG_INF, np.float64)
    count = np.zeros(B, np.int32)
    for b in range(B):
        Tb = min(max(int(in_len[b]), 0), T)
        hyps = beam_search_sample(x[:, b], Tb, W, K, blank, dtype)[:N]
        count[b] = len(hyps)
        for n, (toks, score) in enumerate(hyps):
            lengths[b, n] = len(toks)
            tokens[b, n, :min(len(toks), L)] = toks[:L]
            scores[b, n] = score
    return tokens, lengths, scores, count


def brute_force(x, Tb, blank):
    """{labelling: log P(labelling | x)} from the sum over all C^Tb alignments, in float64.  x [T,C]: log-probabilities,
    or raw logits when blank < 0.  Labellings of probability 0 are left out."""
    C = x.shape[1]
    lp = x[:Tb].astype(np.float64)
    if blank < 0:
        m = lp.max(axis=1, keepdims=True)
        lp = lp - (m + np.log(np.exp(lp - m).sum(axis=1, keepdims=True)))
    prob = {}
    for path in itertools.product(range(C), repeat=Tb):
        logp = sum(lp[t, c] for t, c in enumerate(path))
        if logp == NEG_INF:
            continue
        lab = tuple(c for k, c in enumerate(path) if (k == 0 or c != path[k - 1]) and c != blank)
        prob.setdefault(lab, []).append(logp)
    out = {}
    for lab, terms in prob.items():
        m = max(terms)
        out[lab] = m + float(np.log(np.sum(np.exp(np.asarray(terms) - m))))
    return out
