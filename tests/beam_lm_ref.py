"""CTC prefix beam search fused with a bigram table, restated in plain Python -- what ctc_amd.blank_beam_search and
ctc_amd.noblank_beam_search are held to when `lm` is given (DESIGN.md 3.14 and include/ctc_amd.h state the rules;
tests/test_beam_lm_ref.py checks this restatement against the sum over all alignments).  tests/beam_ref.py with three
differences: every prefix carries g, the sum of its tokens' increments alpha lm[last or C, c] + beta; the selection key is
the acoustic score + g, and an extension whose table entry is -inf is no candidate; a hypothesis comes with its fused and
its acoustic score.

    beam_lm_search_ref(x, in_len, W, K, N, L, blank, lm, alpha, beta, dtype)     blank < 0: the no-blank lattice

`dtype` is the arithmetic of the probabilities and of g.  The class candidates are ordered on the raw float32 input."""
import numpy as np

from tests.beam_ref import NEG_INF, _lae, _score_order


def beam_lm_search_sample(x, Tb, W, K, blank, lm, alpha, beta, dtype=np.float64):
    """One sample.  x [T,C] float32, lm [C+1,C] float32 -> the final beam, best first: a list of (tokens tuple, fused score,
    acoustic score, lm_abs), lm_abs the sum of |increment| over the tokens (what the fp32 sum of g errs relative to)."""
    C = x.shape[1]
    ninf = dtype(NEG_INF)
    alpha, beta = dtype(alpha), dtype(beta)
    parent, token = [-1], [-1]                                  # the trie; node 0 is the empty prefix
    # a beam: [pb, pnb, last, node, g, lm_abs]
    beams = [[dtype(0.0), ninf, -1, 0, dtype(0.0), 0.0]]
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
        # 1. the K non-blank classes of the largest INPUT values: the table has no say here
        classes = [c for c in range(C) if c != blank and row[c] > NEG_INF]
        classes.sort(key=lambda c: (-float(row[c]), c))
        classes = classes[:K]
        # 2. stay candidates
        tot = [_lae(bm[0], bm[1], dtype) for bm in beams]
        stay = []
        for i, (pb, pnb, last, node, g, ab) in enumerate(beams):
            stay.append([dtype(tot[i] + lp_blank), dtype(pnb + lp[last]) if last >= 0 else ninf])
        # 3. extensions: the acoustic value into the stay of the beam that already is this prefix (its g is untouched), or
        # a candidate of their own under the key v + (g + inc) -- unless the table forbids the bigram
        cands = []
        is_beam = {(parent[bj[3]], bj[2]): j for j, bj in enumerate(beams)}
        for i, (pb, pnb, last, node, g, ab) in enumerate(beams):
            for rank, c in enumerate(classes):
                if blank < 0 and c == last:
                    continue                                    # (the stay term covers it; the diagonal is never read)
                v = dtype(lp[c] + (pb if c == last else tot[i]))
                j = is_beam.get((node, c))
                if j is not None:
                    stay[j][1] = _lae(stay[j][1], v, dtype)
                    continue
                entry = lm[last if last >= 0 else C, c]
                if entry == NEG_INF:
                    continue                                    # forbidden whatever alpha is
                inc = dtype(alpha * dtype(entry) + beta)
                gn = dtype(g + inc)
                cands.append((dtype(v + gn), 1, i, rank, c, v, gn, ab + abs(float(inc))))
        for i in range(len(beams)):
            cands.append((dtype(_lae(stay[i][0], stay[i][1], dtype) + beams[i][4]), 0, i, 0, -1))
        # 4. selection
        cands = [c for c in cands if c[0] > NEG_INF]
        cands.sort(key=_score_order)
        new = []
        for slot, cand in enumerate(cands[:W]):
            i = cand[2]
            if cand[1]:
                node = 1 + t * W + slot
                while len(parent) <= node:
                    parent.append(-1)
                    token.append(-1)
                parent[node], token[node] = beams[i][3], cand[4]
                new.append([ninf, cand[5], cand[4], node, cand[6], cand[7]])
            else:
                new.append([stay[i][0], stay[i][1], beams[i][2], beams[i][3], beams[i][4], beams[i][5]])
        beams = new
    final = [(dtype(_lae(bm[0], bm[1], dtype) + bm[4]), 0, i, 0) for i, bm in enumerate(beams)]
    final.sort(key=_score_order)
    out = []
    for score, _, i, _ in final:
        toks, node = [], beams[i][3]
        while node > 0:
            toks.append(token[node])
            node = parent[node]
        out.append((tuple(reversed(toks)), float(score), float(_lae(beams[i][0], beams[i][1], dtype)), beams[i][5]))
    return out


def beam_lm_search_ref(x, in_len, W, K, N, L, blank, lm, alpha, beta, dtype=np.float64):
    """The whole batch in the layout of FusedBeamHypotheses.  x [T,B,C] float32, lm [C+1,C] float32 -> (tokens [B,N,L] int32,
    lengths [B,N] int64, scores [B,N] float64, count [B] int32, ctc_scores [B,N] float64, lm_abs [B,N] float64)."""
    x = np.asarray(x, dtype=np.float32)
    lm = np.asarray(lm, dtype=np.float32)
    T, B, C = x.shape
    assert lm.shape == (C + 1, C)
    K = min(K, C - 1 if blank >= 0 else C)
    tokens = np.full((B, N, L), -1, np.int32)
    lengths = np.zeros((B, N), np.int64)
    scores = np.full((B, N), NEG_INF, np.float64)
    ctc_scores = np.full((B, N), NEG_INF, np.float64)
    lm_abs = np.zeros((B, N), np.float64)
    count = np.zeros(B, np.int32)
    for b in range(B):
        Tb = min(max(int(in_len[b]), 0), T)
        hyps = beam_lm_search_sample(x[:, b], Tb, W, K, blank, lm, alpha, beta, dtype)[:N]
        count[b] = len(hyps)
        for n, (toks, score, ctc, ab) in enumerate(hyps):
            lengths[b, n] = len(toks)
            tokens[b, n, :min(len(toks), L)] = toks[:L]
            scores[b, n], ctc_scores[b, n], lm_abs[b, n] = score, ctc, ab
    return tokens, lengths, scores, count, ctc_scores, lm_abs


def lm_score(toks, lm, alpha, beta):
    """g of a labelling in float64 (-inf where a bigram or the first token is forbidden) and the sum of |increment|"""
    C = lm.shape[1]
    g, ab, prev = 0.0, 0.0, C
    for c in toks:
        if lm[prev, c] == NEG_INF:
            return NEG_INF, ab
        inc = float(alpha) * float(lm[prev, c]) + float(beta)
        g, ab, prev = g + inc, ab + abs(inc), c
    return g, ab
