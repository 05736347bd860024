"""The fused beam search on the MI355X: ctc_amd.blank_beam_search / ctc_amd.noblank_beam_search with a bigram
table `lm` -- against the plain search where the table has no say, against the sum over all alignments where the search is
exact, against the float64 restatement of the rules (tests/beam_lm_ref.py) elsewhere, and against the exact probability of
every hypothesis.

Tolerances.  Acoustic scores: the project's RTOL max(1, |ref|).  Fused scores: RTOL max(1, |ctc_ref| + lm_abs_ref), lm_abs
the sum of the |increments| of the hypothesis's tokens: the fp32 sum of n increments errs by at most about n 2^-24 of the
sum of their magnitudes (n <= ~60 tokens here: 4e-6), not relative to a fused value that may cancel towards 0.  As in
tests/test_beam_search_gpu.py no check depends on how a near-tie falls: a sample counts where the restatement's own best five
FUSED scores lie more than GAP apart, and at most a quarter of a case's samples may be left out."""
import functools

import numpy as np
import pytest
import torch

from tests.beam_lm_ref import beam_lm_search_ref, lm_score
from tests.beam_ref import brute_force
from tests.test_beam_search_gpu import (CASES, GAP, LATTICES, NEG_INF, RTOL, case_inputs, check_padding, counted_samples,
                                        exact_log_prob, lattice_input, log_softmax32, planted, tol)

pytestmark = pytest.mark.gpu

ALPHA = 0.8
BETA = {"blank": 0.5, "noblank": -0.5}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    import ctc_amd  # noqa: F401  (raises if libctc_amd.so is missing)
    return torch.device("cuda:0")


def table(seed, C, forbidden=0.1):
    """the recipe: log-softmax rows of 1.5 x unit noise, then -inf where a uniform draw of the same generator is below
    `forbidden`"""
    rng = np.random.default_rng(seed + 1000)
    lm = log_softmax32(rng.standard_normal((C + 1, C)) * 1.5)
    lm[rng.random((C + 1, C)) < forbidden] = NEG_INF
    return lm


def search(dev, x, in_len, blank, W, K, N, lm, alpha, beta, L=None):
    """the kernel -> numpy (tokens, lengths, scores, count, ctc_scores); lm None: the plain call's four"""
    import ctc_amd
    xd = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    il = torch.as_tensor(np.asarray(in_len), dtype=torch.int64).to(dev)
    kw = dict(beam_width=W, nbest=N, top_classes=K, max_tokens=L)
    if lm is not None:
        kw.update(lm=lm if isinstance(lm, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(lm)).to(dev),
                  lm_weight=alpha, token_bonus=beta)
    if blank >= 0:
        h = ctc_amd.blank_beam_search(xd, il, blank=blank, **kw)
    else:
        h = ctc_amd.noblank_beam_search(xd, il, **kw)
    torch.cuda.synchronize()
    if lm is not None:
        T, B = xd.shape[0], xd.shape[1]
        assert isinstance(h, ctc_amd.FusedBeamHypotheses)
        assert h.tokens.shape == (B, N, T if L is None else L) and h.tokens.dtype == torch.int32
        assert h.lengths.shape == (B, N) and h.lengths.dtype == torch.int64
        assert h.scores.shape == (B, N) and h.scores.dtype == torch.float32
        assert h.ctc_scores.shape == (B, N) and h.ctc_scores.dtype == torch.float32
        assert h.count.shape == (B,) and h.count.dtype == torch.int32
    else:
        assert isinstance(h, ctc_amd.BeamHypotheses)
    return tuple(v.cpu().numpy() for v in h)


def check_both_paddings(got, L):
    """check_padding's rules on both score outputs: rows at and beyond count hold -1 / 0 / -inf, the rows before finite
    scores; the FUSED scores do not rise (the acoustic ones may: they do not order the hypotheses)"""
    tokens, lengths, scores, count, ctc = got
    check_padding((tokens, lengths, scores, count), L)
    for b in range(len(count)):
        n = int(count[b])
        assert (ctc[b, n:] == NEG_INF).all() and np.all(np.isfinite(ctc[b, :n]))


def fused_tol(ctc_ref, lm_abs_ref):
    return RTOL * max(1.0, abs(ctc_ref) + lm_abs_ref)


def check_against_restatement(got, ref, N, L, what):
    """got = the kernel's five arrays, ref = beam_lm_search_ref's six (five hypotheses per sample) -> the largest score
    error over its tolerance, acoustic and fused"""
    rt, rl, rs, rc, ra, rabs = ref
    keep = counted_samples(rs, rc)
    assert (~keep).sum() * 4 <= len(keep), "%s: %d of %d samples are near-ties" % (what, (~keep).sum(), len(keep))
    tokens, lengths, scores, count, ctc = got
    worst_ctc = worst_fused = 0.0
    for b in np.nonzero(keep)[0]:
        n = min(int(rc[b]), N)
        assert count[b] == n, (what, b, count[b], n)
        assert lengths[b, :n].tolist() == rl[b, :n].tolist(), (what, b)
        assert tokens[b, :n].tolist() == rt[b, :n, :L].tolist(), (what, b)
        for k in range(n):
            ec, ef = abs(float(ctc[b, k]) - ra[b, k]), abs(float(scores[b, k]) - rs[b, k])
            worst_ctc = max(worst_ctc, ec / tol(ra[b, k]))
            worst_fused = max(worst_fused, ef / fused_tol(ra[b, k], rabs[b, k]))
            assert ec <= tol(ra[b, k]), (what, b, k, float(ctc[b, k]), ra[b, k])
            assert ef <= fused_tol(ra[b, k], rabs[b, k]), (what, b, k, float(scores[b, k]), rs[b, k])
    check_both_paddings(got, L)
    print("%s: %d of %d samples counted, worst error / tolerance: acoustic %.3g, fused %.3g" % (
        what, keep.sum(), len(keep), worst_ctc, worst_fused))
    return worst_ctc, worst_fused


# ---------------------------------------------------------------------------------------------------------------------------
# 1. a table of zeros: the plain search, bit for bit
# ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lattice", LATTICES)
def test_zero_table_gives_the_plain_bits(dev, lattice):
    x, in_len, blank = case_inputs("A", lattice)
    (T, C, W, K, B) = CASES["A"][0]
    plain = search(dev, x, in_len, blank, W, K, 4, None, 1.0, 0.0)
    fused = search(dev, x, in_len, blank, W, K, 4, np.zeros((C + 1, C), np.float32), 0.7, 0.0)
    for name, u, v in zip(("tokens", "lengths", "scores", "count"), plain, fused):
        assert u.tobytes() == v.tobytes(), name
    assert fused[4].tobytes() == fused[2].tobytes()
    check_both_paddings(fused, T)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. the exact regime: every prefix fits in the beam
# ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lattice", LATTICES)
def test_exact_regime(dev, lattice):
    """C = 3, T_b <= 5 (blank) / 4 (no-blank), W = 64: the hypotheses are the labellings of non-zero probability without a
    forbidden bigram; acoustic score = log-probability from the sum over all alignments, fused = that + g"""
    T, B, C = (5, 16, 3) if lattice == "blank" else (4, 16, 3)
    alpha, beta = 0.8, 0.4
    rng = np.random.default_rng(11)
    x, blank = lattice_input((rng.standard_normal((T, B, C)) * 2.0).astype(np.float32), lattice, blank=0)
    in_len = np.array(list(range(T + 1)) + [int(v) for v in rng.integers(0, T + 1, B - T - 3)] + [T, T])
    assert len(in_len) == B
    lm = table(11, C, forbidden=0.15)
    got = search(dev, x, in_len, blank, 64, 32, 64, lm, alpha, beta)
    tokens, lengths, scores, count, ctc = got
    worst_ctc = worst_fused = 0.0
    for b in range(B):
        acoustic = brute_force(x[:, b], int(in_len[b]), blank)
        want = {lab: (p,) + lm_score(lab, lm, alpha, beta) for lab, p in acoustic.items()}
        want = {lab: v for lab, v in want.items() if v[1] > NEG_INF}
        n = int(count[b])
        assert n == len(want), (b, n, len(want))
        hyps = [tuple(tokens[b, k, :lengths[b, k]].tolist()) for k in range(n)]
        assert set(hyps) == set(want) and len(set(hyps)) == n, b
        for k in range(n):
            p, g, ab = want[hyps[k]]
            ec, ef = abs(float(ctc[b, k]) - p), abs(float(scores[b, k]) - (p + g))
            worst_ctc, worst_fused = max(worst_ctc, ec / tol(p)), max(worst_fused, ef / fused_tol(p, ab))
            assert ec <= tol(p), (b, hyps[k], float(ctc[b, k]), p)
            assert ef <= fused_tol(p, ab), (b, hyps[k], float(scores[b, k]), p + g)
        for k in range(n - 1):                                                  # best first, up to the tolerance
            (p0, g0, a0), (p1, g1, a1) = want[hyps[k]], want[hyps[k + 1]]
            assert p0 + g0 >= p1 + g1 - fused_tol(p0, a0) - fused_tol(p1, a1), (b, hyps[k], hyps[k + 1])
    assert count[0] == 1 and lengths[0, 0] == 0 and scores[0, 0] == 0.0 and ctc[0, 0] == 0.0     # T_b = 0
    check_both_paddings(got, T)
    print("exact regime, %s: worst error / tolerance: acoustic %.3g, fused %.3g" % (lattice, worst_ctc, worst_fused))


# ---------------------------------------------------------------------------------------------------------------------------
# 3. against the float64 restatement; 6. soundness
# ---------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def case_table(name):
    (T, C, W, K, B), _, seed = CASES[name]
    return table(seed, C)


@functools.lru_cache(maxsize=None)
def case_result(name, lattice):
    """the kernel's four hypotheses of a case under its table (one launch per case and lattice, shared by the tests)"""
    x, in_len, blank = case_inputs(name, lattice)
    (T, C, W, K, B) = CASES[name][0]
    return search(torch.device("cuda:0"), x, in_len, blank, W, K, 4, case_table(name), ALPHA, BETA[lattice])


@functools.lru_cache(maxsize=None)
def case_reference(name, lattice):
    x, in_len, blank = case_inputs(name, lattice)
    (T, C, W, K, B) = CASES[name][0]
    return beam_lm_search_ref(x, in_len, W, K, min(5, W), T, blank, case_table(name), ALPHA, BETA[lattice], np.float64)


@pytest.mark.parametrize("lattice", LATTICES)
@pytest.mark.parametrize("name", sorted(CASES))
def test_against_float64_restatement(dev, name, lattice):
    (T, C, W, K, B) = CASES[name][0]
    check_against_restatement(case_result(name, lattice), case_reference(name, lattice), 4, T,
                              "case %s, %s" % (name, lattice))


@pytest.mark.parametrize("lattice", LATTICES)
def test_the_table_changes_the_best_hypothesis(dev, lattice):
    """case A: under the table the best hypothesis is another one than the plain search's in every sample -- what this file
    checks is not the plain search"""
    x, in_len, blank = case_inputs("A", lattice)
    (T, C, W, K, B) = CASES["A"][0]
    plain = search(dev, x, in_len, blank, W, K, 4, None, 1.0, 0.0)
    fused = case_result("A", lattice)
    for b in range(B):
        assert (plain[1][b, 0], plain[0][b, 0].tolist()) != (fused[1][b, 0], fused[0][b, 0].tolist()), b


@pytest.mark.parametrize("lattice", LATTICES)
def test_ctc_scores_never_exceed_the_exact_probability(dev, lattice):
    """case A, every returned hypothesis: the search sums a subset of the hypothesis's alignments, with or without a table"""
    x, in_len, blank = case_inputs("A", lattice)
    tokens, lengths, scores, count, ctc = case_result("A", lattice)
    assert (count >= 1).all()
    for k in range(4):
        exact = exact_log_prob(x, in_len, blank, tokens[:, k], lengths[:, k])
        for b in range(len(in_len)):
            if k < count[b]:
                assert float(ctc[b, k]) <= exact[b] + tol(exact[b]), (b, k, float(ctc[b, k]), exact[b])


# ---------------------------------------------------------------------------------------------------------------------------
# 4. a grammar; 5. a start row that forbids every class
# ---------------------------------------------------------------------------------------------------------------------------

def grammar(C, blank):
    """0 / -inf: class c may be followed by the next and the next but one (cyclically, over the non-blank classes) only; a
    sequence starts with class 1, 2 or 3"""
    classes = [c for c in range(C) if c != blank]
    lm = np.full((C + 1, C), NEG_INF, np.float32)
    for k, c in enumerate(classes):
        lm[c, classes[(k + 1) % len(classes)]] = lm[c, classes[(k + 2) % len(classes)]] = 0.0
    lm[C, 1:4] = 0.0
    return lm


@pytest.mark.parametrize("lattice", LATTICES)
def test_grammar(dev, lattice):
    T, C, W, K, B = 30, 10, 16, 8, 8
    raw = (np.random.default_rng(90).standard_normal((T, B, C)) * 2.0).astype(np.float32)
    x, blank = lattice_input(raw, lattice)
    in_len = np.array([T, T, T, 17, 5, 1, T, T])
    lm = grammar(C, blank)
    got = search(dev, x, in_len, blank, W, K, 4, lm, 1.0, 0.0)
    tokens, lengths, scores, count, ctc = got
    assert (count >= 1).all() and lengths[:, 0].max() > 2
    for b in range(B):
        for k in range(int(count[b])):
            toks = tokens[b, k, :lengths[b, k]].tolist()
            assert lm_score(toks, lm, 1.0, 0.0)[0] == 0.0, (b, k, toks)          # no forbidden bigram, no forbidden start
    assert scores.tobytes() == ctc.tobytes()
    ref = beam_lm_search_ref(x, in_len, W, K, 5, T, blank, lm, 1.0, 0.0, np.float64)
    check_against_restatement(got, ref, 4, T, "grammar, %s" % lattice)


def test_start_row_forbids_everything(dev):
    T, C, B = 6, 5, 4
    raw = (np.random.default_rng(91).standard_normal((T, B, C)) * 2.0).astype(np.float32)
    lm = table(91, C)
    lm[C] = NEG_INF
    in_len = np.array([6, 3, 1, 6])
    x, blank = lattice_input(raw, "blank")
    got = search(dev, x, in_len, blank, 8, 4, 4, lm, ALPHA, 0.5)
    tokens, lengths, scores, count, ctc = got
    assert count.tolist() == [1] * B and (lengths == 0).all() and (tokens == -1).all()
    for b in range(B):
        want = float(x[:in_len[b], b, blank].astype(np.float64).sum())          # the all-blank alignment
        assert abs(float(scores[b, 0]) - want) <= tol(want) and scores[b, 0] == ctc[b, 0]
    check_both_paddings(got, T)
    x, blank = lattice_input(raw, "noblank")
    got = search(dev, x, in_len, blank, 8, 4, 4, lm, ALPHA, -0.5)
    tokens, lengths, scores, count, ctc = got
    assert count.tolist() == [0] * B and (tokens == -1).all() and (lengths == 0).all()
    assert (scores == NEG_INF).all() and (ctc == NEG_INF).all()


# ---------------------------------------------------------------------------------------------------------------------------
# 7. edges
# ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lattice", LATTICES)
def test_edge_views(dev, lattice):
    """the table as a view big[:, :C] of a [C+1, C+7] tensor and the logits as a view of a wider batch: read through their
    strides, the bits of the contiguous call"""
    B, T, C = 6, 20, 10
    raw = planted(66, T, B + 5, C, 3.0)
    x, blank = lattice_input(raw, lattice)
    in_len = np.array([20, 7, 20, 0, 1, 20])
    lm = table(66, C)
    big = torch.full((C + 1, C + 7), float("nan"), device=dev)
    big[:, :C] = torch.from_numpy(lm).to(dev)
    wide = torch.from_numpy(x).to(dev)
    alone = search(dev, wide[:, :B].contiguous(), in_len, blank, 8, 4, 4, lm, ALPHA, BETA[lattice])
    assert not big[:, :C].is_contiguous()
    for xs, table_ in ((wide[:, :B], big[:, :C]), (wide[:, :B].contiguous(), big[:, :C]), (wide[:, :B], lm),
                       (wide[:, :B], big.t().contiguous().t()[:, :C])):      # the last: another column stride, copied
        got = search(dev, xs, in_len, blank, 8, 4, 4, table_, ALPHA, BETA[lattice])
        assert all(a.tobytes() == g.tobytes() for a, g in zip(alone, got))
    ref = beam_lm_search_ref(x[:, :B], in_len, 8, 4, 5, T, blank, lm, ALPHA, BETA[lattice], np.float64)
    check_against_restatement(alone, ref, 4, T, "views, %s" % lattice)


@pytest.mark.parametrize("lattice", LATTICES)
def test_edge_truncated_tokens(dev, lattice):
    """max_tokens = 3 under longer results: lengths are the true counts, tokens the first three, scores the same"""
    raw = planted(63, 40, 8, 10, 4.0)
    x, blank = lattice_input(raw, lattice)
    in_len = np.full(8, 40)
    lm = table(63, 10)
    got = search(dev, x, in_len, blank, 8, 4, 4, lm, ALPHA, BETA[lattice], L=3)
    full = search(dev, x, in_len, blank, 8, 4, 4, lm, ALPHA, BETA[lattice])
    assert (got[1][:, 0] > 3).all()
    assert (full[0][:, :, :3] == got[0]).all() and all(full[k].tobytes() == got[k].tobytes() for k in (1, 2, 3, 4))
    check_both_paddings(got, 3)
    ref = beam_lm_search_ref(x, in_len, 8, 4, 5, 40, blank, lm, ALPHA, BETA[lattice], np.float64)
    check_against_restatement(got, ref, 4, 3, "max_tokens=3, %s" % lattice)


@pytest.mark.parametrize("lattice", LATTICES)
def test_edge_more_than_one_row_pass(dev, lattice):
    """C = 1500: the row takes two passes, the table has 1501 rows of 1500"""
    T, B, C, W, K = 6, 4, 1500, 4, 4
    raw = planted(92, T, B, C, 8.0)
    x, blank = lattice_input(raw, lattice)
    in_len = np.full(B, T)
    lm = table(92, C)
    got = search(dev, x, in_len, blank, W, K, 4, lm, ALPHA, BETA[lattice])
    ref = beam_lm_search_ref(x, in_len, W, K, 4, T, blank, lm, ALPHA, BETA[lattice], np.float64)
    check_against_restatement(got, ref, 4, T, "C=1500, %s" % lattice)


def test_python_refusals_on_the_device(dev):
    """with the logits accepted, the table's own refusals are reached: ValueError before the library is called"""
    import ctc_amd
    x = torch.zeros(6, 2, 5, device=dev)
    good = torch.zeros(6, 5, device=dev)
    for fn in (ctc_amd.blank_beam_search, ctc_amd.noblank_beam_search):
        with pytest.raises(ValueError, match="need a table"):
            fn(x, [6, 6], lm_weight=0.5)
        with pytest.raises(ValueError, match="need a table"):
            fn(x, [6, 6], token_bonus=0.5)
        for bad in (good.cpu(), good.double(), torch.zeros(5, 5, device=dev), torch.zeros(6, 6, device=dev), [[0.0]]):
            with pytest.raises(ValueError, match="lm must be"):
                fn(x, [6, 6], lm=bad)
        for kw in (dict(lm_weight=-0.1), dict(lm_weight=float("nan")), dict(lm_weight=float("inf")),
                   dict(token_bonus=float("nan")), dict(token_bonus=float("-inf"))):
            with pytest.raises(ValueError, match="finite"):
                fn(x, [6, 6], lm=good, **kw)
        assert isinstance(fn(x, [6, 6]), ctc_amd.BeamHypotheses)


# ---------------------------------------------------------------------------------------------------------------------------
# 8. determinism and capture
# ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lattice", LATTICES)
def test_deterministic_and_capture_safe(dev, lattice):
    """two eager calls give equal bits; a call captured into a graph and replayed on new logits AND new table contents
    gives the eager call's"""
    import ctc_amd
    T, B, C = 30, 8, 20

    def data(seed):
        x, _ = lattice_input(planted(seed, T, B, C, 3.0), lattice)
        return torch.from_numpy(x), torch.from_numpy(table(seed, C))

    def call(x, lm, il):
        kw = dict(beam_width=16, nbest=4, top_classes=8, lm=lm, lm_weight=ALPHA, token_bonus=BETA[lattice])
        return ctc_amd.blank_beam_search(x, il, **kw) if lattice == "blank" else ctc_amd.noblank_beam_search(x, il, **kw)

    def same_bits(a, b, what):
        for name, u, v in zip(ctc_amd.FusedBeamHypotheses._fields, a, b):
            assert u.cpu().numpy().tobytes() == v.cpu().numpy().tobytes(), "%s: %s differs" % (what, name)

    xs, lm = (v.to(dev) for v in data(70))
    il = torch.as_tensor([30, 30, 17, 0, 1, 30, 29, 30], dtype=torch.int64).to(dev)
    first, second = call(xs, lm, il), call(xs, lm, il)
    torch.cuda.synchronize()
    same_bits(first, second, "two eager calls")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                     # warm-up on the capture stream
        for _ in range(2):
            call(xs, lm, il)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        captured = call(xs, lm, il)
    before = None
    for seed in (71, 72):
        nx, nlm = data(seed)
        xs.copy_(nx.to(dev))
        lm.copy_(nlm.to(dev))
        g.replay()
        torch.cuda.synchronize()
        got = tuple(v.clone() for v in captured)
        eager = call(xs.clone(), lm.clone(), il)
        torch.cuda.synchronize()
        same_bits(got, eager, "replay on seed %d" % seed)
        assert before is None or not torch.equal(before, got[0])                # (the replay did read the new data)
        before = got[0]
