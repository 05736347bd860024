"""The beam search kernel on the MI355X: ctc_amd.blank_beam_search and ctc_amd.noblank_beam_search against the sum over all
alignments where the search is exact, against the float64 restatement of the rules (tests/beam_ref.py) elsewhere, and
against the exact probability of every hypothesis they return (a search can only lose alignments, never invent any).

No check depends on how a near-tie falls: a sample is compared with the restatement only where the restatement's own best
five scores lie more than GAP apart (fp32 against float64 arithmetic may order closer ones differently, and both are
right); at most a quarter of a case's samples may be left out that way."""
import functools

import numpy as np
import pytest
import torch

from tests.beam_ref import beam_search_ref, brute_force

pytestmark = pytest.mark.gpu

RTOL = 1e-5                                                    # the project's NLL_RTOL: |score - ref| <= RTOL max(1, |ref|)
GAP = 1e-3                                                     # a sample counts when its reference scores are this far apart
NEG_INF = float("-inf")
LATTICES = ["blank", "noblank"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    import ctc_amd  # noqa: F401  (raises if libctc_amd.so is missing)
    return torch.device("cuda:0")


def tol(s):
    return RTOL * max(1.0, abs(s))


def log_softmax32(x):
    x64 = x.astype(np.float64)
    m = x64.max(axis=-1, keepdims=True)
    m = np.where(np.isfinite(m), m, 0.0)
    return (x64 - (m + np.log(np.exp(x64 - m).sum(axis=-1, keepdims=True)))).astype(np.float32)


def planted(seed, T, B, C, lift, scale=1.0):
    """unit noise with a planted transcript: runs of 3-9 frames of one class (no two neighbours equal) raised by `lift`"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((T, B, C)) * scale
    for b in range(B):
        t, prev = 0, -1
        while t < T:
            n = int(rng.integers(3, 10))
            c = int(rng.integers(C))
            while c == prev:
                c = int(rng.integers(C))
            x[t:t + n, b, c] += lift
            t, prev = t + n, c
    return x.astype(np.float32)


def lattice_input(x, lattice, blank=0):
    """(what the function is given, the `blank` of the C ABI): normalised log-probabilities, or the raw logits"""
    return (log_softmax32(x), blank) if lattice == "blank" else (x, -1)


def search(dev, x, in_len, blank, W, K, N, L=None):
    """the kernel -> numpy (tokens, lengths, scores, count)"""
    import ctc_amd
    xd = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    il = torch.as_tensor(np.asarray(in_len), dtype=torch.int64).to(dev)
    if blank >= 0:
        h = ctc_amd.blank_beam_search(xd, il, beam_width=W, nbest=N, top_classes=K, blank=blank, max_tokens=L)
    else:
        h = ctc_amd.noblank_beam_search(xd, il, beam_width=W, nbest=N, top_classes=K, max_tokens=L)
    torch.cuda.synchronize()
    T, B = xd.shape[0], xd.shape[1]
    assert h.tokens.shape == (B, N, T if L is None else L) and h.tokens.dtype == torch.int32
    assert h.lengths.shape == (B, N) and h.lengths.dtype == torch.int64
    assert h.scores.shape == (B, N) and h.scores.dtype == torch.float32
    assert h.count.shape == (B,) and h.count.dtype == torch.int32
    return tuple(v.cpu().numpy() for v in h)


def counted_samples(ref_scores, ref_count):
    """samples whose reference scores (the best five, or all there are) lie more than GAP apart"""
    keep = []
    for b in range(ref_scores.shape[0]):
        s = ref_scores[b, :min(int(ref_count[b]), 5)]
        keep.append(bool(np.all(s[:-1] - s[1:] > GAP)))
    return np.array(keep)


def check_against_reference(got, x, in_len, blank, W, K, N, L=None, what=""):
    """the rule of this file: got = (tokens, lengths, scores, count) of N hypotheses against the float64 restatement, on the
    samples that count.  -> the largest score error over tol (printed by the callers' -s runs)"""
    T = x.shape[0]
    L = T if L is None else L
    n5 = min(5, W)
    rt, rl, rs, rc = beam_search_ref(x, in_len, W, K, n5, L, blank, np.float64)
    keep = counted_samples(rs, rc)
    assert (~keep).sum() * 4 <= len(keep), "%s: %d of %d samples are near-ties" % (what, (~keep).sum(), len(keep))
    tokens, lengths, scores, count = got
    worst = 0.0
    for b in np.nonzero(keep)[0]:
        n = min(int(rc[b]), N)
        assert count[b] == n, (what, b, count[b], n)
        assert lengths[b, :n].tolist() == rl[b, :n].tolist(), (what, b)
        assert tokens[b, :n].tolist() == rt[b, :n].tolist(), (what, b)
        for k in range(n):
            err = abs(float(scores[b, k]) - rs[b, k])
            worst = max(worst, err / tol(rs[b, k]))
            assert err <= tol(rs[b, k]), (what, b, k, float(scores[b, k]), rs[b, k])
    check_padding(got, L)
    print("%s: %d of %d samples counted, worst score error %.3g of the tolerance" % (what, keep.sum(), len(keep), worst))
    return worst


def check_padding(got, L):
    """every element is written: rows at and beyond count hold -1 / 0 / -inf, columns behind a sequence's end -1, scores
    do not rise"""
    tokens, lengths, scores, count = got
    B, N = lengths.shape
    for b in range(B):
        n = int(count[b])
        assert 0 <= n <= N
        assert (tokens[b, n:] == -1).all() and (lengths[b, n:] == 0).all() and (scores[b, n:] == NEG_INF).all()
        for k in range(n):
            ln = min(int(lengths[b, k]), L)
            assert (tokens[b, k, :ln] >= 0).all() and (tokens[b, k, ln:] == -1).all()
        assert np.all(scores[b, 1:n] <= scores[b, :n - 1]) and np.all(np.isfinite(scores[b, :n]))


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the exact regime: every prefix fits in the beam
# ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lattice", LATTICES)
def test_exact_regime(dev, lattice):
    """C = 3, T_b <= 5 (blank) / 4 (no-blank), W = 64: the hypotheses are the labellings of non-zero probability, the
    scores their log-probabilities from the sum over all C^T alignments"""
    T, B, C = (5, 16, 3) if lattice == "blank" else (4, 16, 3)
    rng = np.random.default_rng(11)
    x, blank = lattice_input((rng.standard_normal((T, B, C)) * 2.0).astype(np.float32), lattice, blank=0)
    in_len = np.array([0, 1] + [int(v) for v in rng.integers(0, T + 1, B - 4)] + [T, T])
    got = search(dev, x, in_len, blank, 64, 32, 64)
    tokens, lengths, scores, count = got
    worst = 0.0
    for b in range(B):
        want = brute_force(x[:, b], int(in_len[b]), blank)
        n = int(count[b])
        assert n == len(want), (b, n, len(want))
        hyps = [tuple(tokens[b, k, :lengths[b, k]].tolist()) for k in range(n)]
        assert set(hyps) == set(want) and len(set(hyps)) == n, b
        exact = [want[h] for h in hyps]
        for k in range(n):
            worst = max(worst, abs(float(scores[b, k]) - exact[k]) / tol(exact[k]))
            assert abs(float(scores[b, k]) - exact[k]) <= tol(exact[k]), (b, hyps[k], float(scores[b, k]), exact[k])
        # best first: the exact probabilities of neighbours never contradict the order by more than the tolerance
        for k in range(n - 1):
            assert exact[k] >= exact[k + 1] - 2 * tol(exact[k + 1]), (b, hyps[k], hyps[k + 1])
    assert count[0] == 1 and lengths[0, 0] == 0 and scores[0, 0] == 0.0          # T_b = 0: the empty hypothesis
    check_padding(got, T)
    print("exact regime, %s: worst score error %.3g of the tolerance" % (lattice, worst))


# ---------------------------------------------------------------------------------------------------------------------------
# 2. against the float64 restatement; 3. soundness; 6. composition with blank_token_spans
# ---------------------------------------------------------------------------------------------------------------------------

# name -> (T, C, W, K, B), how the inputs are made, the seed (kept: the restatement alone leaves out <= 1/8 of the samples)
CASES = {"A": ((40, 12, 8, 4, 32), ("planted", 3.0), 1),
         "B": ((300, 50, 16, 8, 8), ("planted", 6.0), 2),
         "C": ((30, 40, 64, 32, 8), ("random", 3.0), 5)}


@functools.lru_cache(maxsize=None)
def case_inputs(name, lattice):
    (T, C, W, K, B), (kind, amount), seed = CASES[name]
    if kind == "planted":
        raw = planted(seed, T, B, C, amount)
    else:
        raw = (np.random.default_rng(seed).standard_normal((T, B, C)) * amount).astype(np.float32)
    x, blank = lattice_input(raw, lattice)
    in_len = np.full(B, T)
    if name == "A":
        in_len = np.random.default_rng(seed + 100).integers(T // 2, T + 1, B)
    return x, in_len, blank


@functools.lru_cache(maxsize=None)
def case_result(name, lattice):
    """the kernel's four hypotheses of a case (one launch per case and lattice, shared by the tests below)"""
    x, in_len, blank = case_inputs(name, lattice)
    (T, C, W, K, B) = CASES[name][0]
    return search(torch.device("cuda:0"), x, in_len, blank, W, K, 4)


@pytest.mark.parametrize("lattice", LATTICES)
@pytest.mark.parametrize("name", sorted(CASES))
def test_against_float64_restatement(dev, name, lattice):
    x, in_len, blank = case_inputs(name, lattice)
    (T, C, W, K, B) = CASES[name][0]
    check_against_reference(case_result(name, lattice), x, in_len, blank, W, K, 4, what="case %s, %s" % (name, lattice))


def exact_log_prob(x, in_len, blank, tokens, lengths):
    """float64 log P(tokens[b] | x[:, b]) for every sample"""
    if blank >= 0:
        lp = torch.from_numpy(x).double()
        tg = torch.from_numpy(np.where(tokens >= 0, tokens, 0)).long()
        nll = torch.nn.functional.ctc_loss(lp, tg, torch.as_tensor(in_len, dtype=torch.long),
                                           torch.as_tensor(lengths, dtype=torch.long), blank=blank, reduction="none")
        return (-nll).numpy()
    from oracle.ctc_numpy import noblank_ctc
    return -noblank_ctc(x, tokens, in_len, lengths, np.float64, want_grad=False)["nll"]


@pytest.mark.parametrize("lattice", LATTICES)
def test_scores_never_exceed_the_exact_probability(dev, lattice):
    """case A, every returned hypothesis: the search sums a subset of the hypothesis's alignments"""
    x, in_len, blank = case_inputs("A", lattice)
    tokens, lengths, scores, count = case_result("A", lattice)
    assert (count == 4).all()
    for k in range(4):
        exact = exact_log_prob(x, in_len, blank, tokens[:, k], lengths[:, k])
        for b in range(len(in_len)):
            assert float(scores[b, k]) <= exact[b] + tol(exact[b]), (b, k, float(scores[b, k]), exact[b])


def test_composes_with_blank_token_spans(dev):
    """the best hypothesis of case A goes straight into blank_token_spans (tokens padded with -1, int64 lengths): its nll
    is the exact probability of that hypothesis, computed on the device"""
    import ctc_amd
    x, in_len, blank = case_inputs("A", "blank")
    lp = torch.from_numpy(x).to(dev)
    il = torch.as_tensor(in_len, dtype=torch.int64).to(dev)
    hyp = ctc_amd.blank_beam_search(lp, il, beam_width=8, nbest=4, top_classes=4)
    spans = ctc_amd.blank_token_spans(lp, hyp.tokens[:, 0, :], il, hyp.lengths[:, 0])
    torch.cuda.synchronize()
    nll, score = spans.nll.cpu().numpy(), hyp.scores[:, 0].cpu().numpy()
    for b in range(len(in_len)):
        assert -float(nll[b]) >= float(score[b]) - tol(float(nll[b])), (b, float(nll[b]), float(score[b]))


# ---------------------------------------------------------------------------------------------------------------------------
# 4. edges
# ---------------------------------------------------------------------------------------------------------------------------

# name -> (T, B, C, W, K, N, lift): planted inputs; the seed is 40 + the name's position, or the one of EDGE_SEEDS (kept, as
# for the cases: the restatement alone leaves out <= 1/8 of the samples)
EDGES = {"W=1": (20, 8, 10, 1, 4, 1, 3.0),
         "W=64,K=32": (12, 8, 40, 64, 32, 4, 3.0),
         "W=16,K=31": (12, 8, 40, 16, 31, 4, 3.0),               # 512 candidates: two keys per lane in the selection
         "W=16,K=32": (12, 8, 40, 16, 32, 4, 3.0),               # 528: three
         "K=1": (20, 8, 10, 8, 1, 4, 3.0),
         "K>C-1": (20, 8, 5, 8, 16, 4, 3.0),
         "C=2": (16, 8, 2, 8, 4, 4, 3.0),
         "C=67": (20, 8, 67, 8, 8, 4, 4.0),
         "C=1024": (8, 4, 1024, 8, 8, 4, 8.0),
         "C=1025": (8, 4, 1025, 8, 8, 4, 8.0),
         "C=1500": (8, 4, 1500, 8, 8, 4, 8.0),
         "T=1": (1, 8, 10, 8, 4, 4, 3.0),
         "B=300,T=6": (6, 300, 8, 4, 4, 4, 3.0)}


EDGE_SEEDS = {"W=64,K=32": 80, "C=1024": 80}


def edge_inputs(name):
    T, B, C, W, K, N, lift = EDGES[name]
    raw = planted(EDGE_SEEDS.get(name, 40 + sorted(EDGES).index(name)), T, B, C, lift)
    if T == 1:
        raw = raw * 3.0                                          # (one frame: spread the scores of its classes)
    return raw, np.full(B, T), W, K, N


@pytest.mark.parametrize("lattice", LATTICES)
@pytest.mark.parametrize("name", sorted(EDGES))
def test_edge_shapes(dev, name, lattice):
    raw, in_len, W, K, N = edge_inputs(name)
    x, blank = lattice_input(raw, lattice)
    got = search(dev, x, in_len, blank, W, K, N)
    check_against_reference(got, x, in_len, blank, W, K, N, what="%s, %s" % (name, lattice))


def test_edge_blank_is_another_class(dev):
    raw = planted(60, 24, 8, 9, 3.0)
    x, blank = lattice_input(raw, "blank", blank=3)
    in_len = np.array([24, 20, 24, 1, 0, 13, 24, 24])
    got = search(dev, x, in_len, blank, 8, 4, 4)
    check_against_reference(got, x, in_len, blank, 8, 4, 4, what="blank=3")
    assert not (got[0] == 3).any()                                              # the blank is never a token


@pytest.mark.parametrize("lattice", LATTICES)
def test_edge_masked_class_column(dev, lattice):
    """a class of probability 0 everywhere (a -inf column): never a candidate, never a token"""
    raw = planted(61, 24, 8, 9, 3.0)
    raw[:, :, 5] = NEG_INF
    x, blank = lattice_input(raw, lattice)
    in_len = np.full(8, 24)
    got = search(dev, x, in_len, blank, 8, 8, 4)
    check_against_reference(got, x, in_len, blank, 8, 8, 4, what="-inf column, %s" % lattice)
    assert not (got[0] == 5).any()


def test_edge_blank_dominates(dev):
    """rows where the blank dominates: the best hypothesis is the empty one, length 0, tokens all -1"""
    rng = np.random.default_rng(62)
    raw = rng.standard_normal((16, 8, 7)).astype(np.float32)
    raw[:, :, 0] += 8.0
    x, blank = lattice_input(raw, "blank")
    in_len = np.full(8, 16)
    got = search(dev, x, in_len, blank, 8, 4, 4)
    check_against_reference(got, x, in_len, blank, 8, 4, 4, what="blank dominates")
    assert (got[1][:, 0] == 0).all() and (got[0][:, 0] == -1).all()


@pytest.mark.parametrize("lattice", LATTICES)
def test_edge_truncated_tokens(dev, lattice):
    """max_tokens = 3 under longer results: lengths are the true counts, tokens the first three"""
    raw = planted(63, 40, 8, 10, 4.0)
    x, blank = lattice_input(raw, lattice)
    in_len = np.full(8, 40)
    got = search(dev, x, in_len, blank, 8, 4, 4, L=3)
    check_against_reference(got, x, in_len, blank, 8, 4, 4, L=3, what="max_tokens=3, %s" % lattice)
    assert (got[1][:, 0] > 3).all()
    full = search(dev, x, in_len, blank, 8, 4, 4)
    assert (full[0][:, :, :3] == got[0]).all() and (full[1] == got[1]).all() and (full[2] == got[2]).all()


@pytest.mark.parametrize("lattice", LATTICES)
def test_edge_view_of_a_wider_batch(dev, lattice):
    """a [T, B + 5, C] buffer viewed as [:, :B]: read through its strides, no copy, nothing of the other samples"""
    B = 6
    raw = planted(66, 20, B + 5, 10, 3.0)
    x, blank = lattice_input(raw, lattice)
    in_len = np.array([20, 7, 20, 0, 1, 20])
    wide = torch.from_numpy(x).to(dev)
    got = search(dev, wide[:, :B], in_len, blank, 8, 4, 4)
    check_against_reference(got, x[:, :B], in_len, blank, 8, 4, 4, what="view, %s" % lattice)
    alone = search(dev, wide[:, :B].contiguous(), in_len, blank, 8, 4, 4)
    assert all((a == g).all() for a, g in zip(alone, got))
    # another class stride: made contiguous by the Python layer
    swapped = wide[:, :B].permute(0, 2, 1).contiguous().permute(0, 2, 1)
    assert swapped.stride(2) != 1
    assert all((a == g).all() for a, g in zip(search(dev, swapped, in_len, blank, 8, 4, 4), got))


# ---------------------------------------------------------------------------------------------------------------------------
# 5. determinism and capture
# ---------------------------------------------------------------------------------------------------------------------------

def _assert_same_bits(a, b, what):
    for name, u, v in zip(("tokens", "lengths", "scores", "count"), a, b):
        u, v = u.cpu().numpy(), v.cpu().numpy()
        assert u.tobytes() == v.tobytes(), "%s: %s differs" % (what, name)


@pytest.mark.parametrize("lattice", LATTICES)
def test_deterministic_and_capture_safe(dev, lattice):
    """two eager calls give equal bits; a call captured into a graph and replayed on new data gives the eager call's"""
    import ctc_amd
    T, B, C = 30, 8, 20

    def data(seed):
        x, _ = lattice_input(planted(seed, T, B, C, 3.0), lattice)
        return torch.from_numpy(x)

    def call(x, il):
        if lattice == "blank":
            return ctc_amd.blank_beam_search(x, il, beam_width=16, nbest=4, top_classes=8)
        return ctc_amd.noblank_beam_search(x, il, beam_width=16, nbest=4, top_classes=8)

    xs = data(70).to(dev)
    il = torch.as_tensor([30, 30, 17, 0, 1, 30, 29, 30], dtype=torch.int64).to(dev)
    first, second = call(xs, il), call(xs, il)
    torch.cuda.synchronize()
    _assert_same_bits(first, second, "two eager calls")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                     # warm-up on the capture stream
        for _ in range(2):
            call(xs, il)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        captured = call(xs, il)
    for seed in (71, 72):
        xs.copy_(data(seed).to(dev))
        g.replay()
        torch.cuda.synchronize()
        got = tuple(v.clone() for v in captured)
        eager = call(xs.clone(), il)
        torch.cuda.synchronize()
        _assert_same_bits(got, eager, "replay on seed %d" % seed)


def test_exact_ties_follow_the_total_order(dev):
    """constant logits: every labelling of a length has bitwise the same score in fp32 as in float64, so the order is the
    tie rule's alone -- stay before extension, then beam slot, then class rank (lower class first on equal inputs)"""
    x = np.zeros((2, 3, 2), np.float32)
    tokens, lengths, scores, count = search(dev, x, np.array([2, 1, 2]), -1, 8, 2, 4)
    assert count.tolist() == [4, 2, 4]
    assert [tokens[0, k, :lengths[0, k]].tolist() for k in range(4)] == [[0], [1], [0, 1], [1, 0]]
    assert [tokens[1, k, :lengths[1, k]].tolist() for k in range(2)] == [[0], [1]]
    assert np.allclose(scores[0], np.log(0.25), atol=1e-6) and (scores[0] == scores[0, 0]).all()
    # a beam of 3 cuts the fourth, not another one; 40 equal classes: ties among the class candidates and among 528 candidates
    tokens, lengths, _, count = search(dev, x, np.array([2, 2, 2]), -1, 3, 2, 3)
    assert [tokens[2, k, :lengths[2, k]].tolist() for k in range(3)] == [[0], [1], [0, 1]]
    x = np.zeros((2, 2, 40), np.float32)
    want = beam_search_ref(x, [2, 2], 16, 32, 16, 2, -1, np.float64)
    got = search(dev, x, np.array([2, 2]), -1, 16, 32, 16)
    assert (got[0] == want[0]).all() and (got[1] == want[1]).all() and (got[3] == want[3]).all()
    lp = log_softmax32(x)
    want = beam_search_ref(lp, [2, 2], 16, 8, 16, 2, 0, np.float64)
    got = search(dev, lp, np.array([2, 2]), 0, 16, 8, 16)
    assert (got[0] == want[0]).all() and (got[1] == want[1]).all() and (got[3] == want[3]).all()
