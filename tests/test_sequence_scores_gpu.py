"""The sequence-score kernel on the MI355X: ctc_amd.blank_sequence_scores and ctc_amd.noblank_sequence_scores against the sum
over all alignments (tests/beam_ref.brute_force), against the float64 restatement of the rules
(tests/sequence_scores_ref.py), and against the rest of the engine (the losses, the beam search).

Tolerance: the project's NLL_RTOL (tests/test_parity_gpu.py) -- |score - ref| <= 1e-5 max(1, |ref|) against float64;
-inf and NaN compare exactly."""
import numpy as np
import pytest
import torch

from tests.beam_ref import brute_force
from tests.sequence_scores_ref import all_sequences, padded, sequence_scores_ref

pytestmark = pytest.mark.gpu

RTOL = 1e-5
NEG_INF = float("-inf")
LATTICES = ["blank", "noblank"]
G = 8                                                          # candidates of one workgroup (kSeqGroup)
FRAMES = {158: 32, 1000: 16}                                   # F, the frames of a tile in LDS, at these C (16384 / C, <= 32)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    import ctc_amd  # noqa: F401  (raises if libctc_amd.so is missing)
    return torch.device("cuda:0")


def log_softmax32(x):
    x64 = x.astype(np.float64)
    m = x64.max(axis=-1, keepdims=True)
    return (x64 - (m + np.log(np.exp(x64 - m).sum(axis=-1, keepdims=True)))).astype(np.float32)


def inputs(seed, T, B, C, lattice, scale=2.0):
    """[T,B,C] float32: normalised log-probabilities (blank lattice) or raw logits"""
    x = (np.random.default_rng(seed).standard_normal((T, B, C)) * scale).astype(np.float32)
    return log_softmax32(x) if lattice == "blank" else x


def to_dev(dev, a, dtype=None):
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
    return t.to(device=dev, dtype=dtype)


def run(dev, x, in_len, seqs, lens, lattice, counts=None, blank=0, seq_dtype=torch.int64):
    """the kernel -> numpy float32 [B,N]"""
    import ctc_amd
    xd = to_dev(dev, x)
    il = to_dev(dev, np.asarray(in_len), torch.int64)
    sq, sl = to_dev(dev, seqs, seq_dtype), to_dev(dev, np.asarray(lens), torch.int64)
    cn = None if counts is None else to_dev(dev, np.asarray(counts), torch.int32)
    if lattice == "blank":
        out = ctc_amd.blank_sequence_scores(xd, il, sq, sl, counts=cn, blank=blank)
    else:
        out = ctc_amd.noblank_sequence_scores(xd, il, sq, sl, counts=cn)
    torch.cuda.synchronize()
    assert out.shape == (xd.shape[1], sq.shape[-2]) and out.dtype == torch.float32 and not out.requires_grad
    return out.cpu().numpy()


def check(got, ref, what=""):
    """-inf and NaN exactly; everything else within RTOL max(1, |ref|)"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, what
    special = ~np.isfinite(ref)
    assert np.array_equal(got[special], ref[special], equal_nan=True), (what, got[special], ref[special])
    err = np.abs(got[~special] - ref[~special])
    bound = RTOL * np.maximum(1.0, np.abs(ref[~special]))
    print("%s: max error %.3g of bound %.3g over %d scores" % (
        what, err.max() if err.size else 0.0, bound[err.argmax()] if err.size else 0.0, err.size))
    assert np.all(np.isfinite(got[~special])) and np.all(err <= bound), (what, float((err / bound).max()))


def reference(x, in_len, seqs, lens, lattice, counts=None, blank=0):
    return sequence_scores_ref(x, in_len, seqs, lens, counts, blank if lattice == "blank" else -1)


def random_sequences(seed, N, L, C, lattice, blank=0, lengths=None, equal_neighbours=True):
    """[N,L] int64 padded with -1, [N] lengths; labels never the blank"""
    rng = np.random.default_rng(seed)
    classes = [c for c in range(C) if lattice != "blank" or c != blank]
    seqs = np.full((N, L), -1, np.int64)
    lens = np.asarray(lengths if lengths is not None else rng.integers(1, L + 1, N), np.int64)
    for n in range(N):
        prev = -1
        for i in range(int(lens[n])):
            c = classes[int(rng.integers(len(classes)))]
            while not equal_neighbours and c == prev:
                c = classes[int(rng.integers(len(classes)))]
            seqs[n, i] = prev = c
    return seqs, lens


# ---- 1. exhaustive: every sequence there is, against the sum over all alignments

@pytest.mark.parametrize("lattice", LATTICES)
def test_every_sequence_against_the_sum_over_all_alignments(dev, lattice):
    T, B, C, blank = 5, 3, 3, 0 if lattice == "blank" else -1
    in_len = [5, 3, 0]
    x = inputs(1, T, B, C, lattice)
    if lattice == "blank":
        seqs = all_sequences((1, 2), 5)                         # all 63 over {1, 2}, the empty one first
    else:
        seqs = all_sequences((0, 1, 2), 5, min_len=1, equal_neighbours=False) + [()]
    arr, lens = padded(seqs)
    got = run(dev, x, in_len, arr, lens, lattice)               # one shared [N,L] set
    ref = np.full((B, len(seqs)), NEG_INF)
    for b in range(B):
        bf = brute_force(x[:, b], in_len[b], blank)
        assert set(bf) <= set(seqs)
        for n, s in enumerate(seqs):
            ref[b, n] = bf.get(s, NEG_INF)
    check(got, ref, "exhaustive " + lattice)
    for b in (0, 1):
        # every score within RTOL (relative 1e-5 of its probability), the fp32 rows normalised to T C 2^-24
        total = float(np.exp(got[b].astype(np.float64)).sum())
        assert abs(total - 1.0) <= 1.2e-5, (b, total)
    empty = seqs.index(())
    assert got[2, empty] == 0.0 and np.all(np.delete(got[2], empty) == NEG_INF)     # T_b = 0
    if lattice == "noblank":
        assert np.all(got[:2, empty] == NEG_INF)                # the empty sequence at T_b >= 1


# ---- 2. states per lane and the wave edge

@pytest.mark.parametrize("lattice,L", [("blank", L) for L in (31, 32, 63, 64, 127, 128, 255)] +
                         [("noblank", L) for L in (64, 65, 128, 129, 255)])
def test_states_per_lane(dev, lattice, L):
    B, C, N, T = 2, 5, 3, 2 * L + 3
    x = inputs(L, T, B, C, lattice)
    in_len = [T, T - 2]
    seqs, lens = random_sequences(L + 1, N, L, C, lattice, lengths=[L, L, max(1, L // 2)])
    seqs[1] = random_sequences(L + 2, 1, L, C, lattice, lengths=[L], equal_neighbours=False)[0][0]
    got = run(dev, x, in_len, seqs, lens, lattice)
    ref = reference(x, in_len, seqs, lens, lattice)
    assert np.isfinite(ref).all()
    check(got, ref, "%s L=%d" % (lattice, L))


# ---- 3. frame tiles, column chunks, candidates across workgroups, the unstaged rows

@pytest.mark.parametrize("lattice", LATTICES)
@pytest.mark.parametrize("T", [1, FRAMES[158] - 1, FRAMES[158], FRAMES[158] + 1, 2 * FRAMES[158] + 1])
def test_frame_tiles_158_classes(dev, lattice, T):
    B, C, N, L = 3, 158, G + 1, 6                               # three column chunks of 64 and a tail; 9 candidates: two workgroups
    x = inputs(T, T, B, C, lattice)
    in_len = [T, max(T - 1, 1), (T + 1) // 2]
    seqs, lens = random_sequences(T, B * N, L, C, lattice)
    seqs, lens = seqs.reshape(B, N, L), lens.reshape(B, N)
    got = run(dev, x, in_len, seqs, lens, lattice)
    check(got, reference(x, in_len, seqs, lens, lattice), "%s C=158 T=%d" % (lattice, T))
    one = run(dev, x, in_len, seqs[:, :1], lens[:, :1], lattice)                    # N = 1
    assert np.array_equal(one, got[:, :1], equal_nan=True)


@pytest.mark.parametrize("lattice", LATTICES)
@pytest.mark.parametrize("C,T", [(1000, 2 * FRAMES[1000] + 1), (4096, 9), (4100, 21)])
def test_wide_rows(dev, lattice, C, T):
    # C = 1000: 16-frame tiles, 16-byte pieces; 4096: the widest staged row (4-frame tiles); 4100: rows not staged
    B, N, L = 2, 2, 7
    x = inputs(C, T, B, C, lattice)
    in_len = [T, T - 3]
    seqs, lens = random_sequences(C, N, L, C, lattice)
    got = run(dev, x, in_len, seqs, lens, lattice)
    check(got, reference(x, in_len, seqs, lens, lattice), "%s C=%d" % (lattice, C))


# ---- 4. long chains: where a rescaling can go wrong

@pytest.mark.parametrize("lattice", LATTICES)
def test_long_chains(dev, lattice):
    T, B, C, N, L = 2000, 2, 40, 4, 100
    x = inputs(4, T, B, C, lattice)
    in_len = [2000, 1777]
    seqs, lens = random_sequences(5, N, L, C, lattice, lengths=[100, 97, 64, 100], equal_neighbours=False)
    seqs[3] = random_sequences(6, 1, L, C, lattice, lengths=[100])[0][0]             # with equal neighbours
    got = run(dev, x, in_len, seqs, lens, lattice)
    ref = reference(x, in_len, seqs, lens, lattice)
    assert np.isfinite(ref).all() and np.abs(ref).min() > 1000.0
    check(got, ref, "%s T=2000" % lattice)


def peaked_clip(seed, T, B, C, transcript, rest):
    """[T,B,C] float32 logits as a trained model's: unit noise, each label of `transcript` held for 3-8 frames and raised by
    10, then class `rest` (the blank, or the transcript's last label) raised by 10 to the end of the clip"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((T, B, C))
    for b in range(B):
        t = 0
        for c in transcript:
            n = int(rng.integers(3, 9))
            x[t:t + n, b, c] += 10.0
            t += n
        x[t:, b, rest] += 10.0
    return x.astype(np.float32)


@pytest.mark.parametrize("lattice", LATTICES)
def test_long_chains_short_candidates(dev, lattice):
    """A short candidate that ends early in a long peaked clip: |score| of order 1 .. 10, so the tolerance is 1e-5 .. 1e-4
    in absolute terms, and almost every state a lane holds lies beyond the candidate's own (they must not take part: fed
    from the last state they would outgrow it by hundreds of bits and the renormalisation would follow them).  The
    no-blank candidate ends in class 0, the column those states gather."""
    T, B, C = 2000, 2, 40
    if lattice == "blank":
        x = log_softmax32(peaked_clip(70, T, B, C, (3, 7, 5), 0))
        seqs, lens = padded([(3, 7, 5), (3, 7), (7,), ()], L=3)
    else:
        x = peaked_clip(71, T, B, C, (3, 7, 0), 0)
        seqs, lens = padded([(3, 7, 0), (3, 0), (0,), (7, 0)], L=3)
    in_len = [2000, 1900]
    got = run(dev, x, in_len, seqs, lens, lattice)
    ref = reference(x, in_len, seqs, lens, lattice)
    assert np.isfinite(ref).all() and np.all(np.abs(ref[:, 0]) < 20.0)      # the planted transcript: a small |score|
    check(got, ref, "%s T=2000, short candidates" % lattice)


# ---- 5. forms: each pair agrees bit for bit

@pytest.mark.parametrize("lattice", LATTICES)
def test_forms_agree_bit_for_bit(dev, lattice):
    import ctc_amd
    T, B, C, N, L = 37, 3, 34, 5, 9
    x = inputs(8, T, B, C, lattice)
    in_len = [37, 30, 12]
    seqs, lens = random_sequences(9, N, L, C, lattice)
    lens[4] = L + 2                                             # one NaN among them
    base = run(dev, x, in_len, seqs, lens, lattice)
    check(base, reference(x, in_len, seqs, lens, lattice), "forms " + lattice)

    def same(other, what):
        assert np.array_equal(base.view(np.uint32), other.view(np.uint32)), what

    same(run(dev, x, in_len, np.broadcast_to(seqs, (B, N, L)).copy(), np.broadcast_to(lens, (B, N)).copy(), lattice),
         "[N,L] shared against [B,N,L] expanded")
    same(run(dev, x, in_len, seqs, lens, lattice, seq_dtype=torch.int32), "int32 against int64")
    xt = to_dev(dev, np.ascontiguousarray(x.transpose(1, 0, 2))).transpose(0, 1)    # a [B,T,C] tensor seen as [T,B,C]
    assert not xt.is_contiguous()
    same(run(dev, xt, in_len, seqs, lens, lattice), "a transposed view against the contiguous tensor")
    same(run(dev, x, in_len, seqs, lens, lattice), "two calls")

    fn = ctc_amd.blank_sequence_scores if lattice == "blank" else ctc_amd.noblank_sequence_scores
    args = (to_dev(dev, x), to_dev(dev, np.asarray(in_len), torch.int64), to_dev(dev, seqs), to_dev(dev, lens))
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        fn(*args)                                               # (warm-up outside the capture)
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = fn(*args)
    out.fill_(7.0)
    graph.replay()
    torch.cuda.synchronize()
    same(out.cpu().numpy(), "a graph replay against eager")


# ---- 6. special cases

def test_special_cases_blank(dev):
    T, B, C, L = 12, 3, 6, 5
    for blank in (0, 2):
        x = inputs(20 + blank, T, B, C, "blank")
        x[:, :, 5] = NEG_INF                                    # a masked class
        other = 1 if blank == 0 else 0
        seqs, lens = padded([(other, 3, 4), (3, 3, 3, 3), (4, 5, 3), (3, blank, 4), (3, C, 4), (3, -2, 4), (3, 4), (4,), (),
                             (3, 4, 3, 4, 3)], L=L)
        lens[6], lens[7] = L + 1, -1                            # longer than the tensor is wide; negative
        in_len = [12, 6, 0]                                     # 6 frames: (3,3,3,3) needs 7
        counts = [10, 9, 4]
        got = run(dev, x, in_len, seqs, lens, "blank", counts=counts, blank=blank)
        ref = reference(x, in_len, seqs, lens, "blank", counts=counts, blank=blank)
        check(got, ref, "special cases, blank %d" % blank)
        assert np.isfinite(got[0, [0, 1, 8, 9]]).all() and np.isfinite(got[1, [0, 8]]).all()
        assert got[1, 1] == NEG_INF                             # repeats needing more frames than T_b
        assert got[0, 2] == NEG_INF and got[1, 2] == NEG_INF    # through the masked class
        assert np.isnan(got[:2, 3:8]).all()                     # label = blank, >= C, < 0; len > L, len < 0
        assert got[1, 9] == NEG_INF                             # beyond the count (it would be finite)
        assert np.all(got[2, :3] == NEG_INF) and np.isnan(got[2, 3])                # T_b = 0; a bad label comes before it
        assert np.all(got[2, 4:] == NEG_INF)                    # beyond the count comes first: the NaN rows too
        nocount = run(dev, x, in_len, seqs, lens, "blank", blank=blank)
        assert nocount[2, 8] == 0.0 and np.isfinite(nocount[1, 9])


def test_special_cases_noblank(dev):
    T, B, C, L = 12, 3, 6, 5
    x = inputs(30, T, B, C, "noblank")
    seqs, lens = padded([(1, 3, 4), (3, 3, 0), (3, C, 4), (3, -1, 4), (3, 4), (4,), (), (0, 1, 2, 3, 4)], L=L)
    lens[4], lens[5] = L + 1, -1
    in_len = [12, 4, 0]
    counts = [8, 7, 2]
    got = run(dev, x, in_len, seqs, lens, "noblank", counts=counts)
    ref = reference(x, in_len, seqs, lens, "noblank", counts=counts)
    check(got, ref, "special cases, no blank")
    assert np.isfinite(got[0, [0, 1, 7]]).all()
    assert np.isnan(got[:2, 2:6]).all()                         # a label >= C, < 0; len > L, len < 0
    assert got[0, 6] == NEG_INF and got[1, 6] == NEG_INF        # the empty sequence at T_b >= 1
    assert got[1, 7] == NEG_INF                                 # beyond the count; (and 5 labels in 4 frames)
    assert np.all(got[2] == NEG_INF)
    nocount = run(dev, x, in_len, seqs, lens, "noblank")
    assert nocount[2, 6] == 0.0 and nocount[1, 7] == NEG_INF and np.isnan(nocount[2, 2])


# ---- 7. against the rest of the engine

@pytest.mark.parametrize("lattice", LATTICES)
def test_against_the_losses(dev, lattice):
    import ctc_amd
    T, B, C, N, L = 37, 3, 34, 4, 12
    x = inputs(40, T, B, C, lattice)
    in_len = [37, 20, 9]                                        # 9 frames: some candidates have no alignment
    seqs, lens = random_sequences(41, B * N, L, C, lattice)
    seqs, lens = seqs.reshape(B, N, L), lens.reshape(B, N)
    got = run(dev, x, in_len, seqs, lens, lattice)
    xd, il = to_dev(dev, x), to_dev(dev, np.asarray(in_len), torch.int64)
    finite = 0
    for n in range(N):
        tg, tl = to_dev(dev, np.maximum(seqs[:, n], 0)), to_dev(dev, lens[:, n])
        with torch.no_grad():
            if lattice == "blank":
                nll = ctc_amd.blank_ctc_loss(xd, tg, il, tl)[1]
            else:
                nll = ctc_amd.noblank_ctc_loss(xd, tg, il, tl)[1]
        nll = nll.cpu().numpy().astype(np.float64)
        for b in range(B):
            if np.isfinite(nll[b]) and nll[b] < 1e12:
                finite += 1
                assert abs(got[b, n] + nll[b]) <= RTOL * max(1.0, abs(nll[b])), (b, n, got[b, n], nll[b])
            else:
                assert got[b, n] == NEG_INF, (b, n, got[b, n], nll[b])
    assert finite >= 8
    check(got, reference(x, in_len, seqs, lens, lattice), "losses' shape " + lattice)


def _search(dev, x, in_len, lattice, W, N, L):
    import ctc_amd
    xd, il = to_dev(dev, x), to_dev(dev, np.asarray(in_len), torch.int64)
    if lattice == "blank":
        return xd, il, ctc_amd.blank_beam_search(xd, il, beam_width=W, nbest=N, top_classes=16, max_tokens=L)
    return xd, il, ctc_amd.noblank_beam_search(xd, il, beam_width=W, nbest=N, top_classes=16, max_tokens=L)


@pytest.mark.parametrize("lattice", LATTICES)
def test_scoring_beam_hypotheses_as_they_are(dev, lattice):
    import ctc_amd
    fn = ctc_amd.blank_sequence_scores if lattice == "blank" else ctc_amd.noblank_sequence_scores
    T, B, C, W, N = 30, 4, 12, 8, 4
    x = inputs(50, T, B, C, lattice)
    in_len = [30, 17, 1, 0]                                     # one frame: fewer hypotheses than nbest on the blank lattice
    xd, il, hyp = _search(dev, x, in_len, lattice, W, N, None)
    exact = fn(xd, il, hyp.tokens, hyp.lengths, counts=hyp.count)
    torch.cuda.synchronize()
    exact, found, count = exact.cpu().numpy().astype(np.float64), hyp.scores.cpu().numpy().astype(np.float64), hyp.count.cpu().numpy()
    for b in range(B):
        for n in range(N):
            if n >= count[b]:
                assert exact[b, n] == NEG_INF                   # rows beyond `count`
            else:                                               # a search can only lose alignments
                assert np.isfinite(exact[b, n]) and exact[b, n] >= found[b, n] - RTOL * max(1.0, abs(found[b, n]))
    assert count[3] == 1 and exact[3, 0] == 0.0                 # T_b = 0: the one empty hypothesis
    ref = reference(x, in_len, hyp.tokens.cpu().numpy(), hyp.lengths.cpu().numpy(), lattice, counts=count)
    check(exact, ref, "beam hypotheses " + lattice)
    # truncated hypotheses are "not scored": two token columns are fewer than the best hypotheses have tokens
    xd, il, short = _search(dev, x, in_len, lattice, W, N, 2)
    cut = fn(xd, il, short.tokens, short.lengths, counts=short.count).cpu().numpy()
    lengths = short.lengths.cpu().numpy()
    assert (lengths[0, :count[0]] > 2).any()
    for b in range(B):
        for n in range(N):
            if n < count[b]:
                assert np.isnan(cut[b, n]) == (lengths[b, n] > 2)


@pytest.mark.parametrize("lattice", LATTICES)
def test_a_beam_that_holds_every_prefix_is_exact(dev, lattice):
    import ctc_amd
    fn = ctc_amd.blank_sequence_scores if lattice == "blank" else ctc_amd.noblank_sequence_scores
    T, B, C, W = 4, 3, 3, 64
    x = inputs(60, T, B, C, lattice)
    in_len = [4, 3, 2]
    xd, il, hyp = _search(dev, x, in_len, lattice, W, W, None)
    exact = fn(xd, il, hyp.tokens, hyp.lengths, counts=hyp.count).cpu().numpy().astype(np.float64)
    found, count = hyp.scores.cpu().numpy().astype(np.float64), hyp.count.cpu().numpy()
    for b in range(B):
        assert count[b] >= 3
        for n in range(W):
            if n < count[b]:
                assert abs(exact[b, n] - found[b, n]) <= RTOL * max(1.0, abs(found[b, n])), (b, n)
            else:
                assert exact[b, n] == NEG_INF
