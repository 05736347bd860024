"""The gradient of the sequence scores on the MI355X: ctc_amd_sequence_scores_grad (through ctc_amd.functional's raw call)
and the autograd of ctc_amd.blank_sequence_scores / ctc_amd.noblank_sequence_scores, against the float64 alpha / beta
restatement (tests/sequence_scores_grad_ref.py).

Tolerance, on the occupancy scale (what an error of a state posterior becomes): |grad - ref| <= A sum_n |w[b, n]| per sample,
A = GAMMA_ATOL = 2e-4 (tests/lattice_inputs_ref.py) for T <= 300 and 5e-4 at T = 2000 (the blank posteriors' documented
bound); exact zeros and the scores compare exactly.  Every check prints its largest error as a fraction of the bound."""
import numpy as np
import pytest
import torch

from tests.lattice_inputs_ref import GAMMA_ATOL
from tests.sequence_scores_ref import all_sequences, padded
from tests.sequence_scores_grad_ref import sequence_scores_grad_ref
from tests.test_sequence_scores_gpu import inputs, log_softmax32, peaked_clip, random_sequences, to_dev

pytestmark = pytest.mark.gpu

LONG_ATOL = 5e-4
LATTICES = ["blank", "noblank"]
# F, the frames of a tile: of the forward kernel that stores the rows (unchanged by the gradient: its tile of the gradient
# is not in that kernel's LDS) and, the same numbers, the frames of a fold workgroup (4 waves x min(8, 4096 / C) rows)
FRAMES = {158: 32, 1000: 16}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    import ctc_amd  # noqa: F401  (raises if libctc_amd.so is missing)
    return torch.device("cuda:0")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def raw(dev, x, in_len, seqs, lens, w, lattice, counts=None, blank=0, seq_dtype=torch.int64, out=None):
    """the raw entry on a gradient tensor filled with NaN -> (grad [T,B,C], scores [B,N]) numpy float32"""
    from ctc_amd import functional as F
    xd = x if isinstance(x, torch.Tensor) else to_dev(dev, x)
    il = to_dev(dev, np.asarray(in_len), torch.int64)
    sq, sl = to_dev(dev, seqs, seq_dtype), to_dev(dev, np.asarray(lens), torch.int64)
    cn = None if counts is None else to_dev(dev, np.asarray(counts), torch.int32)
    xs, call = F._sequence_scores_call(xd, "x", il, sq, sl, cn, blank if lattice == "blank" else None)
    wd = to_dev(dev, np.asarray(w, np.float32))
    if out is None:
        out = torch.empty(tuple(xd.shape), dtype=torch.float32, device=dev)
    out.fill_(float("nan"))
    grad, scores = F._sequence_scores_grad(xs, call, wd, out=out, want_scores=True)
    torch.cuda.synchronize()
    return grad.cpu().numpy(), scores.cpu().numpy()


def forward(dev, x, in_len, seqs, lens, lattice, counts=None, blank=0):
    import ctc_amd
    xd = x if isinstance(x, torch.Tensor) else to_dev(dev, x)
    il = to_dev(dev, np.asarray(in_len), torch.int64)
    sq, sl = to_dev(dev, seqs, torch.int64), to_dev(dev, np.asarray(lens), torch.int64)
    cn = None if counts is None else to_dev(dev, np.asarray(counts), torch.int32)
    if lattice == "blank":
        return ctc_amd.blank_sequence_scores(xd, il, sq, sl, counts=cn, blank=blank).cpu().numpy()
    return ctc_amd.noblank_sequence_scores(xd, il, sq, sl, counts=cn).cpu().numpy()


def reference(x, in_len, seqs, lens, w, lattice, counts=None, blank=0):
    return sequence_scores_grad_ref(x, in_len, seqs, lens, w, counts, blank if lattice == "blank" else -1)


def check(grad, ref_scores, ref_grad, w, what, atol=GAMMA_ATOL):
    """|grad - ref| <= atol sum_n |w[b, n]| over the candidates scored finite; exact zeros where the reference has them in
    whole rows (t >= T_b, samples without a gradient); no NaN anywhere"""
    assert not np.isnan(grad).any(), what
    live = np.isfinite(ref_scores)
    bound = atol * np.where(live, np.abs(np.where(live, w, 0.0)), 0.0).sum(axis=1)       # [B]
    err = np.abs(grad.astype(np.float64) - ref_grad).max(axis=(0, 2))                    # [B]
    zero_rows = ~ref_grad.any(axis=2)                                                    # [T,B]
    assert not grad[zero_rows].any(), what
    with np.errstate(divide="ignore", invalid="ignore"):
        frac = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    print("%s: max error %.3g, %.3f of the bound" % (what, err.max(), frac.max()))
    assert np.all(frac <= 1.0), (what, frac)


def check_scores(scores, ref_scores, what):
    special = ~np.isfinite(ref_scores)
    assert np.array_equal(scores[special].astype(np.float64), ref_scores[special], equal_nan=True), what
    assert np.all(np.abs(scores[~special] - ref_scores[~special]) <= 1e-5 * np.maximum(1.0, np.abs(ref_scores[~special]))), what


def weights(seed, B, N):
    return np.random.default_rng(seed).standard_normal((B, N)).astype(np.float32)


# ---- 1. exhaustive

@pytest.mark.parametrize("lattice", LATTICES)
def test_every_short_sequence(dev, lattice):
    T, B, C = 5, 3, 3
    x = inputs(1, T, B, C, lattice)
    seqs = all_sequences((1, 2) if lattice == "blank" else (0, 1, 2), 3)
    arr, lens = padded(seqs)
    for in_len in ([5, 3, 0], [4, 1, 5]):
        w = weights(2, B, len(seqs))
        grad, scores = raw(dev, x, in_len, arr, lens, w, lattice)
        rs, rg = reference(x, in_len, arr, lens, w, lattice)
        check_scores(scores, rs, "exhaustive")
        check(grad, rs, rg, w, "exhaustive %s %s" % (lattice, in_len))
        assert np.array_equal(bits(scores), bits(forward(dev, x, in_len, arr, lens, lattice)))


# ---- 2. 1, 2, 4 and 8 states per lane side by side

@pytest.mark.parametrize("lattice", LATTICES)
def test_states_per_lane(dev, lattice):
    T, B, C, N = 264, 2, 40, 4
    x = inputs(3, T, B, C, lattice)
    lengths = [3, 40, 100, 255]
    seqs, lens = random_sequences(4, N, 255, C, lattice, lengths=lengths, equal_neighbours=False)
    in_len = [264, 261]
    w = weights(5, B, N)
    grad, scores = raw(dev, x, in_len, seqs, lens, w, lattice)
    rs, rg = reference(x, in_len, seqs, lens, w, lattice)
    assert np.isfinite(rs).all()
    check_scores(scores, rs, "states per lane")
    check(grad, rs, rg, w, "states per lane " + lattice)
    assert np.array_equal(bits(scores), bits(forward(dev, x, in_len, seqs, lens, lattice)))      # (9: the scores output)


# ---- 3. tile edges, both staging paths

@pytest.mark.parametrize("lattice", LATTICES)
@pytest.mark.parametrize("C", [158, 1000])
def test_tile_edges(dev, lattice, C):
    F = FRAMES[C]
    B, N, L = 2, 3, 6
    Tmax = 2 * F + 1
    seqs, lens = random_sequences(6, N, L, C, lattice)
    w = weights(7, B, N)
    x = inputs(8, Tmax, B, C, lattice)
    for T in (F - 1, F, F + 1, 2 * F - 1, 2 * F, 2 * F + 1):
        xt = np.ascontiguousarray(x[:T])
        in_len = [T, max(1, T - 3)]
        grad, scores = raw(dev, xt, in_len, seqs, lens, w, lattice)
        rs, rg = reference(xt, in_len, seqs, lens, w, lattice)
        check(grad, rs, rg, w, "tile edges %s C=%d T=%d" % (lattice, C, T))
    # C % 4 != 0 (C = 158 is; 157 here) and a strided view: the 4-byte staging path; the gradient with strides of its own
    T = 2 * F + 1
    wide = to_dev(dev, np.zeros((T, B, C + 3), np.float32))
    xv = wide[:, :, 1:C]                                        # C - 1 classes, rows 4 bytes off a 16-byte boundary
    Cv = C - 1
    xs = inputs(9, T, B, Cv, lattice)
    xv.copy_(to_dev(dev, xs))
    assert not xv.is_contiguous()
    sv, lv = random_sequences(10, N, L, Cv, lattice)
    in_len = [T, T - 5]
    out = torch.empty((B, T, Cv + 2), dtype=torch.float32, device=dev).transpose(0, 1)[:, :, :Cv]
    grad, scores = raw(dev, xv, in_len, sv, lv, w, lattice, out=out)
    rs, rg = reference(xs, in_len, sv, lv, w, lattice)
    check(grad, rs, rg, w, "strided %s C=%d" % (lattice, Cv))
    base, _ = raw(dev, xs, in_len, sv, lv, w, lattice)
    assert np.array_equal(bits(grad), bits(base))               # the views give the contiguous tensors' bits


# ---- 4. candidate groups

@pytest.mark.parametrize("lattice", LATTICES)
def test_candidate_groups(dev, lattice):
    T, B, C, L = 20, 3, 12, 6
    x = inputs(11, T, B, C, lattice)
    in_len = [20, 17, 9]
    seqs, lens = random_sequences(12, 17, L, C, lattice)
    w = weights(13, B, 17)
    for N in (1, 8, 9, 17):
        grad, scores = raw(dev, x, in_len, seqs[:N], lens[:N], w[:, :N], lattice)
        rs, rg = reference(x, in_len, seqs[:N], lens[:N], w[:, :N], lattice)
        check(grad, rs, rg, w[:, :N], "groups %s N=%d" % (lattice, N))
        if N == 9:
            nine = grad
        if N == 17:
            full, full_scores = grad, scores
    w0 = w.copy()
    w0[:, 9:] = 0.0
    part, _ = raw(dev, x, in_len, seqs, lens, w0, lattice)
    assert np.array_equal(bits(part), bits(nine))               # the order of the sum does not depend on who follows
    exp_seqs = np.broadcast_to(seqs, (B,) + seqs.shape).copy()
    exp_lens = np.broadcast_to(lens, (B,) + lens.shape).copy()
    expanded, exp_scores = raw(dev, x, in_len, exp_seqs, exp_lens, w, lattice)
    assert np.array_equal(bits(expanded), bits(full)) and np.array_equal(bits(exp_scores), bits(full_scores))
    i32, _ = raw(dev, x, in_len, seqs, lens, w, lattice, seq_dtype=torch.int32)
    assert np.array_equal(bits(i32), bits(full))


# ---- 5. repeated classes

def repeated_inputs(lattice):
    T, B, C = 130, 2, 12
    x = inputs(14, T, B, C, lattice)
    rng = np.random.default_rng(15)
    half = [3 if i % 2 == 0 else int(rng.integers(4, C)) for i in range(60)]       # class 3 fills half of 60 positions
    seqs, lens = padded([(5, 5, 5, 5), tuple(half), () if lattice == "blank" else (7,)], L=60)
    return x, [130, 128], seqs, lens, weights(16, B, 3)


@pytest.mark.parametrize("lattice", LATTICES)
def test_repeated_classes(dev, lattice):
    x, in_len, seqs, lens, w = repeated_inputs(lattice)
    grad, scores = raw(dev, x, in_len, seqs, lens, w, lattice)
    rs, rg = reference(x, in_len, seqs, lens, w, lattice)
    assert np.isfinite(rs).all()
    check(grad, rs, rg, w, "repeated classes " + lattice)
    if lattice == "blank":                                      # the all-blank path alone: 1 on x[t, blank], exactly
        one = np.zeros((2, 3), np.float32)
        one[:, 2] = 1.0
        g, _ = raw(dev, x, in_len, seqs, lens, one, lattice)
        for b in range(2):
            assert np.allclose(g[:in_len[b], b, 0], 1.0, atol=GAMMA_ATOL) and not g[:, b, 1:].any()
            assert not g[in_len[b]:, b].any()


# ---- 6. determinism

@pytest.mark.parametrize("lattice", LATTICES)
@pytest.mark.parametrize("which", ["groups", "repeats"])
def test_two_calls_and_a_graph_replay_give_the_same_bits(dev, lattice, which):
    from ctc_amd import functional as F
    if which == "groups":
        x = inputs(11, 20, 3, 12, lattice)
        in_len = [20, 17, 9]
        seqs, lens = random_sequences(12, 17, 6, 12, lattice)
        w = weights(13, 3, 17)
    else:
        x, in_len, seqs, lens, w = repeated_inputs(lattice)
    first, s1 = raw(dev, x, in_len, seqs, lens, w, lattice)
    second, s2 = raw(dev, x, in_len, seqs, lens, w, lattice)
    assert np.array_equal(bits(first), bits(second)) and np.array_equal(bits(s1), bits(s2))
    xd, il = to_dev(dev, x), to_dev(dev, np.asarray(in_len), torch.int64)
    sq, sl = to_dev(dev, seqs, torch.int64), to_dev(dev, lens, torch.int64)
    xs, call = F._sequence_scores_call(xd, "x", il, sq, sl, None, 0 if lattice == "blank" else None)
    wd = to_dev(dev, w)
    out = torch.full(tuple(xd.shape), float("nan"), dtype=torch.float32, device=dev)
    F._sequence_scores_grad(xs, call, wd, out=out)              # (the scratch exists before the capture)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        F._sequence_scores_grad(xs, call, wd, out=out)          # this stream's scratch, outside the capture
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=side):
            F._sequence_scores_grad(xs, call, wd, out=out)
    out.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(bits(out.cpu().numpy()), bits(first))


# ---- 7. special cases

@pytest.mark.parametrize("lattice", LATTICES)
def test_special_cases(dev, lattice):
    T, B, C, L = 20, 5, 12, 4
    x = inputs(17, T, B, C, lattice)
    x[:, 3, [4, 7, 9]] = -np.inf                                # sample 3: a masked vocabulary, class 4 is a label
    if lattice == "blank":
        x[:, 3] = log_softmax32(np.where(np.isinf(x[:, 3]), -np.inf, x[:, 3]))
    in_len = [20, 0, 18, 20, 20]
    good = [(1, 2, 3), (5, 6), (2, 2, 1), (8,)]
    seqs, lens = padded(good + [(4, 5), (1, 99), (1, 2), (3, 1, 2, 5)], L=L)
    lens[6] = L + 3                                             # n = 4: through the masked class on sample 3; 5: a bad label;
    counts = [8, 8, 7, 8, 8]                                    # 6: a bad length; 7: beyond sample 2's count
    w = weights(18, B, 8)
    w[:, 5], w[:, 6] = np.nan, np.inf
    w[2, 7] = np.nan
    w[3, 4] = np.inf                                            # (-inf scored on sample 3 alone)
    exp_seqs = np.broadcast_to(seqs, (B,) + seqs.shape).copy()
    exp_lens = np.broadcast_to(lens, (B,) + lens.shape).copy()
    exp_seqs[4, :4] = [[1, 99, -1, -1], [0 if lattice == "blank" else -5, 1, -1, -1], [3, 3, 3, 3], [2, 1, 0, 0]]
    exp_lens[4, :4] = [2, 2, 9, -1]                             # sample 4: none of its candidates is scored: four NaN,
    exp_seqs[4, 4], exp_lens[4, 4] = [1, 1, 1, 1], 4            # one through a masked class (-inf), the rest absent
    counts[4] = 5
    x4 = x.copy()
    x4[:, 4, 1] = -np.inf
    grad, scores = raw(dev, x4, in_len, exp_seqs, exp_lens, w, lattice, counts=counts)
    rs, rg = reference(x4, in_len, exp_seqs, exp_lens, w, lattice, counts=counts)
    assert not np.isfinite(rs[4]).any() and not np.isfinite(rs[1, 1:]).any()
    assert np.isneginf(rs[3, 4]) and np.isnan(rs[0, 5]) and np.isnan(rs[0, 6]) and np.isneginf(rs[2, 7])
    check_scores(scores, rs, "special cases")
    check(grad, rs, rg, w, "special cases " + lattice)
    assert not grad[:, 1].any() and not grad[:, 4].any()        # T_b = 0; nobody scored
    assert not grad[18:, 2].any()
    assert not grad[:, 3][:, [4, 7, 9]].any()                   # -inf inputs: exactly 0
    assert np.array_equal(bits(scores), bits(forward(dev, x4, in_len, exp_seqs, exp_lens, lattice, counts=counts)))
    # the other samples' bits do not depend on the bad candidates being there
    keep = [0, 1, 2, 3, 4, 7]                                   # (5 and 6, the NaN-scored ones with w = NaN / inf, taken out)
    clean, _ = raw(dev, x4, in_len, exp_seqs[:, keep], exp_lens[:, keep], w[:, keep], lattice, counts=[6, 6, 5, 6, 5])
    for b in (0, 2, 3):
        assert np.array_equal(bits(clean[:, b]), bits(grad[:, b])), b


# ---- 8. long chains

@pytest.mark.parametrize("lattice", LATTICES)
def test_long_chains(dev, lattice):
    T, B, C, N = 2000, 2, 50, 3
    x = inputs(19, T, B, C, lattice)
    seqs, lens = random_sequences(20, N, 180, C, lattice, lengths=[170, 165, 180], equal_neighbours=False)
    in_len = [2000, 1900]
    w = weights(21, B, N)
    grad, scores = raw(dev, x, in_len, seqs, lens, w, lattice)
    rs, rg = reference(x, in_len, seqs, lens, w, lattice)
    assert np.isfinite(rs).all() and np.abs(rs).min() > 4000.0
    check_scores(scores, rs, "long")
    check(grad, rs, rg, w, "T=2000 random %s" % lattice, atol=LONG_ATOL)
    if lattice == "blank":
        xp = log_softmax32(peaked_clip(70, T, B, 40, (3, 7, 5), 0))
        ps, pl = padded([(3, 7, 5), (3, 7), (7,)], L=3)
    else:
        xp = peaked_clip(71, T, B, 40, (3, 7, 0), 0)
        ps, pl = padded([(3, 7, 0), (3, 0), (7, 0)], L=3)
    grad, scores = raw(dev, xp, in_len, ps, pl, w, lattice)
    rs, rg = reference(xp, in_len, ps, pl, w, lattice)
    assert np.isfinite(rs).all() and np.all(np.abs(rs[:, 0]) < 20.0)
    check_scores(scores, rs, "long peaked")
    check(grad, rs, rg, w, "T=2000 peaked %s" % lattice, atol=LONG_ATOL)


# ---- 10. autograd

@pytest.mark.parametrize("lattice", LATTICES)
def test_autograd_is_the_raw_entry(dev, lattice):
    import ctc_amd
    T, B, C, N, L = 30, 4, 12, 5, 6
    x = inputs(22, T, B, C, lattice)
    in_len = [30, 25, 30, 11]
    seqs, lens = random_sequences(23, N, L, C, lattice)
    fn = ctc_amd.blank_sequence_scores if lattice == "blank" else ctc_amd.noblank_sequence_scores
    il, sq, sl = to_dev(dev, np.asarray(in_len), torch.int64), to_dev(dev, seqs), to_dev(dev, lens)
    plain = fn(to_dev(dev, x), il, sq, sl)
    assert not plain.requires_grad
    xd = to_dev(dev, x).requires_grad_(True)
    with torch.no_grad():
        assert not fn(xd, il, sq, sl).requires_grad
    s = fn(xd, il, sq, sl)
    assert s.requires_grad and np.array_equal(bits(s.detach().cpu().numpy()), bits(plain.cpu().numpy()))
    s.sum().backward()
    ones, _ = raw(dev, x, in_len, seqs, lens, np.ones((B, N), np.float32), lattice)
    assert xd.grad.is_contiguous() and xd.grad.dtype == torch.float32
    assert np.array_equal(bits(xd.grad.cpu().numpy()), bits(ones))
    w = weights(24, B, N)
    xd.grad = None
    fn(xd, il, sq, sl).backward(to_dev(dev, w))
    want, _ = raw(dev, x, in_len, seqs, lens, w, lattice)
    assert np.array_equal(bits(xd.grad.cpu().numpy()), bits(want))
    assert ctc_amd.release_workspaces() > 0                     # the scratch was the cache's, and is freed
    assert ctc_amd.release_workspaces() == 0


def test_autograd_behind_log_softmax_against_torch(dev):
    import ctc_amd
    T, B, C, L = 30, 4, 12, 6
    logits = inputs(25, T, B, C, "noblank")
    in_len = np.array([30, 25, 30, 14])
    tgt, tl = random_sequences(26, B, L, C, "blank")
    w = weights(27, B, 1)
    z = torch.tensor(logits, dtype=torch.float64, requires_grad=True)
    nll = torch.nn.functional.ctc_loss(torch.log_softmax(z, 2), torch.tensor(tgt), torch.tensor(in_len), torch.tensor(tl),
                                       blank=0, reduction="none")
    (-(nll * torch.tensor(w[:, 0], dtype=torch.float64))).sum().backward()
    zd = to_dev(dev, logits).requires_grad_(True)
    s = ctc_amd.blank_sequence_scores(torch.log_softmax(zd, 2), to_dev(dev, in_len), to_dev(dev, tgt[:, None, :]),
                                      to_dev(dev, tl[:, None]))
    (s * to_dev(dev, w)).sum().backward()
    err = np.abs(zd.grad.cpu().numpy().astype(np.float64) - z.grad.numpy()).max(axis=(0, 2))
    # g - softmax rowsum(g): an occupancy error of A |w| reaches a logit at most doubled
    bound = 2 * GAMMA_ATOL * np.abs(w[:, 0])
    print("behind log_softmax: %.3f of the bound" % (err / bound).max())
    assert np.all(err <= bound)


# ---- 11. an MWER step end to end

@pytest.mark.parametrize("lattice", LATTICES)
def test_mwer_step(dev, lattice):
    import ctc_amd
    T, B, C, N = 30, 4, 12, 4
    # logits that lean towards the reference transcript (each label held for two frames and raised by 3), so that the
    # list holds the reference and near misses of it: the hypotheses' error counts differ and every sample has weights
    logits = inputs(29, T, B, C, "noblank", scale=1.0)
    in_len = np.array([30, 25, 30, 14])
    refs, ref_len = random_sequences(30, B, 6, C, "blank", equal_neighbours=False)
    for b in range(B):
        for i in range(int(ref_len[b])):
            logits[2 * i:2 * i + 2, b, refs[b, i]] += 3.0
        logits[2 * int(ref_len[b]):, b, 0 if lattice == "blank" else refs[b, int(ref_len[b]) - 1]] += 3.0
    zd = to_dev(dev, logits).requires_grad_(True)
    il = to_dev(dev, in_len)
    if lattice == "blank":
        x = torch.log_softmax(zd, 2)
        hyp = ctc_amd.blank_beam_search(x.detach(), il, beam_width=8, nbest=N)
        scores = ctc_amd.blank_sequence_scores(x, il, hyp.tokens, hyp.lengths, counts=hyp.count)
    else:
        x = zd
        hyp = ctc_amd.noblank_beam_search(x.detach(), il, beam_width=8, nbest=N)
        scores = ctc_amd.noblank_sequence_scores(x, il, hyp.tokens, hyp.lengths, counts=hyp.count)
    if x is not zd:
        x.retain_grad()
    rd, rl = to_dev(dev, refs), to_dev(dev, ref_len)
    dist = torch.stack([ctc_amd.edit_distance(hyp.tokens[:, n], hyp.lengths[:, n], rd, rl) for n in range(N)], dim=1)
    dist = dist.to(torch.float32)
    ok = torch.isfinite(scores)
    post = torch.softmax(torch.where(ok, scores, scores.new_tensor(-1e30)), dim=1)
    risk = (torch.where(ok, post * dist, post.new_zeros(())).sum(dim=1)).mean()
    risk.backward()
    torch.cuda.synchronize()
    # the float64 reference, given the same hypotheses: w = d risk / d scores from the reference's own scores
    tokens, lengths, count = hyp.tokens.cpu().numpy(), hyp.lengths.cpu().numpy(), hyp.count.cpu().numpy()
    x64 = x.detach().cpu().numpy()
    rs, _ = reference(x64, in_len, tokens, lengths, np.zeros((B, N)), lattice, counts=count)
    s64 = torch.tensor(np.where(np.isfinite(rs), rs, -1e30), dtype=torch.float64, requires_grad=True)
    okr = torch.tensor(np.isfinite(rs))
    assert np.array_equal(okr.numpy(), ok.cpu().numpy()) and okr.any(dim=1).all()
    p64 = torch.softmax(s64, dim=1)
    (torch.where(okr, p64 * torch.tensor(dist.cpu().numpy(), dtype=torch.float64), torch.zeros((), dtype=torch.float64))
     .sum(dim=1)).mean().backward()
    w = s64.grad.numpy()
    _, rg = reference(x64, in_len, tokens, lengths, w, lattice, counts=count)
    live = np.isfinite(rs)
    bound = GAMMA_ATOL * np.where(live, np.abs(w), 0).sum(axis=1)
    assert np.all(bound > 0)
    # at the kernel's input (the log-probabilities, or the logits themselves): the bound as it stands
    got = x.grad.cpu().numpy().astype(np.float64)
    err = np.abs(got - rg).max(axis=(0, 2))
    print("MWER %s: %.3f of the bound" % (lattice, (err / bound).max()))
    assert not np.isnan(got).any() and np.all(err <= bound)
    assert float(np.abs(got).max()) > 0.0
    if lattice == "blank":
        # at the logits: g - softmax rowsum(g); an error of g appears once itself and once, times softmax <= 1, through
        # the row sum (the total occupancy, an error of the same kind): twice the bound
        pulled = rg - np.exp(x64.astype(np.float64)) * rg.sum(axis=2, keepdims=True)
        got = zd.grad.cpu().numpy().astype(np.float64)
        err = np.abs(got - pulled).max(axis=(0, 2))
        print("MWER blank, at the logits: %.3f of the bound" % (err / (2 * bound)).max())
        assert not np.isnan(got).any() and np.all(err <= 2 * bound)
