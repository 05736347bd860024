"""The evaluation kernels on the MI355X: ctc_amd.collapse_frames, ctc_amd.edit_distance and ctc_amd.label_error_rate against
the Python / numpy restatements of tests/eval_ref.py.  Both operations are integer-exact, so every comparison is for
equality: torch.equal on the integers, bit equality on the confidences (no tolerance anywhere in this file)."""
import functools

import numpy as np
import pytest
import torch

from tests.eval_ref import collapse_ref, edit_distance_ref, label_error_rate_ref

pytestmark = pytest.mark.gpu

BLANK = 0
LENGTHS = [0, 1, 63, 64, 65, 129]                              # T_b around the 64-frame chunks of the scan
WIDTHS = [0, 1, 63, 64, 65, 127, 128, 129, 1023]               # M: every K of the kernel and each lane boundary


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    import ctc_amd  # noqa: F401  (raises if libctc_amd.so is missing)
    return torch.device("cuda:0")


def runs(rng, T, alphabet, stay=0.6):
    """T frame labels from `alphabet` in which a frame repeats the one before it with probability `stay`"""
    out = np.empty(T, np.int64)
    for t in range(T):
        out[t] = out[t - 1] if t and rng.random() < stay else rng.choice(alphabet)
    return out


def bits(a):
    return a.view(torch.int32) if isinstance(a, torch.Tensor) else a.view(np.int32)


def check_collapse(got, frames, in_len, blank, frame_conf=None, max_tokens=None):
    """every output against the restatement, for equality"""
    fr = frames.cpu().numpy()
    fc = None if frame_conf is None else frame_conf.cpu().numpy()
    tokens, lengths, start, end, conf = collapse_ref(fr, np.asarray(in_len), blank, fc, max_tokens)
    assert got.tokens.dtype == torch.int32 and got.lengths.dtype == torch.int64
    assert got.start.dtype == torch.int32 and got.end.dtype == torch.int32
    assert torch.equal(got.lengths.cpu(), torch.from_numpy(lengths))
    assert torch.equal(got.tokens.cpu(), torch.from_numpy(tokens))
    assert torch.equal(got.start.cpu(), torch.from_numpy(start))
    assert torch.equal(got.end.cpu(), torch.from_numpy(end))
    if fc is None:
        assert got.conf is None
    else:
        assert got.conf.dtype == torch.float32
        assert torch.equal(bits(got.conf.cpu()), torch.from_numpy(bits(conf)))
    return tokens, lengths, start, end, conf


@functools.lru_cache(maxsize=None)
def chunk_case():
    """(frames [6,130] int64, in_len, frame_conf) -- T_b = 0, 1, 63, 64, 65, 129, built once and left unchanged.  Behind
    T_b the row goes on: frame T_b repeats frame T_b - 1 (read, it would stretch the last run), then labels that occur
    nowhere else (read, they would add tokens); frame_conf behind T_b is huge."""
    rng = np.random.default_rng(11)
    T = 130
    frames = np.stack([runs(rng, T, [BLANK, 1, 2, 3, 4, 5], stay=0.25) for _ in LENGTHS])
    conf = rng.random((len(LENGTHS), T), dtype=np.float32)
    for b, Tb in enumerate(LENGTHS):
        if Tb:
            frames[b, Tb - 1] = 1 + b % 3                      # a label (not the blank) ends the sample ...
        frames[b, Tb:] = rng.integers(6, 9, T - Tb)
        if Tb:
            frames[b, Tb] = frames[b, Tb - 1]                  # ... and the garbage behind it continues that run
        conf[b, Tb:] = 1e30
    return torch.from_numpy(frames), list(LENGTHS), torch.from_numpy(conf)


@pytest.mark.parametrize("dtype", [torch.int64, torch.int32])
@pytest.mark.parametrize("with_conf", [False, True])
@pytest.mark.parametrize("blank", [BLANK, None])
def test_collapse_chunk_lengths(dev, dtype, with_conf, blank):
    import ctc_amd
    frames, in_len, conf = chunk_case()
    fr = frames.to(dev, dtype)
    fc = conf.to(dev) if with_conf else None
    got = ctc_amd.collapse_frames(fr, in_len, blank=blank, frame_conf=fc)
    tokens, lengths, start, end, cf = check_collapse(got, frames, in_len, blank, conf if with_conf else None)
    # the padding, spelled out: -1 / -1 / -1 / 0 at and beyond the count, in every output
    for b, n in enumerate(lengths):
        assert (got.tokens[b, n:] == -1).all() and (got.start[b, n:] == -1).all() and (got.end[b, n:] == -1).all()
        assert (got.tokens[b, :n] >= 0).all() and (got.end[b, :n] >= got.start[b, :n]).all()
        if with_conf:
            assert (bits(got.conf[b, n:]) == 0).all()
    assert lengths[0] == 0 and int(end[5, lengths[5] - 1]) == 128      # T_b = 0: nothing; T_b = 129: ends at frame 128


@pytest.mark.parametrize("layout", ["contiguous", "time_major_view", "column_slice", "row_slice"])
def test_collapse_input_layouts(dev, layout):
    """[B,T] contiguous, the .t() view of a [T,B] tensor, and slices of a wider tensor: no copy, the same answer"""
    import ctc_amd
    frames, in_len, conf = chunk_case()
    B, T = frames.shape
    if layout == "contiguous":
        fr, fc = frames.to(dev), conf.to(dev)
    elif layout == "time_major_view":
        fr, fc = frames.t().contiguous().to(dev).t(), conf.t().contiguous().to(dev).t()
        assert fr.stride() == (1, B)
    elif layout == "column_slice":
        wide = torch.full((B, T + 12), 77, dtype=torch.int64)
        wide[:, 5:5 + T] = frames
        widec = torch.full((B, T + 12), 1e30)
        widec[:, 7:7 + T] = conf
        fr, fc = wide.to(dev)[:, 5:5 + T], widec.to(dev)[:, 7:7 + T]
        assert fr.stride() == (T + 12, 1)
    else:
        wide = torch.full((B + 5, T), 77, dtype=torch.int64)
        wide[2:2 + B] = frames
        fr, fc = wide.to(dev)[2:2 + B], conf.to(dev)
    ptr = fr.data_ptr()
    got = ctc_amd.collapse_frames(fr, in_len, blank=BLANK, frame_conf=fc)
    assert fr.data_ptr() == ptr
    check_collapse(got, frames, in_len, BLANK, conf)


def test_collapse_long_sample(dev):
    """T = 2000: 32 chunks, more tokens than one chunk holds, runs that cross chunk boundaries, a second, short sample"""
    import ctc_amd
    rng = np.random.default_rng(12)
    T = 2000
    frames = np.stack([runs(rng, T, [BLANK, 1, 2, 3, 4], stay=0.55), runs(rng, T, [BLANK, 1], stay=0.97)])
    conf = rng.random((2, T), dtype=np.float32)
    in_len = [2000, 777]
    fr, fc = torch.from_numpy(frames), torch.from_numpy(conf)
    for blank in (BLANK, None):
        got = ctc_amd.collapse_frames(fr.to(dev), in_len, blank=blank, frame_conf=fc.to(dev))
        _, lengths, _, _, _ = check_collapse(got, fr, in_len, blank, fc)
        assert lengths[0] > 128


def test_collapse_beyond_the_default_lds(dev):
    """T = 6000 with max_tokens = T: 72 KB of LDS, above the 64 KB a launch gets without asking; T = 4096 below it"""
    import ctc_amd
    rng = np.random.default_rng(14)
    for T in (4096, 6000):
        frames = np.stack([runs(rng, T, [BLANK, 1, 2, 3], stay=0.5), runs(rng, T, [BLANK, 1, 2, 3], stay=0.9)])
        conf = rng.random((2, T), dtype=np.float32)
        in_len = [T, T - 65]
        fr, fc = torch.from_numpy(frames), torch.from_numpy(conf)
        got = ctc_amd.collapse_frames(fr.to(dev), in_len, blank=BLANK, frame_conf=fc.to(dev))
        _, lengths, _, _, _ = check_collapse(got, fr, in_len, BLANK, fc)
        assert lengths[0] > 900


def test_collapse_shaped_rows(dev):
    """a run across a 64-frame boundary, all frames equal, all blank, strictly alternating, a blank a"""
    import ctc_amd
    T = 200
    a = 5
    rows = np.zeros((6, T), np.int64)
    rows[0, :] = np.arange(T) % 7 + 1
    rows[0, 60:70] = 9                                         # one run over frames 60..69
    rows[1, :] = a
    rows[2, :] = BLANK
    rows[3, :] = 1 + np.arange(T) % 2
    rows[4, :3] = [a, BLANK, a]
    rows[5, :2] = [a, a]
    in_len = [200, 200, 200, 200, 3, 2]
    conf = np.random.default_rng(13).random((6, T), dtype=np.float32)
    fr, fc = torch.from_numpy(rows), torch.from_numpy(conf)
    got = ctc_amd.collapse_frames(fr.to(dev), in_len, blank=BLANK, frame_conf=fc.to(dev))
    tokens, lengths, start, end, _ = check_collapse(got, fr, in_len, BLANK, fc)
    assert lengths.tolist() == [191, 1, 0, 200, 2, 1]
    assert (tokens[0, 60], start[0, 60], end[0, 60]) == (9, 60, 69)
    assert (start[1, 0], end[1, 0]) == (0, 199)
    assert tokens[4, :2].tolist() == [a, a] and start[4, :2].tolist() == [0, 2]
    assert (start[5, 0], end[5, 0]) == (0, 1)
    got = ctc_amd.collapse_frames(fr.to(dev), in_len, blank=None)              # the blank is a label like the others
    _, lengths, _, _, _ = check_collapse(got, fr, in_len, None)
    assert lengths.tolist() == [191, 1, 1, 200, 3, 1]


def test_collapse_no_blank_keeps_minus_one(dev):
    """blank=None on label positions with -1 (a failed best path): taken literally"""
    import ctc_amd
    rows = np.array([[0, 0, 1, 1, 1, 2, -1, -1], [-1] * 8, [0, -1, 0, -1, 1, 1, 1, 1]], np.int64)
    in_len = [8, 8, 6]
    for dtype in (torch.int32, torch.int64):
        fr = torch.from_numpy(rows).to(dtype)
        got = ctc_amd.collapse_frames(fr.to(dev), in_len, blank=None)
        tokens, lengths, _, _, _ = check_collapse(got, fr, in_len, None)
        assert lengths.tolist() == [4, 1, 5] and tokens[0, :4].tolist() == [0, 1, 2, -1] and tokens[1, 0] == -1


@pytest.mark.parametrize("max_tokens", [1, 5, 64, 65])
def test_collapse_truncation(dev, max_tokens):
    """max_tokens below the count: lengths stays true, the stored prefix is exact"""
    import ctc_amd
    frames, in_len, conf = chunk_case()
    got = ctc_amd.collapse_frames(frames.to(dev), in_len, blank=None, frame_conf=conf.to(dev), max_tokens=max_tokens)
    assert got.tokens.shape == (len(in_len), max_tokens)
    _, lengths, _, _, _ = check_collapse(got, frames, in_len, None, conf, max_tokens)
    full = collapse_ref(frames.numpy(), np.asarray(in_len), None)
    assert (lengths == full[1]).all() and lengths.max() > max_tokens
    assert (got.tokens.cpu().numpy() == full[0][:, :max_tokens]).all()


# ---- edit distance ---------------------------------------------------------------------------------------------------

def check_edit(dev, hyp, hyp_len, ref, ref_len, **kw):
    import ctc_amd
    got = ctc_amd.edit_distance(hyp.to(dev), hyp_len, ref.to(dev), ref_len, **kw)
    want = edit_distance_ref(hyp.numpy(), hyp_len, ref.numpy(), ref_len)
    assert got.dtype == torch.int32 and got.shape == (hyp.shape[0],)
    assert torch.equal(got.cpu(), torch.from_numpy(want))
    return want


@functools.lru_cache(maxsize=None)
def width_case(M):
    """(hyp [6,M+3], hyp_len, ref [6,M], ref_len): hypotheses shorter than, as long as and longer than the reference, over
    four symbols (so that alignments are not trivial); the reference's last sample is one label short"""
    rng = np.random.default_rng(100 + M)
    N = M + 3
    hyp = torch.from_numpy(rng.integers(1, 5, (6, N)))
    ref = torch.from_numpy(rng.integers(1, 5, (6, M)))
    hyp_len = [0, max(M - 2, 0), max(M - 1, 0), M, M + 1, M + 3]
    ref_len = [M, M, M, M, M, max(M - 1, 0)]
    return hyp, hyp_len, ref, ref_len


@pytest.mark.parametrize("M", WIDTHS)
def test_edit_distance_reference_widths(dev, M):
    hyp, hyp_len, ref, ref_len = width_case(M)
    want = check_edit(dev, hyp, hyp_len, ref, ref_len)
    assert want[0] == M                                        # an empty hypothesis: M insertions
    if M <= 129:                                               # the hypothesis TENSOR narrower than / as wide as the reference
        for N in sorted({max(M - 1, 0), M}):
            check_edit(dev, hyp[:, :N], [min(n, N) for n in hyp_len], ref, ref_len)


def test_edit_distance_empty_hypotheses(dev):
    """N = 0: a hypothesis tensor without columns"""
    ref = torch.from_numpy(np.random.default_rng(3).integers(1, 5, (3, 20)))
    want = check_edit(dev, torch.zeros((3, 0), dtype=torch.int64), [0, 0, 0], ref, [20, 0, 7])
    assert want.tolist() == [20, 0, 7]


def test_edit_distance_long_hypothesis(dev):
    """N = 2000 against M = 100: a hypothesis as long as T"""
    rng = np.random.default_rng(4)
    hyp = torch.from_numpy(rng.integers(1, 5, (3, 2000)))
    ref = torch.from_numpy(rng.integers(1, 5, (3, 100)))
    want = check_edit(dev, hyp, [2000, 1999, 130], ref, [100, 99, 100])
    assert want[0] >= 1900


def test_edit_distance_known_answers(dev):
    """identical sequences, disjoint alphabets, one edit at the first / last position, repeated tokens"""
    rng = np.random.default_rng(6)
    M = 130                                                    # two cells per lane ... three lanes beyond a wave's worth
    base = rng.integers(1, 50, M)
    rows, hyp_len, want = [], [], []

    def add(h, d):
        rows.append(np.concatenate([h, np.full(M + 1 - len(h), 99)]))
        hyp_len.append(len(h))
        want.append(d)
    add(base, 0)                                               # identical
    add(base + 100, M)                                         # disjoint alphabets: max(N, M)
    add((base + 100)[:40], M)
    add(np.concatenate([[77], base]), 1)                       # an insertion at the first position
    add(np.concatenate([base, [77]]), 1)                       # ... at the last
    add(base[1:], 1)                                           # a deletion at the first position
    add(base[:-1], 1)                                          # ... at the last
    add(np.concatenate([[77], base[1:]]), 1)                   # a substitution at the first position
    add(np.concatenate([base[:-1], [77]]), 1)                  # ... at the last
    hyp = torch.from_numpy(np.stack(rows))
    ref = torch.from_numpy(np.tile(base, (len(rows), 1)))
    got = check_edit(dev, hyp, hyp_len, ref, [M] * len(rows))
    assert got.tolist() == want
    # repeated tokens: a^n against a^m is |n - m|; a two-symbol alphabet with long repeats
    n = [0, 1, 70, 64, 129, 130]
    m = [130, 130, 3, 64, 128, 0]
    ones = torch.ones((6, 130), dtype=torch.int64)
    got = check_edit(dev, ones, n, ones, m)
    assert got.tolist() == [abs(a - b) for a, b in zip(n, m)]
    two = torch.from_numpy(np.stack([runs(rng, 130, [1, 2], stay=0.9) for _ in range(12)]))
    check_edit(dev, two[:6], [130, 100, 64, 65, 1, 30], two[6:], [130, 130, 65, 64, 130, 2])


def test_edit_distance_dtypes_strides_and_garbage(dev):
    """int32 against int64, a strided reference, and elements beyond both lengths that would change the answer if read"""
    import ctc_amd
    rng = np.random.default_rng(7)
    B, N, M = 5, 90, 70
    hyp = rng.integers(1, 6, (B, N))
    ref = rng.integers(1, 6, (B, M))
    hyp_len, ref_len = [90, 50, 0, 33, 64], [70, 64, 20, 0, 1]
    want = edit_distance_ref(hyp, hyp_len, ref, ref_len)
    for b in range(B):                                         # beyond the lengths: each sequence goes on as the OTHER one does
        n, m = hyp_len[b], ref_len[b]
        k = min(N - n, M - m)
        hyp[b, n:n + k] = 9
        ref[b, m:m + k] = 9
    h, r = torch.from_numpy(hyp), torch.from_numpy(ref)
    for hd, rd in [(torch.int32, torch.int64), (torch.int64, torch.int32), (torch.int32, torch.int32)]:
        got = ctc_amd.edit_distance(h.to(dev, hd), hyp_len, r.to(dev, rd), ref_len)
        assert torch.equal(got.cpu(), torch.from_numpy(want))
    wide = torch.full((B, M + 30), 9, dtype=torch.int64)
    wide[:, 11:11 + M] = r
    rs = wide.to(dev)[:, 11:11 + M]                            # a batch stride of M + 30: read in place
    assert rs.stride() == (M + 30, 1)
    assert torch.equal(ctc_amd.edit_distance(h.to(dev), hyp_len, rs, ref_len).cpu(), torch.from_numpy(want))
    every2 = torch.full((B, 2 * M), 9, dtype=torch.int64)
    every2[:, ::2] = r
    assert torch.equal(ctc_amd.edit_distance(h.to(dev), hyp_len, every2.to(dev)[:, ::2], ref_len).cpu(), torch.from_numpy(want))
    rows = torch.full((2 * B, N), 9, dtype=torch.int64)
    rows[::2] = h
    assert torch.equal(ctc_amd.edit_distance(rows.to(dev)[::2], hyp_len, r.to(dev), ref_len).cpu(), torch.from_numpy(want))


@functools.lru_cache(maxsize=None)
def mixed_batch():
    """70 samples (four per workgroup: seventeen workgroups and half of another) of mixed lengths, empty ones among them"""
    rng = np.random.default_rng(8)
    B, N, M = 70, 48, 70
    hyp, ref = rng.integers(1, 7, (B, N)), rng.integers(1, 7, (B, M))
    hyp_len, ref_len = rng.integers(0, N + 1, B), rng.integers(0, M + 1, B)
    hyp_len[:4] = [0, 0, N, N]
    ref_len[:4] = [0, M, 0, M]
    for b in range(8, B, 3):                                   # hypotheses that ARE close to their reference
        n = min(int(ref_len[b]), N)
        hyp[b, :n] = ref[b, :n]
        hyp[b, n // 2] = 7
        hyp_len[b] = n
    return torch.from_numpy(hyp), hyp_len.tolist(), torch.from_numpy(ref), ref_len.tolist()


def test_edit_distance_mixed_batch(dev):
    hyp, hyp_len, ref, ref_len = mixed_batch()
    want = check_edit(dev, hyp, hyp_len, ref, ref_len)
    assert want[:4].tolist() == [0, 70, 48, want[3]] and len(set(want.tolist())) > 10


def test_label_error_rate(dev):
    import ctc_amd
    hyp, hyp_len, ref, ref_len = mixed_batch()
    for rl in (ref_len, [0] * len(ref_len)):                   # (no reference label at all: sum(dist) / 1)
        want_ler, want_dist = label_error_rate_ref(hyp.numpy(), hyp_len, ref.numpy(), rl)
        ler, dist = ctc_amd.label_error_rate(hyp.to(dev), hyp_len, ref.to(dev), rl)
        assert ler.dtype == torch.float32 and ler.dim() == 0 and ler.device == dist.device and dist.is_cuda
        assert torch.equal(dist.cpu(), torch.from_numpy(want_dist))
        assert bits(ler.cpu().reshape(1)).item() == bits(np.array([want_ler], np.float32))[0]
    assert want_ler == np.float32(sum(hyp_len))


# ---- the pieces together ---------------------------------------------------------------------------------------------

def test_best_path_collapses_to_its_targets(dev):
    """T = 40, B = 6, C = 12: the classes along blank_best_path's path, collapsed, are the target prefix -- distance 0"""
    import ctc_amd
    T, B, C, S = 40, 6, 12, 9
    g = torch.Generator().manual_seed(21)
    lp = torch.randn(T, B, C, generator=g).log_softmax(2).to(dev)
    tg = torch.randint(1, C, (B, S), generator=g)
    tg[1, 1] = tg[1, 0]                                        # adjacent repeats: a blank must come between them
    tg[2, :] = 3
    L = torch.tensor([9, 9, 9, 1, 5, 0])
    Tb = torch.tensor([40, 30, 19, 1, 40, 7])                  # (every sample has an alignment: T_b >= L_b + repeats)
    path, score = ctc_amd.blank_best_path(lp, tg.to(dev), Tb, L, blank=BLANK)
    assert bool(torch.isfinite(score).all())
    classes, frame_lp = ctc_amd.blank_forced_align(lp, tg.to(dev), Tb, L, blank=BLANK)
    got = ctc_amd.collapse_frames(classes, Tb, blank=BLANK, frame_conf=frame_lp.exp())
    check_collapse(got, classes.cpu(), Tb.tolist(), BLANK, frame_lp.exp().cpu())
    assert torch.equal(got.lengths.cpu(), L)
    for b in range(B):
        assert torch.equal(got.tokens[b, :L[b]].cpu().long(), tg[b, :L[b]])
    dist = ctc_amd.edit_distance(got.tokens, got.lengths, tg.to(dev), L)
    assert dist.tolist() == [0] * B
    ler, _ = ctc_amd.label_error_rate(got.tokens, got.lengths, tg.to(dev), L)
    assert ler.item() == 0.0
    # the greedy decision goes the same way without a copy: argmax of [T,B,C] is [T,B]
    greedy = lp.argmax(-1)
    dec = ctc_amd.collapse_frames(greedy.t(), Tb, blank=BLANK)
    check_collapse(dec, greedy.t().cpu(), Tb.tolist(), BLANK)


def _both(frames, in_len, conf, hyp, hyp_len, ref, ref_len):
    import ctc_amd
    c = ctc_amd.collapse_frames(frames, in_len, blank=BLANK, frame_conf=conf)
    d = ctc_amd.edit_distance(hyp, hyp_len, ref, ref_len)
    return [c.tokens, c.lengths, c.start, c.end, c.conf, d]


def _device_inputs(dev):
    frames, in_len, conf = chunk_case()
    hyp, hyp_len, ref, ref_len = mixed_batch()
    i64 = functools.partial(torch.tensor, dtype=torch.int64, device=dev)
    return (frames.to(dev), i64(in_len), conf.to(dev), hyp.to(dev), i64(hyp_len), ref.to(dev), i64(ref_len))


def test_determinism(dev):
    """two calls give equal bits in fresh output tensors"""
    args = _device_inputs(dev)
    first, second = _both(*args), _both(*args)
    for a, b in zip(first, second):
        assert a.data_ptr() != b.data_ptr()
        assert torch.equal(bits(a) if a.dtype is torch.float32 else a, bits(b) if b.dtype is torch.float32 else b)


def test_capture_and_status(dev):
    """both calls captured into ONE torch.cuda.graph on a side stream (a single chain) and replayed twice over outputs
    filled with garbage give the eager calls' bits; nothing here touches a workspace, and the status stays 0"""
    import ctc_amd
    args = _device_inputs(dev)
    eager = _both(*args)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                              # warm-up on the capture stream
        _both(*args)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        captured = _both(*args)
    for _ in range(2):
        for x in captured:
            x.fill_(float("nan") if x.dtype is torch.float32 else 123456)
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(eager, captured):
            assert torch.equal(bits(a) if a.dtype is torch.float32 else a, bits(b) if b.dtype is torch.float32 else b)
    assert ctc_amd.workspace_status() == 0
