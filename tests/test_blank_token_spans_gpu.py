"""Blank-CTC token spans on the MI355X: blank_token_spans against the calls it composes (blank_best_path and
blank_posteriors, bit for bit), against the numpy restatement of the span stage (tests/test_blank_token_spans_abi.py)
and against the float64 posteriors; structure of the spans, input forms, a workspace shared with the loss, determinism
and graph capture.  Narrow lattices (S <= 255, K = 2, 4, 8 states per lane) and wide ones (256 <= S <= 1023, W = 2, 3, 4
waves per row) run the same assertions."""
import functools

import numpy as np
import pytest
import torch

from tests.helpers import np_, synth_blank
from tests.test_blank_posteriors_abi import posteriors_blank
from tests.test_blank_posteriors_gpu import _case
from tests.test_blank_token_spans_abi import padded, spans_of_path
from tests.test_blank_wide_gpu import CASES, make_case

pytestmark = pytest.mark.gpu

NARROW = {
    "T1": ((1, 3, 5, 1), False),
    "S20r": ((150, 16, 158, 20), True),
    "S60r": ((300, 6, 400, 60), True),                            # K = 2
    "S100": ((300, 6, 400, 100), False),                          # K = 4
    "S255r": ((40, 5, 600, 255), True),                           # K = 8 (T < S: only its L = 0 samples have an alignment)
    "S255": ((300, 4, 600, 255), False),                          # K = 8 with every state on some path
}
FIELDS = ("start", "end", "conf", "frame_conf", "path", "score", "nll")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    import ctc_amd  # noqa: F401  (raises if libctc_amd.so is missing)
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(lp, tgt, Tb, L) of a narrow or a wide case, built once and left unchanged"""
    if name in NARROW:
        shape, ragged = NARROW[name]
        return _case(31, *shape, ragged)
    return make_case(name)


def _spans(dev, lp, tgt, Tb, L, blank=0, lpd=None):
    import ctc_amd
    lpd = lp.to(dev) if lpd is None else lpd
    out = ctc_amd.blank_token_spans(lpd, tgt.to(dev), Tb.to(dev), L.to(dev), blank=blank)
    torch.cuda.synchronize()
    return out


def _bits(t):
    return t.view(torch.int32) if t.dtype is torch.float32 else t


def _same(a, b, what=""):
    for name, x, y in zip(FIELDS, a, b):
        assert torch.equal(_bits(x), _bits(y)), "%s %s" % (what, name)


def _composition(dev, out, lp, tgt, Tb, L, blank=0, lpd=None):
    """the identities of the contract: path, score, nll and frame_conf bitwise against the two existing calls, the spans
    bitwise against the restatement on that path and those confidences"""
    import ctc_amd
    lpd = lp.to(dev) if lpd is None else lpd
    args = (lpd, tgt.to(dev), Tb.to(dev), L.to(dev))
    path, score = ctc_amd.blank_best_path(*args, blank=blank)
    gamma, nll = ctc_amd.blank_posteriors(*args, blank=blank)
    torch.cuda.synchronize()
    S = tgt.shape[1]
    assert out.path.dtype is torch.int32 and out.start.dtype is torch.int32 and out.end.dtype is torch.int32
    assert tuple(out.start.shape) == tuple(out.end.shape) == tuple(out.conf.shape) == (tgt.shape[0], S)
    assert torch.equal(out.path, path), "path"
    assert torch.equal(_bits(out.score), _bits(score)), "score"
    assert torch.equal(_bits(out.nll), _bits(nll)), "nll"
    want = torch.gather(gamma, 2, path.clamp(min=0).long().unsqueeze(2)).squeeze(2)
    want = torch.where(path < 0, torch.zeros_like(want), want)
    assert torch.equal(_bits(out.frame_conf), _bits(want)), "frame_conf"
    s, e, c = spans_of_path(np_(path), np_(out.frame_conf), np_(Tb), np_(L))
    assert np.array_equal(np_(out.start), padded(s, S, -1)), "start"
    assert np.array_equal(np_(out.end), padded(e, S, -1)), "end"
    assert np.array_equal(np_(out.conf).view(np.int32), padded(c, S, 0).view(np.int32)), "conf"
    return path, gamma


def _kinds(lp, tgt, Tb, L):
    """which kinds of samples a batch holds, from its inputs (a sample has an alignment when T_b covers its labels and
    one blank per adjacent repeat)"""
    T, B, S = lp.shape[0], tgt.shape[0], tgt.shape[1]
    reps = torch.tensor([int((tgt[b, 1:int(L[b])] == tgt[b, :max(int(L[b]) - 1, 0)]).sum()) for b in range(B)])
    feasible = Tb >= L + reps
    return {"empty": bool((L == 0).any()), "infeasible": bool((~feasible).any()),
            "short": bool((Tb < T).any()),
            "padded": bool((L < S).any()), "repeat": bool((reps > 0).any())}


# ---- 1. composition, bitwise -------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(NARROW) + list(CASES))
def test_composition(dev, name):
    lp, tgt, Tb, L = inputs(name)
    out = _spans(dev, lp, tgt, Tb, L)
    _composition(dev, out, lp, tgt, Tb, L)
    ragged = NARROW[name][1] if name in NARROW else name == "ragged"
    if ragged:
        kinds = _kinds(lp, tgt, Tb, L)
        assert all(kinds.values()), kinds


# ---- 2. structure ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["S20r", "ragged"])
def test_structure(dev, name):
    lp, tgt, Tb, L = inputs(name)
    out = _spans(dev, lp, tgt, Tb, L)
    start, end, conf, fc, path = (np_(t) for t in out[:5])
    fin = np.isfinite(np_(out.score))
    assert fin.any() and (~fin).any() and (np_(L) == 0).any()
    for b in range(tgt.shape[0]):
        tb, l = int(Tb[b]), int(L[b])
        assert (fc[b, tb:] == 0).all()
        if not fin[b] or l == 0:
            assert (start[b] == -1).all() and (end[b] == -1).all() and (conf[b] == 0).all()
            if not fin[b]:
                assert (fc[b] == 0).all() and (path[b] == -1).all()
            continue
        s, e = start[b, :l], end[b, :l]
        assert (start[b, l:] == -1).all() and (end[b, l:] == -1).all() and (conf[b, l:] == 0).all()
        assert (0 <= s).all() and (s < e).all() and (e[:-1] <= s[1:]).all() and e[-1] <= tb
        rep = np_(tgt[b, 1:l] == tgt[b, :l - 1])
        assert (e[:-1][rep] < s[1:][rep]).all(), "a blank between two equal labels"
        inside = np.zeros(tb, dtype=bool)
        for j in range(l):
            assert (path[b, s[j]:e[j]] == 2 * j + 1).all()
            inside[s[j]:e[j]] = True
        assert (path[b, :tb][~inside] % 2 == 0).all() and (path[b, :tb][~inside] >= 0).all()
        assert int((e - s).sum()) + int((~inside).sum()) == tb
        assert (conf[b, :l] > 0).all() and (conf[b, :l] <= 1.0 + 1e-6).all()


# ---- 3. against float64 ----------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _f64_case(name):
    if name == "peaked":
        lp, tgt, Tb, L = _case(8, 1000, 4, 500, 100, peaked=True)
    else:
        lp, tgt, Tb, L = inputs(name)
    rg, _ = posteriors_blank(np_(lp), np_(tgt), np_(Tb), np_(L), 0)
    return (lp, tgt, Tb, L), rg


@pytest.mark.parametrize("name", ["S20r", "peaked", "S300"])
def test_against_float64(dev, name):
    """frame_conf within the posteriors' own bound of the float64 gamma at the path (2e-5 for T <= 256, 5e-4 above);
    conf within that bound plus (n + 1) 2^-24 of the float64 mean: a sequential float32 sum of n values <= 1 rounds n - 1
    times at no more than 2^-24 n each before the division by n, and the division rounds once"""
    (lp, tgt, Tb, L), rg = _f64_case(name)
    out = _spans(dev, lp, tgt, Tb, L)
    path, fc = np_(out.path), np_(out.frame_conf).astype(np.float64)
    start, end, conf = np_(out.start), np_(out.end), np_(out.conf).astype(np.float64)
    T = lp.shape[0]
    bound = 2e-5 if T <= 256 else 5e-4
    ref = np.take_along_axis(rg, np.maximum(path, 0)[:, :, None].astype(np.int64), 2)[:, :, 0]
    ref[path < 0] = 0.0
    dfc = np.abs(fc - ref).max()
    dconf, slack, nspans = 0.0, 0.0, 0
    for b in range(tgt.shape[0]):
        for j in range(tgt.shape[1]):
            if start[b, j] < 0:
                continue
            n = int(end[b, j] - start[b, j])
            d = abs(conf[b, j] - ref[b, start[b, j]:end[b, j]].mean())
            dconf, nspans = max(dconf, d), nspans + 1
            slack = max(slack, d - (bound + (n + 1) * 2.0 ** -24))
    print("%s: max|dframe_conf| %.3g, max|dconf| %.3g over %d spans (bound %.0e + (n+1) 2^-24, worst excess %.3g)"
          % (name, dfc, dconf, nspans, bound, slack))
    assert nspans > 0
    assert dfc <= bound
    assert slack <= 0.0


# ---- 4. input forms ------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["S20", "S300"])
def test_blank_last_class(dev, name):
    if name == "S20":
        lp, tgt, Tb, L = _case(3, 150, 8, 158, 20, ragged=True, blank=157)
    else:
        lp, _, Tb, L = inputs(name)
        tgt = torch.randint(0, lp.shape[2] - 1, tuple(inputs(name)[1].shape), generator=torch.Generator().manual_seed(4))
    C = lp.shape[2]
    assert int(tgt.max()) < C - 1
    out = _spans(dev, lp, tgt, Tb, L, blank=C - 1)
    _composition(dev, out, lp, tgt, Tb, L, blank=C - 1)
    assert np.isfinite(np_(out.score)).any()
    # the same values with classes 0 and C - 1 exchanged and blank = 0: the same seven outputs
    lp0, tgt0 = lp.clone(), tgt.clone()
    lp0[:, :, 0], lp0[:, :, C - 1] = lp[:, :, C - 1], lp[:, :, 0]
    tgt0[tgt == 0] = C - 1
    _same(out, _spans(dev, lp0, tgt0, Tb, L, blank=0), "blank = C - 1")


@pytest.mark.parametrize("name", ["S20r", "S300"])
def test_int32_targets(dev, name):
    lp, tgt, Tb, L = inputs(name)
    _same(_spans(dev, lp, tgt.int(), Tb, L), _spans(dev, lp, tgt, Tb, L), "int32 targets")


@pytest.mark.parametrize("name", ["S20r", "S300"])
def test_strided_log_probs(dev, name):
    """every second sample of a batch twice as large, as a view"""
    lp, tgt, Tb, L = inputs(name)
    T, B, C = lp.shape
    wide = torch.randn(T, 2 * B, C, generator=torch.Generator().manual_seed(23)).log_softmax(2)
    wide[:, ::2] = lp
    x = wide.to(dev)[:, ::2]
    assert x.stride(1) == 2 * C and not x.is_contiguous()
    _same(_spans(dev, None, tgt, Tb, L, lpd=x), _spans(dev, lp, tgt, Tb, L), "strided")


def test_masked_classes(dev):
    lp, tgt, Tb, L = _case(7, 150, 16, 158, 20, ragged=True, masked=True)
    assert bool(torch.isinf(lp).any())
    out = _spans(dev, lp, tgt, Tb, L)
    _composition(dev, out, lp, tgt, Tb, L)


# ---- 5. shared workspace ---------------------------------------------------------------------------------

def _loss_outputs(dev, lp, tgt, Tb, L):
    import ctc_amd
    x = lp.to(dev).requires_grad_(True)
    loss, nll = ctc_amd.blank_ctc_loss(x, tgt.to(dev), Tb.to(dev), L.to(dev))
    loss.backward()
    torch.cuda.synchronize()
    return [t.detach().clone() for t in (loss, nll, x.grad)]


@pytest.mark.parametrize("name", ["persistent", "S300"])
def test_shared_workspace_leaves_the_loss_alone(dev, name):
    """the loss, then the token spans, then the loss again on ONE stream's workspace: the two loss results are bitwise
    equal and no status bit is set"""
    import ctc_amd
    if name == "persistent":
        lp, tgt, Tb, L = synth_blank(5, 260, 32, 512, 100, var_T=True)
        ctc_amd.set_blank_schedule(1)
    else:
        lp, tgt, Tb, L = inputs(name)
    try:
        first = _loss_outputs(dev, lp, tgt, Tb, L)
        out = _spans(dev, lp, tgt, Tb, L)
        second = _loss_outputs(dev, lp, tgt, Tb, L)
    finally:
        ctc_amd.set_blank_schedule(-1)
    for a, b in zip(first, second):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert ctc_amd.workspace_status() == 0
    _composition(dev, out, lp, tgt, Tb, L)


# ---- 6. determinism and graph capture -------------------------------------------------------------------

@pytest.mark.parametrize("name", ["S40r", "S300"])
def test_deterministic_and_graph_capturable(dev, name):
    import ctc_amd
    lp, tgt, Tb, L = _case(10, 300, 8, 200, 40, ragged=True) if name == "S40r" else inputs(name)
    T, B, C = lp.shape
    lpd, tgd, Tbd, Ld = lp.to(dev), tgt.to(dev), Tb.to(dev), L.to(dev)
    a = ctc_amd.blank_token_spans(lpd, tgd, Tbd, Ld)
    b = ctc_amd.blank_token_spans(lpd, tgd, Tbd, Ld)
    torch.cuda.synchronize()
    _same(a, b, "eager twice")

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                # warm-up on the capture stream (its workspace)
        ctc_amd.blank_token_spans(lpd, tgd, Tbd, Ld)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):                       # one straight line of launches
        captured = ctc_amd.blank_token_spans(lpd, tgd, Tbd, Ld)
    for seed in (12, 13):
        lp2, _, _, _ = synth_blank(seed, T, B, C, tgt.shape[1])
        with torch.no_grad():
            lpd.copy_(lp2.to(dev))
        g.replay()
        torch.cuda.synchronize()
        eager = ctc_amd.blank_token_spans(lpd, tgd, Tbd, Ld)
        torch.cuda.synchronize()
        _same(captured, eager, "graph replay")
        assert bool((captured.start >= 0).any())
    assert ctc_amd.workspace_status() == 0


# ---- 7. errors ---------------------------------------------------------------------------------------------

def test_errors(dev):
    import ctc_amd
    lp, tgt, Tb, L = synth_blank(0, 8, 2, 6, 3)
    args = (tgt.to(dev), Tb.to(dev), L.to(dev))
    with pytest.raises(ctc_amd.CtcAmdError, match="1023"):
        ctc_amd.blank_token_spans(lp.to(dev), torch.ones(2, 1024, dtype=torch.int64, device=dev), args[1], args[2])
    with pytest.raises(ValueError):
        ctc_amd.blank_token_spans(lp.to(dev).bfloat16(), *args)
    with pytest.raises(ValueError):
        ctc_amd.blank_token_spans(lp.to(dev), tgt.float().to(dev), args[1], args[2])
