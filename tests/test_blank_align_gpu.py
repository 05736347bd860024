"""Blank-CTC best path on the MI355X: exact path and bitwise score parity with the float32 restatement of
tests/test_blank_align_abi.py, the input variants, ties, consistency with the blank loss, the forced-alignment
read-out, determinism and graph capture."""
import numpy as np
import pytest
import torch

from tests.helpers import np_, synth_blank
from tests.test_blank_align_abi import tokens_of, viterbi_blank

pytestmark = pytest.mark.gpu

# Back-pointers stay in LDS up to this many steps at 65..128 extended states (K = 4 states per lane: 4 steps per
# 32-bit word per lane, 507 word rows beside the 64-row emission ring); longer samples spill the rest to the workspace.
LDS_STEPS_K4 = 2028


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    import ctc_amd  # noqa: F401  (raises if libctc_amd.so is missing)
    return torch.device("cuda:0")


def _case(seed, T, B, C, S, ragged=False, blank=0):
    """synth_blank inputs; ragged: varied T_b, some L_b = 0, some samples too short for an alignment"""
    lp, tgt, Tb, L = synth_blank(seed, T, B, C, S, var_T=ragged)
    if blank == C - 1:
        g = torch.Generator().manual_seed(seed + 1)
        tgt = torch.randint(0, C - 1, (B, S), generator=g)
    if ragged:
        g = torch.Generator().manual_seed(seed + 2)
        Tb = torch.randint(1, T + 1, (B,), generator=g)
        L[::5] = 0
        tgt[1::4, 1] = tgt[1::4, 0]                             # adjacent repeats
        short = torch.arange(B) % 3 == 2
        L[short] = torch.clamp(L[short], min=min(2, S))
        Tb[short] = torch.clamp(L[short] - 1, min=1)            # one step fewer than the labels: no alignment
    return lp, tgt, Tb.long(), L.long()


def _run(dev, lp, tgt, Tb, L, blank=0, lpd=None):
    import ctc_amd
    lpd = lp.to(dev) if lpd is None else lpd
    path, score = ctc_amd.blank_best_path(lpd, tgt.to(dev), Tb.to(dev), L.to(dev), blank=blank)
    torch.cuda.synchronize()
    return np_(path), np_(score)


def _check(path, score, lp, tgt, Tb, L, blank=0):
    rp, rs = viterbi_blank(np_(lp), np_(tgt), np_(Tb), np_(L), blank)
    assert np.array_equal(score.view(np.int32), rs.view(np.int32)), \
        np.nonzero(score.view(np.int32) != rs.view(np.int32))
    bad = np.nonzero((path != rp).any(1))[0]
    assert bad.size == 0, "samples %s differ" % bad[:8]
    return rp, rs


@pytest.mark.parametrize("shape,ragged", [
    ((1, 3, 5, 1), False),
    ((50, 8, 20, 6), True),
    ((300, 16, 1000, 40), False),
    ((2000, 64, 1000, 100), False),                             # BASELINE config 5
    ((2000, 4, 600, 255), False),                               # largest S: back-pointers beyond 1020 steps spill
    ((LDS_STEPS_K4, 2, 300, 100), False),                       # the LDS threshold at K = 4: all in LDS ...
    ((LDS_STEPS_K4 + 1, 2, 300, 100), False),                   # ... one step beyond it: one word row spills
])
def test_exact_parity(dev, shape, ragged):
    T, B, C, S = shape
    lp, tgt, Tb, L = _case(11, T, B, C, S, ragged)
    path, score = _run(dev, lp, tgt, Tb, L)
    _check(path, score, lp, tgt, Tb, L)
    if ragged:
        assert (score == -np.inf).any() and np.isfinite(score).any() and (np_(L) == 0).any()


def test_masked_classes(dev):
    """-inf log-probs (tests/blank_grad_ref.py's mask): holes in the blank and in sample 0's first label, and samples
    with no alignment through their EMISSIONS alone -- path -1 and score -inf exactly where the loss has nll = +inf"""
    import ctc_amd
    from tests.blank_grad_ref import feasible_by_length, make_case
    lp, tgt, Tb, L = make_case("k2", "masked")
    path, score = _run(dev, lp, tgt, Tb, L)
    rp, rs = _check(path, score, lp, tgt, Tb, L)
    none = rs == -np.inf
    assert list(none) == [False, False, True, False, False, True] and feasible_by_length(tgt, Tb, L).all()
    assert (rp[none] == -1).all() and not np.isnan(rs).any()
    _, nll = ctc_amd.blank_ctc_loss(lp.to(dev), tgt.to(dev), Tb.to(dev), L.to(dev))
    assert np.array_equal(np_(nll) == np.inf, none)


@pytest.mark.parametrize("T,B,C,S", [(50, 8, 20, 6), (300, 6, 1000, 100)])
def test_blank_last_class(dev, T, B, C, S):
    lp, tgt, Tb, L = _case(3, T, B, C, S, ragged=T < 100, blank=C - 1)
    path, score = _run(dev, lp, tgt, Tb, L, blank=C - 1)
    _check(path, score, lp, tgt, Tb, L, blank=C - 1)


def test_int32_targets(dev):
    lp, tgt, Tb, L = _case(4, 120, 8, 50, 20, ragged=True)
    path, score = _run(dev, lp, tgt.int(), Tb, L)
    _check(path, score, lp, tgt, Tb, L)


def test_strided_log_probs(dev):
    T, B, C, S = 200, 6, 300, 30
    lp2, tgt, Tb, L = _case(5, T, 2 * B, C, S)
    x = lp2.to(dev)[:, ::2]                                      # [T,B,C] view, batch stride 2C
    tgt, Tb, L = tgt[::2].contiguous(), Tb[::2].contiguous(), L[::2].contiguous()
    path, score = _run(dev, None, tgt, Tb, L, lpd=x)
    _check(path, score, lp2[:, ::2], tgt, Tb, L)
    btc = lp2[:, :B].transpose(0, 1).contiguous()                # [B,T,C] storage, read as [T,B,C]
    path, score = _run(dev, None, tgt, Tb, L, lpd=btc.to(dev).transpose(0, 1))
    _check(path, score, lp2[:, :B], tgt, Tb, L)


@pytest.mark.parametrize("T,B,C,S", [(60, 8, 6, 10), (500, 4, 40, 100)])
def test_ties_quantised_inputs(dev, T, B, C, S):
    lp, tgt, Tb, L = _case(6, T, B, C, S, ragged=T < 100)
    lp = torch.clamp(torch.round(lp * 2) / 2, min=-6.0)         # multiples of 0.5: exact sums, ties everywhere
    tgt = tgt % 3 + 1                                            # few classes: many repeats
    path, score = _run(dev, lp, tgt, Tb, L)
    _check(path, score, lp, tgt, Tb, L)


@pytest.mark.parametrize("T,B,C,S,ragged", [(50, 8, 20, 6, True), (400, 8, 200, 40, False)])
def test_consistent_with_the_loss(dev, T, B, C, S, ragged):
    import ctc_amd
    lp, tgt, Tb, L = _case(7, T, B, C, S, ragged)
    _, score = _run(dev, lp, tgt, Tb, L)
    _, nll = ctc_amd.blank_ctc_loss(lp.to(dev), tgt.to(dev), Tb.to(dev), L.to(dev))
    nll = np_(nll).astype(np.float64)
    assert np.array_equal(score == -np.inf, nll == np.inf)
    fin = np.isfinite(nll)
    assert (score[fin] <= -nll[fin] + 1e-4 * np.abs(nll[fin])).all()


@pytest.mark.parametrize("T,B,C,S,blank", [(50, 8, 20, 6, 0), (300, 8, 100, 40, 99)])
def test_forced_align_is_well_formed(dev, T, B, C, S, blank):
    import ctc_amd
    lp, tgt, Tb, L = _case(8, T, B, C, S, ragged=True, blank=blank)
    lpd = lp.to(dev)
    path, score = _run(dev, lp, tgt, Tb, L, blank=blank)
    tok, fs = ctc_amd.blank_forced_align(lpd, tgt.to(dev), Tb.to(dev), L.to(dev), blank=blank)
    tok, fs = np_(tok), np_(fs)
    lpn, tgn = np_(lp), np_(tgt)
    assert np.array_equal(tok, tokens_of(path, tgn, blank))
    for b in range(B):
        tb, lb = int(Tb[b]), int(L[b])
        assert (path[b, tb:] == -1).all() and (tok[b, tb:] == -1).all() and (fs[b, tb:] == 0).all()
        if score[b] == -np.inf:
            assert (path[b] == -1).all() and (fs[b] == 0).all()
            continue
        p = path[b, :tb]
        assert p[0] in (0, 1)
        assert p[-1] in ((2 * lb - 1, 2 * lb) if lb else (0,))
        d = np.diff(p)
        assert ((d >= 0) & (d <= 2)).all()
        for t in np.nonzero(d == 2)[0]:
            s = p[t + 1]
            assert s % 2 == 1 and tgn[b, (s - 1) // 2] != blank and tgn[b, (s - 1) // 2] != tgn[b, (s - 3) // 2]
        acc = np.float32(0)
        for t in range(tb):
            assert fs[b, t] == lpn[t, b, tok[b, t]]
            acc = np.float32(acc + fs[b, t])
        assert acc.view(np.int32) == score[b].view(np.int32)


def test_deterministic_and_graph_capturable(dev):
    import ctc_amd
    T, B, C, S = 300, 8, 200, 40
    lp, tgt, Tb, L = _case(9, T, B, C, S)
    lpd, tgd, Tbd, Ld = lp.to(dev), tgt.to(dev), Tb.to(dev), L.to(dev)
    before = [t.clone() for t in (lpd, tgd, Tbd, Ld)]
    p1, s1 = ctc_amd.blank_best_path(lpd, tgd, Tbd, Ld)
    p2, s2 = ctc_amd.blank_best_path(lpd, tgd, Tbd, Ld)
    torch.cuda.synchronize()
    assert torch.equal(p1, p2) and torch.equal(s1.view(torch.int32), s2.view(torch.int32))
    for a, b in zip(before, (lpd, tgd, Tbd, Ld)):
        assert torch.equal(a, b)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                # warm-up on the capture stream (its workspace)
        ctc_amd.blank_best_path(lpd, tgd, Tbd, Ld)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        gp, gs = ctc_amd.blank_best_path(lpd, tgd, Tbd, Ld)
    for seed in (12, 13):
        lp2, _, _, _ = _case(seed, T, B, C, S)
        with torch.no_grad():
            lpd.copy_(lp2.to(dev))
        g.replay()
        torch.cuda.synchronize()
        ep, es = ctc_amd.blank_best_path(lpd, tgd, Tbd, Ld)
        torch.cuda.synchronize()
        assert torch.equal(gp, ep) and torch.equal(gs.view(torch.int32), es.view(torch.int32))
        _check(np_(gp), np_(gs), lp2, tgt, Tb, L)
    assert ctc_amd.workspace_status() == 0
