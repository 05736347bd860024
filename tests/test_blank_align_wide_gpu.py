"""Blank-CTC best path on the wide lattice (256 <= S <= 1023 labels, ctc_amd_blank_best_path_wide) on the MI355X: exact
path and bitwise score parity with the float32 restatement of tests/test_blank_align_abi.py -- the comparison is exact,
so there is no tolerance.  Inputs are the cases of tests/test_blank_wide_gpu.py (their repeats put a forced blank on the
256-, 512-, 1024- and 1536-state seams) plus final states on the first state of a wave, ties, the input forms, the
forced-alignment read-out, the loss on the same workspace, determinism and graph capture."""
import functools

import numpy as np
import pytest
import torch

from tests.helpers import np_, synth_blank
from tests.test_blank_align_abi import tokens_of, viterbi_blank
from tests.test_blank_wide_gpu import CASES, make_case, run_loss

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    import ctc_amd  # noqa: F401  (raises if libctc_amd.so is missing)
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def reference(name):
    """computed once per case and shared (read-only): inputs, the restatement's path and score"""
    inputs = make_case(name)
    lp, tgt, Tb, L = inputs
    rp, rs = viterbi_blank(np_(lp), np_(tgt), np_(Tb), np_(L), 0)
    return inputs, rp, rs


def _run(dev, lp, tgt, Tb, L, blank=0, lpd=None):
    import ctc_amd
    lpd = lp.to(dev) if lpd is None else lpd
    path, score = ctc_amd.blank_best_path(lpd, tgt.to(dev), Tb.to(dev), L.to(dev), blank=blank)
    torch.cuda.synchronize()
    return np_(path), np_(score)


def _same(path, score, rp, rs):
    assert np.array_equal(score.view(np.int32), rs.view(np.int32)), \
        np.nonzero(score.view(np.int32) != rs.view(np.int32))
    bad = np.nonzero((path != rp).any(1))[0]
    assert bad.size == 0, "samples %s differ" % bad[:8]


def _check(path, score, lp, tgt, Tb, L, blank=0):
    rp, rs = viterbi_blank(np_(lp), np_(tgt), np_(Tb), np_(L), blank)
    _same(path, score, rp, rs)
    return rp, rs


@pytest.mark.parametrize("name", list(CASES))
def test_exact_parity(dev, name):
    (lp, tgt, Tb, L), rp, rs = reference(name)
    if name == "ragged":
        # sample 3: nine labels in five frames; sample 4: no labels
        assert list(np.isfinite(rs)) == [True, True, True, False, True, True]
        assert (rp[3] == -1).all() and (rp[4, :30] == 0).all() and (rp[4, 30:] == -1).all()
    else:
        assert np.isfinite(rs).all()
    path, score = _run(dev, lp, tgt, Tb, L)
    _same(path, score, rp, rs)


@pytest.mark.parametrize("form", ["as_they_are", "last_blank_raised", "last_label_lowered"])
def test_final_state_at_a_wave_seam(dev, form):
    """2L = 1536 and 1024 are the first state of a wave, 2L - 1 the last state of the wave below; L = 769: both in one
    wave, one lane apart from the seam; L = 800, T_b = T - 1.

    last_blank_raised: lp[T_b - 1, b, blank] = 0 for samples 0 and 2.  Sample 0 then ends in 2L = 1536 (it does so as
    it is, too).  Sample 2 does not: with 512 labels and 21 adjacent repeats in 600 frames its last label is best
    entered at the last frame, and the restatement ends in 2L - 1 = 1023 whatever the last blank costs.
    last_label_lowered: the same, and the last label of sample 2 at -40 in its last frame, so that the restatement ends
    in 1024 there as well.  The final states are asserted on the restatement: a test that misses the seam shows nothing."""
    T, B, C, S = 900, 4, 24, 800
    lp, tgt, _, _ = synth_blank(T + B + C + S, T, B, C, S)
    L = torch.tensor([768, 769, 512, 800])
    Tb = torch.tensor([900, 900, 600, 899])
    if form != "as_they_are":
        for b in (0, 2):
            lp[int(Tb[b]) - 1, b, 0] = 0.0
    if form == "last_label_lowered":
        lp[599, 2, tgt[2, 511]] = -40.0
    path, score = _run(dev, lp, tgt, Tb, L)
    rp, rs = _check(path, score, lp, tgt, Tb, L)
    assert np.isfinite(rs).all()
    if form != "as_they_are":
        assert rp[0, 899] == 1536
    if form == "last_label_lowered":
        assert rp[2, 599] == 1024
    else:
        assert rp[2, 599] == 1023


def test_masked_classes(dev):
    """-inf log-probs (tests/blank_grad_ref.py's mask): holes in the blank and in sample 0's first label, and a sample
    with no alignment through its EMISSIONS alone -- path -1 and score -inf exactly where the loss has nll = +inf"""
    from tests.blank_grad_ref import feasible_by_length, make_case
    lp, tgt, Tb, L = make_case("w2", "masked")
    path, score = _run(dev, lp, tgt, Tb, L)
    rp, rs = _check(path, score, lp, tgt, Tb, L)
    none = rs == -np.inf
    assert list(none) == [False, False, True] and feasible_by_length(tgt, Tb, L).all()
    assert (rp[none] == -1).all() and not np.isnan(rs).any()
    nll = run_loss(dev, lp, tgt, Tb, L, grad=False)["nll"]
    assert np.array_equal(np_(nll) == np.inf, none)


def test_ties_quantised_inputs(dev):
    T, B, C, S = 700, 2, 12, 300
    lp, tgt, Tb, _ = synth_blank(6, T, B, C, S)
    lp = torch.clamp(torch.round(lp * 2) / 2, min=-6.0)           # multiples of 0.5: exact sums, ties everywhere
    tgt = tgt % 3 + 1                                             # few classes: many adjacent repeats
    L = torch.tensor([300, 260])
    path, score = _run(dev, lp, tgt, Tb, L)
    _, rs = _check(path, score, lp, tgt, Tb, L)
    assert np.isfinite(rs).all()


def test_blank_last_class(dev):
    T, B, C, S = 400, 3, 40, 300
    lp, _, Tb, _ = synth_blank(21, T, B, C, S)
    tgt = torch.randint(0, C - 1, (B, S), generator=torch.Generator().manual_seed(22))
    L = torch.tensor([300, 299, 57])
    path, score = _run(dev, lp, tgt, Tb, L, blank=C - 1)
    _, rs = _check(path, score, lp, tgt, Tb, L, blank=C - 1)
    assert np.isfinite(rs).all()


def test_int32_targets(dev):
    (lp, tgt, Tb, L), rp, rs = reference("S300")
    path, score = _run(dev, lp, tgt.int(), Tb, L)
    _same(path, score, rp, rs)


def test_strided_log_probs(dev):
    T, B, C, S = 400, 3, 40, 300
    lp2, tgt2, Tb2, _ = synth_blank(23, T, 2 * B, C, S)
    x = lp2.to(dev)[:, ::2]                                       # [T,B,C] view, batch stride 2C
    assert x.stride(1) == 2 * C
    tgt, Tb = tgt2[::2].contiguous(), Tb2[::2].contiguous()
    L = torch.tensor([300, 256, 120])
    path, score = _run(dev, None, tgt, Tb, L, lpd=x)
    _check(path, score, lp2[:, ::2], tgt, Tb, L)


def test_forced_align(dev):
    import ctc_amd
    (lp, tgt, Tb, L), rp, rs = reference("S300")
    tok, fs = ctc_amd.blank_forced_align(lp.to(dev), tgt.to(dev), Tb.to(dev), L.to(dev))
    tok, fs = np_(tok), np_(fs)
    lpn = np_(lp)
    assert np.array_equal(tok, tokens_of(rp, np_(tgt), 0))
    for b in range(lp.shape[1]):
        tb = int(Tb[b])
        assert (tok[b, tb:] == -1).all() and (fs[b, tb:] == 0).all()
        acc = np.float32(0)
        for t in range(tb):
            assert fs[b, t] == lpn[t, b, tok[b, t]]
            acc = np.float32(acc + fs[b, t])
        assert acc.view(np.int32) == rs[b].view(np.int32)


def test_forced_align_beyond_the_input_length(dev):
    import ctc_amd
    (lp, tgt, Tb, L), rp, _ = reference("ragged")
    tok, fs = ctc_amd.blank_forced_align(lp.to(dev), tgt.to(dev), Tb.to(dev), L.to(dev))
    tok, fs = np_(tok), np_(fs)
    assert np.array_equal(tok, tokens_of(rp, np_(tgt), 0))
    for b in range(lp.shape[1]):
        assert (tok[b, int(Tb[b]):] == -1).all() and (fs[b, int(Tb[b]):] == 0).all()
    assert (tok[3] == -1).all() and (fs[3] == 0).all()           # no alignment


def test_the_loss_after_the_best_path(dev):
    """the loss, the wide best path, the loss again on ONE stream's workspace: the two loss results are bitwise equal"""
    import ctc_amd
    (lp, tgt, Tb, L), rp, rs = reference("S300")
    first = run_loss(dev, lp, tgt, Tb, L)
    path, score = _run(dev, lp, tgt, Tb, L)
    second = run_loss(dev, lp, tgt, Tb, L)
    for k in ("loss", "nll", "grad"):
        assert torch.equal(first[k].view(torch.int32), second[k].view(torch.int32)), k
    assert bool(torch.isfinite(first["nll"]).all())
    _same(path, score, rp, rs)
    assert ctc_amd.workspace_status() == 0


def test_deterministic_and_graph_capturable(dev):
    import ctc_amd
    (lp, tgt, Tb, L), _, _ = reference("S300")
    T, B, C = lp.shape
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
    with torch.cuda.graph(g, stream=side):                       # a single chain of two launches
        gp, gs = ctc_amd.blank_best_path(lpd, tgd, Tbd, Ld)
    lp2, _, _, _ = synth_blank(12, T, B, C, tgt.shape[1])
    with torch.no_grad():
        lpd.copy_(lp2.to(dev))
    g.replay()
    torch.cuda.synchronize()
    ep, es = ctc_amd.blank_best_path(lpd, tgd, Tbd, Ld)
    torch.cuda.synchronize()
    assert torch.equal(gp, ep) and torch.equal(gs.view(torch.int32), es.view(torch.int32))
    _check(np_(gp), np_(gs), lp2, tgt, Tb, L)
    assert ctc_amd.workspace_status() == 0


def test_too_many_labels_raises(dev):
    import ctc_amd
    lp, tgt, Tb, L = synth_blank(3, 40, 2, 8, 1024)
    L = torch.tensor([5, 7])
    with pytest.raises(ctc_amd.CtcAmdError, match="1023"):
        ctc_amd.blank_best_path(lp.to(dev), tgt.to(dev), Tb.to(dev), L.to(dev))
    with pytest.raises(ctc_amd.CtcAmdError, match="1023"):
        ctc_amd.blank_forced_align(lp.to(dev), tgt.to(dev), Tb.to(dev), L.to(dev))
