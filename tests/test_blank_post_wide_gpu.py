"""Blank-CTC per-frame state posteriors on the wide lattice (256 <= S <= 1023 labels, ctc_amd_blank_posteriors_wide) on
the MI355X, against the float64 restatement of tests/test_blank_posteriors_abi.py on the same fp32 inputs.  The contract
is the narrow one, unchanged: `_check` of tests/test_blank_posteriors_gpu.py (gamma within 5e-4 at T > 256, nll within
1e-5 relative, exact zeros where the restatement has zeros, rows summing to 1 within 1e-5, gamma[:, :, 0] == 1 where
L_b = 0); it prints max |dgamma| and max |dnll| before it asserts.  Inputs are the cases of tests/test_blank_wide_gpu.py
(their repeats put a forced blank on the 256-, 512-, 1024- and 1536-state seams, and gamma mass straddles every seam),
final and entry states split over two waves, the input forms, the loss and torch's float64 gradient, the loss and the
wide best path on the same workspace, determinism and graph capture."""
import functools

import numpy as np
import pytest
import torch

from tests.helpers import np_, synth_blank
from tests.test_blank_posteriors_abi import class_occupancy, posteriors_blank
from tests.test_blank_posteriors_gpu import _check
from tests.test_blank_wide_gpu import CASES, make_case, run_loss

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    import ctc_amd  # noqa: F401  (raises if libctc_amd.so is missing)
    return torch.device("cuda:0")


def _run(dev, lp, tgt, Tb, L, blank=0, lpd=None):
    import ctc_amd
    lpd = lp.to(dev) if lpd is None else lpd
    gamma, nll = ctc_amd.blank_posteriors(lpd, tgt.to(dev), Tb.to(dev), L.to(dev), blank=blank)
    torch.cuda.synchronize()
    return np_(gamma), np_(nll)


@functools.lru_cache(maxsize=None)
def case_gamma(dev, name):
    """computed once per case and shared (read-only): inputs and the library's (gamma, nll)"""
    inputs = make_case(name)
    return inputs, _run(dev, *inputs)


def _seam_frames(rg, b, seam):
    """frames of sample b with more than 1e-3 of the restatement's gamma on both sides of state `seam`"""
    return int(((rg[b, :, :seam].sum(1) > 1e-3) & (rg[b, :, seam:].sum(1) > 1e-3)).sum())


@pytest.mark.parametrize("name", list(CASES))
def test_accuracy(dev, name):
    (lp, tgt, Tb, L), (gamma, nll) = case_gamma(dev, name)
    rg, rn = _check(gamma, nll, lp, tgt, Tb, L, label=name)
    if name == "ragged":
        # sample 3: nine labels in five frames; sample 4: no labels
        assert list(np.isfinite(rn)) == [True, True, True, False, True, True]
    else:
        assert np.isfinite(rn).all()
    # a test whose gamma mass never crosses a wave seam shows nothing about the seams
    for seam in range(512, 2 * int(L.max()) + 1, 512):
        assert max(_seam_frames(rg, b, seam) for b in range(lp.shape[1])) >= 1, seam


@pytest.mark.parametrize("form", ["as_they_are", "last_blank_raised"])
def test_final_states_in_two_waves(dev, form):
    """2L = 1536 and 1024 are the first state of a wave, 2L - 1 the last state of the wave below (alpha's two final
    states and beta's two entry states); L = 769: both in one wave, one lane from the seam; L = 800, T_b = T - 1.
    last_blank_raised: lp[T_b - 1, b, blank] = 0 for samples 0 and 2.  Both final states of sample 0 carry more than
    0.05 of the last frame in both forms, asserted on the restatement."""
    T, B, C, S = 900, 4, 24, 800
    lp, tgt, _, _ = synth_blank(T + B + C + S, T, B, C, S)
    L = torch.tensor([768, 769, 512, 800])
    Tb = torch.tensor([900, 900, 600, 899])
    if form != "as_they_are":
        for b in (0, 2):
            lp[int(Tb[b]) - 1, b, 0] = 0.0
    gamma, nll = _run(dev, lp, tgt, Tb, L)
    rg, rn = _check(gamma, nll, lp, tgt, Tb, L, label="final states, " + form)
    assert np.isfinite(rn).all()
    print("sample 0, last frame: gamma(2L-1) %.3f, gamma(2L) %.3f" % (rg[0, 899, 1535], rg[0, 899, 1536]))
    assert rg[0, 899, 1535] > 0.05 and rg[0, 899, 1536] > 0.05


S300 = (400, 3, 40, 300)


def test_blank_last_class(dev):
    T, B, C, S = S300
    (lp, _, Tb, L), _ = case_gamma(dev, "S300")
    tgt = torch.randint(0, C - 1, (B, S), generator=torch.Generator().manual_seed(4))
    assert int(tgt.max()) < C - 1                                 # (no label is the blank: _case's remap moves nothing)
    gamma, nll = _run(dev, lp, tgt, Tb, L, blank=C - 1)
    _, rn = _check(gamma, nll, lp, tgt, Tb, L, blank=C - 1, label="S300 blank=C-1")
    assert np.isfinite(rn).all()


def test_int32_targets(dev):
    (lp, tgt, Tb, L), (g64, n64) = case_gamma(dev, "S300")
    gamma, nll = _run(dev, lp, tgt.int(), Tb, L)
    _check(gamma, nll, lp, tgt, Tb, L, label="S300 int32 targets")
    assert np.array_equal(gamma.view(np.int32), g64.view(np.int32)) and np.array_equal(nll.view(np.int32), n64.view(np.int32))


def test_strided_log_probs(dev):
    """every second sample of a batch of six"""
    (lp, tgt, Tb, L), _ = case_gamma(dev, "S300")
    T, B, C = lp.shape
    six = torch.randn(T, 2 * B, C, generator=torch.Generator().manual_seed(23))
    six[:, ::2] = lp
    x = six.to(dev)[:, ::2]                                       # [T,B,C] view, batch stride 2C
    assert x.stride(1) == 2 * C and not x.is_contiguous()
    gamma, nll = _run(dev, None, tgt, Tb, L, lpd=x)
    _check(gamma, nll, lp, tgt, Tb, L, label="S300 strided")


def test_masked_classes(dev):
    """holes in the blank and a class no fifth frame may emit: one sample without an alignment, exact zeros and
    non-zeros in the second wave of another (asserted on the restatement)"""
    (lp, tgt, Tb, L), _ = case_gamma(dev, "S300")
    lp = lp.clone()
    lp[::7, :, 0] = -float("inf")
    lp[::5, :, int(tgt[0, 0])] = -float("inf")
    gamma, nll = _run(dev, lp, tgt, Tb, L)
    rg, rn = _check(gamma, nll, lp, tgt, Tb, L, label="S300 -inf entries")
    assert list(np.isfinite(rn)) == [False, True, True]
    second = rg[1, :, 512:2 * int(L[1]) + 1]
    assert (second == 0).any() and (second > 0).any()


def test_peaked_inputs(dev):
    """log_softmax(30 randn): lp down to -217, most rows decided -- the case the per-frame maximum c_t exists for"""
    T, B, C, S = S300
    (_, tgt, Tb, L), _ = case_gamma(dev, "S300")
    lp = (30.0 * torch.randn(T, B, C, generator=torch.Generator().manual_seed(8))).log_softmax(2)
    gamma, nll = _run(dev, lp, tgt, Tb, L)
    rg, rn = _check(gamma, nll, lp, tgt, Tb, L, label="S300 peaked")
    assert np.isfinite(rn).all() and float(lp.min()) < -150
    assert (rg.max(2) > 0.99).mean() > 0.5


def test_consistent_with_the_loss_and_torch(dev):
    (lp, tgt, Tb, L), (gamma, nll) = case_gamma(dev, "ragged")
    C = lp.shape[2]
    lnll = np_(run_loss(dev, lp, tgt, Tb, L, grad=False)["nll"])
    assert np.array_equal(np.isinf(nll), np.isinf(lnll))
    fin = np.isfinite(lnll)
    assert (np.abs(nll[fin] - lnll[fin]) <= 2e-5 * np.abs(lnll[fin])).all()
    # class occupancies from gamma against torch's float64 CPU gradient (feasible samples, t < T_b)
    keep = torch.tensor(np.nonzero(fin)[0])
    x = lp[:, keep].double().requires_grad_(True)
    torch.nn.functional.ctc_loss(x, tgt[keep], Tb[keep], L[keep], reduction="sum", zero_infinity=False).backward()
    want = np.exp(np_(x)) - np_(x.grad)
    occ = class_occupancy(gamma[np_(keep)].astype(np.float64), np_(tgt[keep]), np_(Tb[keep]), np_(L[keep]), C)
    for i, b in enumerate(np_(keep)):
        d = np.abs(occ[:int(Tb[b]), i] - want[:int(Tb[b]), i]).max()
        print("sample %d: occupancy against torch float64 %.3g" % (b, d))
        assert d <= 2e-5, (b, d)


@pytest.mark.parametrize("between", ["posteriors", "best_path"])
def test_shared_workspace_leaves_the_loss_alone(dev, between):
    """the loss, then the wide posteriors (or the wide best path around them), then the loss again on ONE stream's
    workspace: the two loss results are bitwise equal and no status bit is set"""
    import ctc_amd
    (lp, tgt, Tb, L), _ = case_gamma(dev, "S300")
    first = run_loss(dev, lp, tgt, Tb, L)
    args = (lp.to(dev), tgt.to(dev), Tb.to(dev), L.to(dev))
    if between == "best_path":
        ctc_amd.blank_best_path(*args)
    gamma, nll = ctc_amd.blank_posteriors(*args)
    if between == "best_path":
        ctc_amd.blank_best_path(*args)
    second = run_loss(dev, lp, tgt, Tb, L)
    for k in ("loss", "nll", "grad"):
        assert torch.equal(first[k].view(torch.int32), second[k].view(torch.int32)), k
    assert ctc_amd.workspace_status() == 0
    _check(np_(gamma), np_(nll), lp, tgt, Tb, L, label="S300 shared workspace")


def test_deterministic_and_graph_capturable(dev):
    import ctc_amd
    (lp, tgt, Tb, L), _ = case_gamma(dev, "S300")
    T, B, C = lp.shape
    lpd, tgd, Tbd, Ld = lp.to(dev), tgt.to(dev), Tb.to(dev), L.to(dev)
    before = [t.clone() for t in (lpd, tgd, Tbd, Ld)]
    g1, n1 = ctc_amd.blank_posteriors(lpd, tgd, Tbd, Ld)
    g2, n2 = ctc_amd.blank_posteriors(lpd, tgd, Tbd, Ld)
    torch.cuda.synchronize()
    assert torch.equal(g1.view(torch.int32), g2.view(torch.int32)) and torch.equal(n1.view(torch.int32), n2.view(torch.int32))
    for a, b in zip(before, (lpd, tgd, Tbd, Ld)):
        assert torch.equal(a, b)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                # warm-up on the capture stream (its workspace)
        ctc_amd.blank_posteriors(lpd, tgd, Tbd, Ld)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):                       # a single chain of three launches
        gg, gn = ctc_amd.blank_posteriors(lpd, tgd, Tbd, Ld)
    for seed in (12, 13):
        lp2, _, _, _ = synth_blank(seed, T, B, C, tgt.shape[1])
        with torch.no_grad():
            lpd.copy_(lp2.to(dev))
        g.replay()
        torch.cuda.synchronize()
        eg, en = ctc_amd.blank_posteriors(lpd, tgd, Tbd, Ld)
        torch.cuda.synchronize()
        assert torch.equal(gg.view(torch.int32), eg.view(torch.int32))
        assert torch.equal(gn.view(torch.int32), en.view(torch.int32))
        _check(np_(gg), np_(gn), lp2, tgt, Tb, L, label="S300 graph replay")
    assert ctc_amd.workspace_status() == 0


def test_confidence_at_the_best_path(dev):
    """gamma at the wide best path's states: a probability"""
    import ctc_amd
    (lp, tgt, Tb, L), (gamma, nll) = case_gamma(dev, "ragged")
    path, _ = ctc_amd.blank_best_path(lp.to(dev), tgt.to(dev), Tb.to(dev), L.to(dev))
    path = np_(path).astype(np.int64)
    ok = path >= 0
    conf = np.take_along_axis(gamma, np.maximum(path, 0)[:, :, None], 2)[:, :, 0]
    assert ok.any() and ((conf > 0) & (conf <= 1.0 + 1e-6))[ok].all()
    assert np.array_equal(ok.any(1), np.isfinite(nll))


def test_too_many_labels_raises(dev):
    import ctc_amd
    lp, tgt, Tb, L = synth_blank(3, 40, 2, 8, 1024)
    L = torch.tensor([5, 7])
    with pytest.raises(ctc_amd.CtcAmdError, match="1023"):
        ctc_amd.blank_posteriors(lp.to(dev), tgt.to(dev), Tb.to(dev), L.to(dev))
    assert ctc_amd.workspace_status() == 0                        # (the last test of the file: nothing raised a bit)
