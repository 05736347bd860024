"""Blank-CTC per-frame state posteriors on the MI355X: accuracy against the float64 restatement of
tests/test_blank_posteriors_abi.py (gamma, nll, exact zeros, row sums), the input variants, consistency with the blank
loss and torch's float64 gradient, a workspace shared with the loss and the best path, determinism and graph capture."""
import numpy as np
import pytest
import torch

from tests.helpers import np_, synth_blank
from tests.test_blank_posteriors_abi import class_occupancy, posteriors_blank

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    import ctc_amd  # noqa: F401  (raises if libctc_amd.so is missing)
    return torch.device("cuda:0")


def _case(seed, T, B, C, S, ragged=False, blank=0, peaked=False, masked=False):
    """synth_blank inputs; ragged: varied T_b, some L_b = 0, adjacent repeats, some samples one step too short"""
    lp, tgt, Tb, L = synth_blank(seed, T, B, C, S, var_T=ragged)
    g = torch.Generator().manual_seed(seed + 1)
    if blank != 0:
        tgt = torch.randint(0, C - 1, (B, S), generator=g)
        tgt[tgt >= blank] += 1
    if peaked:
        lp = (30.0 * torch.randn(T, B, C, generator=g)).log_softmax(2)
    if masked:                                                   # a class no frame may emit, and holes in the blank
        lp[:, :, int(tgt[0, 0])] = -float("inf")
        lp[::7, :, blank] = -float("inf")
    if ragged:
        Tb = torch.randint(1, T + 1, (B,), generator=g)
        L[::5] = 0
        if S > 1:
            tgt[1::4, 1] = tgt[1::4, 0]                          # adjacent repeats
        short = torch.arange(B) % 3 == 2
        L[short] = torch.clamp(L[short], min=min(2, S))
        Tb[short] = torch.clamp(L[short] - 1, min=1)             # one step fewer than the labels: no alignment
        Tb[0] = T
    return lp, tgt, Tb.long(), L.long()


def _run(dev, lp, tgt, Tb, L, blank=0, lpd=None):
    import ctc_amd
    lpd = lp.to(dev) if lpd is None else lpd
    gamma, nll = ctc_amd.blank_posteriors(lpd, tgt.to(dev), Tb.to(dev), L.to(dev), blank=blank)
    torch.cuda.synchronize()
    return np_(gamma), np_(nll)


def _check(gamma, nll, lp, tgt, Tb, L, blank=0, label=""):
    """the bounds of the contract against the float64 restatement on the same fp32 inputs -> (ref gamma, ref nll)"""
    rg, rn = posteriors_blank(np_(lp), np_(tgt), np_(Tb), np_(L), blank)
    T = gamma.shape[1]
    Tb, L = np_(Tb), np_(L)
    assert gamma.shape == rg.shape and gamma.dtype == np.float32
    assert np.array_equal(np.isinf(nll), np.isinf(rn)) and not np.isnan(nll).any()
    fin = np.isfinite(rn)
    dn = np.abs(nll[fin].astype(np.float64) - rn[fin])
    assert (dn <= 1e-5 * np.maximum(1.0, np.abs(rn[fin]))).all(), dn.max()
    dg = np.abs(gamma - rg).max()
    bound = 2e-5 if T <= 256 else 5e-4
    print("%s max|dgamma| %.3g (bound %.0e)  max|dnll| %.3g" % (label, dg, bound, dn.max() if dn.size else 0.0))
    assert dg <= bound
    assert (gamma[rg == 0] == 0).all(), "non-zero gamma where no path passes / outside the support"
    for b in np.nonzero(fin)[0]:
        np.testing.assert_allclose(gamma[b, :Tb[b]].sum(1), 1.0, atol=1e-5)
        if L[b] == 0:
            assert (gamma[b, :Tb[b], 0] == 1.0).all()
    return rg, rn


@pytest.mark.parametrize("shape,ragged", [
    ((1, 3, 5, 1), False),
    ((150, 16, 158, 20), True),
    ((300, 6, 400, 60), True),                                    # K = 2
    ((300, 6, 400, 100), False),                                  # K = 4
    ((300, 4, 600, 255), False),                                  # K = 8
    ((40, 5, 600, 255), True),
])
def test_accuracy(dev, shape, ragged):
    T, B, C, S = shape
    lp, tgt, Tb, L = _case(21, T, B, C, S, ragged)
    gamma, nll = _run(dev, lp, tgt, Tb, L)
    _check(gamma, nll, lp, tgt, Tb, L, label=str(shape))
    if ragged and B > 3:
        assert np.isinf(nll).any() and np.isfinite(nll).any() and (np_(L) == 0).any()


def test_accuracy_config5(dev):
    T, B, C, S = 2000, 64, 1000, 100                              # BASELINE config 5, every sample checked
    lp, tgt, Tb, L = _case(5, T, B, C, S)
    gamma, nll = _run(dev, lp, tgt, Tb, L)
    _check(gamma, nll, lp, tgt, Tb, L, label="config 5")


@pytest.mark.parametrize("T,B,C,S", [(150, 8, 158, 20), (300, 4, 600, 100)])
def test_blank_last_class(dev, T, B, C, S):
    lp, tgt, Tb, L = _case(3, T, B, C, S, ragged=True, blank=C - 1)
    gamma, nll = _run(dev, lp, tgt, Tb, L, blank=C - 1)
    _check(gamma, nll, lp, tgt, Tb, L, blank=C - 1, label="blank=C-1")


def test_int32_targets(dev):
    lp, tgt, Tb, L = _case(4, 150, 16, 158, 20, ragged=True)
    gamma, nll = _run(dev, lp, tgt.int(), Tb, L)
    _check(gamma, nll, lp, tgt, Tb, L, label="int32")


def test_strided_log_probs(dev):
    lp, tgt, Tb, L = _case(6, 150, 32, 158, 20, ragged=True)
    lpd = lp.to(dev)[:, ::2]
    assert not lpd.is_contiguous()
    gamma, nll = _run(dev, None, tgt[::2], Tb[::2], L[::2], lpd=lpd)
    _check(gamma, nll, lp[:, ::2], tgt[::2], Tb[::2], L[::2], label="strided")


@pytest.mark.parametrize("T,B,C,S", [(150, 16, 158, 20), (600, 4, 300, 100)])
def test_masked_classes(dev, T, B, C, S):
    lp, tgt, Tb, L = _case(7, T, B, C, S, ragged=True, masked=True)
    gamma, nll = _run(dev, lp, tgt, Tb, L)
    _check(gamma, nll, lp, tgt, Tb, L, label="-inf entries")


@pytest.mark.parametrize("T,B,C,S", [(150, 16, 158, 20), (1000, 4, 500, 100)])
def test_peaked_inputs(dev, T, B, C, S):
    lp, tgt, Tb, L = _case(8, T, B, C, S, ragged=True, peaked=True)
    gamma, nll = _run(dev, lp, tgt, Tb, L)
    _check(gamma, nll, lp, tgt, Tb, L, label="peaked")


def test_consistent_with_the_loss_and_torch(dev):
    import ctc_amd
    T, B, C, S = 150, 16, 158, 20
    lp, tgt, Tb, L = _case(9, T, B, C, S, ragged=True)
    gamma, nll = _run(dev, lp, tgt, Tb, L)
    _, lnll = ctc_amd.blank_ctc_loss(lp.to(dev), tgt.to(dev), Tb.to(dev), L.to(dev))
    lnll = np_(lnll)
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
        assert d <= 2e-5, (b, d)


def _loss_outputs(dev, lp, tgt, Tb, L):
    import ctc_amd
    x = lp.to(dev).requires_grad_(True)
    loss, nll = ctc_amd.blank_ctc_loss(x, tgt.to(dev), Tb.to(dev), L.to(dev))
    loss.backward()
    torch.cuda.synchronize()
    return [t.detach().clone() for t in (loss, nll, x.grad)]


@pytest.mark.parametrize("between", ["posteriors", "best_path"])
def test_shared_workspace_leaves_the_loss_alone(dev, between):
    """persistent loss, then the posteriors (or the best path, then the posteriors), then the loss again on ONE stream's
    workspace: the two loss results are bitwise equal and no status bit is set"""
    import ctc_amd
    T, B, C, S = 260, 32, 512, 100
    lp, tgt, Tb, L = synth_blank(5, T, B, C, S, var_T=True)
    ctc_amd.set_blank_schedule(1)
    try:
        first = _loss_outputs(dev, lp, tgt, Tb, L)
        args = (lp.to(dev), tgt.to(dev), Tb.to(dev), L.to(dev))
        if between == "best_path":
            ctc_amd.blank_best_path(*args)
        gamma, nll = ctc_amd.blank_posteriors(*args)
        if between == "best_path":
            ctc_amd.blank_best_path(*args)
        second = _loss_outputs(dev, lp, tgt, Tb, L)
    finally:
        ctc_amd.set_blank_schedule(-1)
    for a, b in zip(first, second):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert ctc_amd.workspace_status() == 0
    _check(np_(gamma), np_(nll), lp, tgt, Tb, L, label="shared workspace")


def test_deterministic_and_graph_capturable(dev):
    import ctc_amd
    T, B, C, S = 300, 8, 200, 40
    lp, tgt, Tb, L = _case(10, T, B, C, S, ragged=True)
    lpd, tgd, Tbd, Ld = lp.to(dev), tgt.to(dev), Tb.to(dev), L.to(dev)
    g1, n1 = ctc_amd.blank_posteriors(lpd, tgd, Tbd, Ld)
    g2, n2 = ctc_amd.blank_posteriors(lpd, tgd, Tbd, Ld)
    torch.cuda.synchronize()
    assert torch.equal(g1.view(torch.int32), g2.view(torch.int32)) and torch.equal(n1.view(torch.int32), n2.view(torch.int32))

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                # warm-up on the capture stream (its workspace)
        ctc_amd.blank_posteriors(lpd, tgd, Tbd, Ld)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        gg, gn = ctc_amd.blank_posteriors(lpd, tgd, Tbd, Ld)
    for seed in (12, 13):
        lp2, _, _, _ = _case(seed, T, B, C, S)
        with torch.no_grad():
            lpd.copy_(lp2.to(dev))
        g.replay()
        torch.cuda.synchronize()
        eg, en = ctc_amd.blank_posteriors(lpd, tgd, Tbd, Ld)
        torch.cuda.synchronize()
        assert torch.equal(gg.view(torch.int32), eg.view(torch.int32))
        assert torch.equal(gn.view(torch.int32), en.view(torch.int32))
        _check(np_(gg), np_(gn), lp2, tgt, Tb, L, label="graph replay")
    assert ctc_amd.workspace_status() == 0


def test_confidence_at_the_best_path(dev):
    """gamma at the best path's states: a probability, 1 where the alignment is forced"""
    import ctc_amd
    lp, tgt, Tb, L = _case(11, 150, 16, 158, 20, ragged=True)
    args = (lp.to(dev), tgt.to(dev), Tb.to(dev), L.to(dev))
    path, _ = ctc_amd.blank_best_path(*args)
    gamma, nll = ctc_amd.blank_posteriors(*args)
    ok = path >= 0
    conf = torch.gather(gamma, 2, path.clamp(min=0).long().unsqueeze(2)).squeeze(2)
    assert bool(((conf > 0) & (conf <= 1.0 + 1e-6))[ok].all())
    assert bool((ok.any(1) == torch.isfinite(nll)).all())
