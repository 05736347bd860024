"""Blank-CTC per-frame state posteriors: the C ABI (declared, exported, bound, argument errors before any HIP call), the
missing CPU path, and a float64 numpy restatement of the contract, checked on lattices with known answers and against
torch's own float64 CTC gradient (runs without a GPU).  tests/test_blank_posteriors_gpu.py checks the kernels against
the same restatement."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "ctc_amd_blank_posteriors"
NINF = -np.inf


def posteriors_blank(lp, targets, in_len, tgt_len, blank=0):
    """float64 restatement of ctc_amd_blank_posteriors -> (gamma [B,T,2S+1] float64, nll [B] float64).

    alpha / beta' in natural log with -inf kept as -inf; gamma = exp(alpha + beta' + nll), exactly 0 outside the support,
    where no path passes, and on every row of a sample with no alignment (nll = +inf)."""
    lp = np.asarray(lp, dtype=np.float64)
    targets = np.asarray(targets)
    T, B, _ = lp.shape
    S = targets.shape[1]
    gamma = np.zeros((B, T, 2 * S + 1))
    nll = np.full(B, np.inf)
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(B):
            Tb, L = int(in_len[b]), int(tgt_len[b])
            n = 2 * L + 1
            ext = np.full(n, blank, dtype=np.int64)
            ext[1::2] = targets[b, :L]
            em = lp[:Tb, b, ext]                                        # [Tb, n]
            skip = np.zeros(n, dtype=bool)
            for s in range(3, n, 2):
                skip[s] = ext[s] != blank and ext[s] != ext[s - 2]
            skip_up = np.concatenate([skip[2:], [False, False]])[:n]    # beta: s from s+2 under the rule for s+2
            alpha = np.full((Tb, n), NINF)
            alpha[0, 0] = em[0, 0]
            if n > 1:
                alpha[0, 1] = em[0, 1]
            for t in range(1, Tb):
                prev = alpha[t - 1]
                adv = np.concatenate([[NINF], prev[:-1]])
                sk = np.where(skip, np.concatenate([[NINF, NINF], prev])[:n], NINF)
                alpha[t] = np.logaddexp(np.logaddexp(prev, adv), sk) + em[t]
            beta = np.full((Tb, n), NINF)
            beta[Tb - 1, n - 1] = 0.0
            if n > 1:
                beta[Tb - 1, n - 2] = 0.0
            for t in range(Tb - 2, -1, -1):
                nxt = beta[t + 1] + em[t + 1]
                adv = np.concatenate([nxt[1:], [NINF]])
                sk = np.where(skip_up, np.concatenate([nxt[2:], [NINF, NINF]])[:n], NINF)
                beta[t] = np.logaddexp(np.logaddexp(nxt, adv), sk)
            ll = np.logaddexp(alpha[Tb - 1, n - 1], alpha[Tb - 1, n - 2] if n > 1 else NINF)
            if not ll > NINF:
                continue
            nll[b] = -ll
            gamma[b, :Tb, :n] = np.exp(alpha + beta + nll[b])
    return gamma, nll


def class_occupancy(gamma, targets, in_len, tgt_len, C, blank=0):
    """[T,B,C]: sum over the states s with l'_s = c of gamma_t(s)"""
    B, T, _ = gamma.shape
    occ = np.zeros((T, B, C))
    for b in range(B):
        L = int(tgt_len[b])
        ext = np.full(2 * L + 1, blank, dtype=np.int64)
        ext[1::2] = np.asarray(targets)[b, :L]
        for s, c in enumerate(ext):
            occ[:, b, c] += gamma[b, :, s]
    return occ


def _one(rows, labels, blank=0, Tb=None):
    lp = np.asarray(rows, dtype=np.float64)[:, None, :]
    T = lp.shape[0]
    tg = np.asarray([list(labels) + [1]], dtype=np.int64)
    g, nll = posteriors_blank(lp, tg, [T if Tb is None else Tb], [len(labels)], blank)
    n = 2 * len(labels) + 1
    assert (g[0, :, n:] == 0).all()                          # the padding column's states
    return g[0, :, :n], nll[0]


def _rand_lp(rng, T, C):
    x = rng.standard_normal((T, C))
    return x - np.log(np.exp(x).sum(1, keepdims=True))


# ---- ABI ---------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    from ctc_amd import _lib, build
    build.build()
    return _lib.load()


def test_symbol_declared_exported_and_bound(lib):
    from ctc_amd import _lib
    header = open(os.path.join(ROOT, "include", "ctc_amd.h")).read()
    assert re.search(r"\b%s\s*\(" % NAME, header)
    assert hasattr(ctypes.CDLL(_lib.SO_PATH), NAME)
    res, args = _lib.PROTOTYPES[NAME]
    assert res is ctypes.c_int and len(args) == 16
    assert lib.ctc_amd_abi_version() == 2


def test_status_bit_named():
    from ctc_amd import functional
    assert functional.STATUS_BITS[16] == "blank-CTC posteriors"
    header = open(os.path.join(ROOT, "include", "ctc_amd.h")).read()
    assert "16 blank-CTC posteriors" in header


def test_python_export():
    import ctc_amd
    assert "blank_posteriors" in ctc_amd.__all__
    assert ctc_amd.blank_posteriors is ctc_amd.functional.blank_posteriors


def _call(lib, ptr=16, T=4, B=2, C=5, S=3, blank=0, **null):
    p = {k: (None if null.get(k) else ptr) for k in ("lp", "tgt", "il", "tl", "nll", "gamma", "ws")}
    return lib.ctc_amd_blank_posteriors(p["lp"], 0, 0, p["tgt"], 0, p["il"], p["tl"], T, B, C, S, blank,
                                        p["nll"], p["gamma"], p["ws"], None)


@pytest.mark.parametrize("which", ["lp", "tgt", "il", "tl", "nll", "gamma", "ws"])
def test_null_pointers(lib, which):
    # rejected before anything is dereferenced or launched: the other pointers are non-null but bogus
    assert _call(lib, **{which: True}) == -1


@pytest.mark.parametrize("kw", [dict(T=0), dict(B=0), dict(C=0), dict(S=0), dict(T=-3), dict(B=-1), dict(blank=-1),
                                dict(blank=5), dict(C=5, blank=7)])
def test_bad_sizes_and_blank(lib, kw):
    assert _call(lib, **kw) == -1


@pytest.mark.parametrize("S", [256, 300])
def test_too_many_labels(lib, S):
    assert _call(lib, S=S, C=1000) == -2


def test_no_cpu_path():
    import ctc_amd
    lp = torch.randn(6, 2, 5).log_softmax(2)
    with pytest.raises(ctc_amd.CtcAmdError):
        ctc_amd.blank_posteriors(lp, torch.tensor([[1, 2], [3, 3]]), torch.tensor([6, 6]), torch.tensor([2, 2]))


# ---- the restatement on lattices with known answers ---------------------------------------------------

def test_frames_equal_labels_distinct_is_one_hot():
    rng = np.random.default_rng(0)
    lab = [3, 1, 4, 2]
    g, nll = _one(_rand_lp(rng, 4, 6), lab)
    assert np.isfinite(nll)
    want = np.zeros((4, 9))
    want[np.arange(4), 2 * np.arange(4) + 1] = 1.0
    np.testing.assert_allclose(g, want, atol=1e-12)
    assert (g[want == 0] == 0).all()


def test_empty_target_all_mass_on_state_zero():
    rng = np.random.default_rng(1)
    lp = _rand_lp(rng, 7, 5)[:, None, :]
    g, nll = posteriors_blank(lp, np.array([[2, 3]]), [5], [0])
    np.testing.assert_allclose(g[0, :5, 0], 1.0, rtol=1e-14)
    assert (g[0, :5, 1:] == 0).all() and (g[0, 5:] == 0).all()
    np.testing.assert_allclose(nll[0], -lp[:5, 0, 0].sum(), rtol=1e-14)


def test_one_step_too_short_is_infeasible():
    rng = np.random.default_rng(2)
    g, nll = _one(_rand_lp(rng, 5, 6), [1, 2, 3], Tb=2)
    assert nll == np.inf and (g == 0).all()
    g, nll = _one(_rand_lp(rng, 5, 6), [2, 2], Tb=2)       # a repeat needs a blank between: 3 frames
    assert nll == np.inf and (g == 0).all()


def test_adjacent_repeat_forces_a_blank():
    rng = np.random.default_rng(3)
    g, nll = _one(_rand_lp(rng, 3, 6), [4, 4])
    assert np.isfinite(nll)
    want = np.zeros((3, 5))
    want[0, 1] = want[1, 2] = want[2, 3] = 1.0
    np.testing.assert_allclose(g, want, atol=1e-12)
    assert (g[want == 0] == 0).all()


def test_masked_class_keeps_exact_zeros():
    rng = np.random.default_rng(4)
    lp = _rand_lp(rng, 8, 6)
    lp[:, 2] = -np.inf                                       # label 2 can never be emitted: not a path left
    g, nll = _one(lp, [1, 2])
    assert nll == np.inf and (g == 0).all()
    lp = _rand_lp(rng, 8, 6)
    lp[3, 1] = -np.inf                                       # label 1 not at frame 3
    g, nll = _one(lp, [1, 5])
    assert np.isfinite(nll) and (g[3, 1] == 0)
    np.testing.assert_allclose(g[:8].sum(1), 1.0, atol=1e-12)


def test_rows_sum_to_one():
    rng = np.random.default_rng(5)
    T, B, C, S = 30, 6, 9, 5
    lp = np.stack([_rand_lp(rng, T, C) for _ in range(B)], 1)
    tg = rng.integers(1, C, (B, S))
    tg[1, 1] = tg[1, 0]
    Tb = np.array([30, 25, 12, 30, 1, 18])
    L = np.array([5, 3, 0, 4, 0, 5])
    g, nll = posteriors_blank(lp, tg, Tb, L)
    for b in range(B):
        np.testing.assert_allclose(g[b, :Tb[b]].sum(1), 1.0, atol=1e-12)
        assert (g[b, Tb[b]:] == 0).all() and (g[b, :, 2 * L[b] + 1:] == 0).all()


@pytest.mark.parametrize("seed", range(4))
def test_occupancy_matches_torch_gradient(seed):
    """sum over {s: l'_s = c} of gamma_t(s) = exp(lp) - d(sum nll)/d(lp), torch's float64 CPU kernel"""
    rng = np.random.default_rng(100 + seed)
    T = int(rng.integers(4, 40))
    B = int(rng.integers(1, 6))
    C = int(rng.integers(3, 12))
    S = int(rng.integers(1, 8))
    blank = int(rng.integers(0, C))
    lp = torch.tensor(np.stack([_rand_lp(rng, T, C) for _ in range(B)], 1), requires_grad=True)
    others = np.array([c for c in range(C) if c != blank])
    tg = others[rng.integers(0, C - 1, (B, S))]
    if S > 1:
        tg[0, 1] = tg[0, 0]                                  # an adjacent repeat
    L = rng.integers(0, S + 1, B)
    Tb = rng.integers(1, T + 1, B)
    Tb[0] = T
    g, nll = posteriors_blank(lp.detach().numpy(), tg, Tb, L, blank)
    loss = torch.nn.functional.ctc_loss(lp, torch.tensor(tg), torch.tensor(Tb), torch.tensor(L), blank=blank,
                                        reduction="sum", zero_infinity=False)
    feas = np.isfinite(nll)
    if feas.all():
        loss.backward()
        grad = lp.grad.numpy()
    else:                                                    # the gradient of the feasible samples alone
        keep = torch.tensor(np.nonzero(feas)[0])
        if keep.numel() == 0:
            return
        tl = torch.nn.functional.ctc_loss(lp[:, keep], torch.tensor(tg)[keep], torch.tensor(Tb)[keep],
                                          torch.tensor(L)[keep], blank=blank, reduction="sum", zero_infinity=False)
        tl.backward()
        grad = lp.grad.numpy()
    ref_nll = torch.nn.functional.ctc_loss(lp.detach(), torch.tensor(tg), torch.tensor(Tb), torch.tensor(L), blank=blank,
                                           reduction="none", zero_infinity=False).numpy()
    assert np.array_equal(np.isinf(ref_nll), ~feas)
    np.testing.assert_allclose(nll[feas], ref_nll[feas], rtol=1e-12)
    occ = class_occupancy(g, tg, Tb, L, C, blank)
    want = np.exp(lp.detach().numpy()) - grad
    for b in np.nonzero(feas)[0]:
        np.testing.assert_allclose(occ[:Tb[b], b], want[:Tb[b], b], atol=1e-10, rtol=0)
