"""A float64 reference of the label-smoothed no-blank loss that is defined at -inf, and the cases of
tests/test_smoothing_ref.py (no GPU) and tests/test_smoothing_gpu.py (the four-rows-per-wave kernel, every form of it).

The emission (oracle/ctc_numpy.noblank_ctc): e[t,l] = a lp[t,c_l] + b sum_n lp[t,n], b = (1 - lam) / C,
a = lam - b, lp = log_softmax(x).  The contract this file states:
  * a live row that holds a -inf logit gives every state of that row e = -inf (b sum_n lp[n] = -inf, whatever a lp[c_l]
    is), so the sample has no alignment;
  * a sample is without an alignment when its float64 nll is >= 1e12 or infinite (NO_ALIGNMENT, include/ctc_amd.h) --
    that includes finite pad logits (-1e30) whose b sum_n lp[n] alone carries nll past 1e12; its nll is reported as
    +inf here, its gradient as 0;
  * elsewhere grad = ((1 - b) softmax - a occupancy - b) / B on live rows, 0 beyond T_b.
lam = 1 is the plain loss (a = 1, b = 0: no row rule).  lam = 0 (a < 0) together with -inf would ask for -inf + inf: left
undefined, and no case here combines a <= 0 with a masked logit -- `masked` runs at lam = 0.9 and 0.5 only.

The lattice, the cases' inputs, the plain bound and the tolerances are those of tests/lattice_inputs_ref.py; `offset` is
its `aligned` case with 3.0e4 added to every logit (softmax-invariant: what a sum of raw logits loses in float32)."""
import functools

import numpy as np
import torch

from oracle import ctc_numpy
from tests.helpers import np_
from tests.lattice_inputs_ref import (NINF, NLL_RTOL, NO_ALIGNMENT, NOBLANK_SHAPES, R16, _finite_max,  # noqa: F401
                                      _log_softmax, lattice, make_case, plain_bound)

OFFSET = 3.0e4
PATHS = list(R16)                                   # r16, r16_n4, r16_n2, r16_c158, r16_s31, r16_t168, r16_ps
REGIMES = ("aligned", "wrongpeak", "masked", "ties", "offset")


def lams(path, regime):
    """the label_smoothing values of a (path, regime): 0.9, 0.5, 1 / (C + 1) (a = 0 up to rounding) and 0 (a = -1 / C);
    `masked`: the two with a > 0"""
    C = NOBLANK_SHAPES[path][2]
    return (0.9, 0.5) if regime == "masked" else (0.9, 0.5, 1.0 / (C + 1), 0.0)


# (path, regime, lam); lam = 1.0 once per path, on `aligned`
CASES = [(p, r, lam) for p in PATHS for r in REGIMES for lam in lams(p, r)] + [(p, "aligned", 1.0) for p in PATHS]


def case_id(case):
    p, r, lam = case
    name = {0.9: "0.9", 0.5: "0.5", 0.0: "0", 1.0: "1"}.get(lam, "1/(C+1)")
    return "%s-%s-lam%s" % (p, r, name)


def make_smoothing_case(path, regime):
    """-> (x [T,B,C] float32, lab, Tb, L, kinds) of tests/lattice_inputs_ref.make_case; `offset`: `aligned` + 3.0e4"""
    x, lab, Tb, L, kinds = make_case("noblank", path, "aligned" if regime == "offset" else regime)
    if regime == "offset":
        x = x + OFFSET
    return x, lab, Tb, L, kinds


def coefficients(lam, C):
    b = (1.0 - lam) / C
    return lam - b, b


def smoothed_ref(x, lab, Tb, L, lam):
    """float64 -> dict(nll [B] (+inf without an alignment), grad [T,B,C] of mean_b nll_b, fin [B], e [T,B,S])"""
    x = np.asarray(np_(x), np.float64)
    lab, Tb, L = np_(lab), np_(Tb).astype(np.int64), np_(L).astype(np.int64)
    T, B, C = x.shape
    a, b = coefficients(lam, C)
    k = lab.astype(np.int64) % C
    lp = _log_softmax(x)
    e = np.take_along_axis(lp, k[None].repeat(T, 0), axis=2)
    if b != 0.0:
        tail = lp.sum(axis=2, keepdims=True)
        with np.errstate(invalid="ignore"):
            e = np.where(np.isneginf(tail), NINF, a * e + b * tail)      # a row with a -inf logit: every state -inf
    S = e.shape[2]
    alpha, beta, nll = lattice(e, Tb, L)
    fin = nll < NO_ALIGNMENT
    nll = np.where(fin, nll, np.inf)
    live = (np.arange(T)[:, None] < Tb[None, :]) & fin[None, :]
    gamma = np.where(live[:, :, None], np.exp(alpha + beta + np.where(fin, nll, 0.0)[None, :, None]), 0.0)
    occ = np.zeros((T, B, C))
    tt, bb, _ = np.meshgrid(np.arange(T), np.arange(B), np.arange(S), indexing="ij")
    np.add.at(occ, (tt, bb, k[None].repeat(T, 0)), gamma)
    grad = np.where(live[:, :, None], ((1.0 - b) * np.exp(lp) - a * occ - b) / B, 0.0)
    return {"nll": nll, "grad": grad, "fin": fin, "e": e}


def port(x, lab, Tb, L, lam, dtype):
    """oracle/ctc_numpy.noblank_ctc with label_smoothing in `dtype` (NaN / inf where it is undefined) -> nll, grad in float64"""
    with np.errstate(all="ignore"):
        r = ctc_numpy.noblank_ctc(np_(x), np_(lab), np_(Tb), np_(L), dtype, label_smoothing=lam)
    return {"nll": r["nll"].astype(np.float64), "grad": r["grad"].astype(np.float64)}


@functools.lru_cache(maxsize=None)
def inputs(path, regime):
    return make_smoothing_case(path, regime)


@functools.lru_cache(maxsize=None)
def reference(path, regime, lam):
    """computed once per case and shared (read-only) -> dict: inputs (x, lab, Tb, L), kinds, nll, grad, fin, err32 /
    err32_nll = max |port32 - float64| of the gradient / of nll (relative to max(1, |nll|)) over the feasible samples on
    which the float32 port gives a number, plain = plain_bound at this B, bound = max(plain, 2 err32), gmax = max |grad|."""
    x, lab, Tb, L, kinds = inputs(path, regime)
    B = x.shape[1]
    r = smoothed_ref(x, lab, Tb, L, lam)
    p32 = port(x, lab, Tb, L, lam, np.float32)
    fin = r["fin"]
    ok = fin & np.isfinite(p32["nll"])
    err32 = _finite_max(np.abs(p32["grad"][:, ok] - r["grad"][:, ok]))
    err32_nll = _finite_max(np.abs(p32["nll"][ok] - r["nll"][ok]) / np.maximum(1.0, np.abs(r["nll"][ok])))
    plain = plain_bound("noblank", B)
    r.update(inputs=(x, lab, Tb, L), kinds=kinds, err32=err32, err32_nll=err32_nll, plain=plain,
             bound=max(plain, 2.0 * err32), gmax=float(np.abs(r["grad"]).max()))
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return r


def batch_case(B, seed=0):
    """the batch-loss-sum case: `aligned`-style inputs at (24, B, 10, 6) -> (x, lab, Tb, L)"""
    T, C, S = 24, 10, 6
    g = torch.Generator().manual_seed(1000 + B + seed)
    x = torch.randn(T, B, C, generator=g) * 3.0
    lab = torch.randint(0, C, (B, S), generator=g, dtype=torch.int32)
    Tb = torch.randint(T // 2, T + 1, (B,), generator=g).long()
    L = torch.randint(1, S + 1, (B,), generator=g).long()
    Tb[0], L[0] = T, S
    lab[torch.arange(S)[None, :] >= L[:, None]] = -1
    return x, lab, Tb, L
