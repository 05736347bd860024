"""A float64 reference of the blank-CTC loss and gradient that is defined at -inf log-probs, and the peaked / masked
input cases of tests/test_blank_inputs_ref.py (no GPU) and tests/test_blank_inputs_gpu.py (the kernels).

torch's own CTC gives NaN at masked entries and on whole samples with no alignment, and the oracle's exp(occ + nll - lp)
is exp(nan) there; posteriors_blank / class_occupancy of tests/test_blank_posteriors_abi.py keep -inf as -inf, so the
gradient follows from them in its occupancy form, (exp(lp) - occupancy) / (max(L_b,1) B), in which both terms are
exactly 0 at a -inf entry."""
import functools

import numpy as np
import torch

from tests.helpers import np_, synth_blank
from tests.test_blank_posteriors_abi import class_occupancy, posteriors_blank

NINF = -float("inf")


def blank_loss_grad_ref(lp, tgt, Tb, L, blank=0):
    """-> (nll [B], grad [T,B,C] of mean_b(nll_b / max(L_b,1)), fin [B]) in float64.

    grad = (exp(lp) - class occupancy of gamma) / (max(L_b,1) B); exactly 0 for t >= T_b, on every row of a sample with
    nll = +inf (no alignment: through its lengths or through its emissions) and at every -inf entry."""
    lp = np.asarray(np_(lp), dtype=np.float64)
    tgt, Tb, L = np_(tgt), np_(Tb), np_(L)
    T, B, C = lp.shape
    gamma, nll = posteriors_blank(lp, tgt, Tb, L, blank)
    fin = np.isfinite(nll)
    occ = class_occupancy(gamma, tgt, Tb, L, C, blank)
    grad = np.zeros((T, B, C))
    for b in np.nonzero(fin)[0]:
        tb = int(Tb[b])
        grad[:tb, b] = (np.exp(lp[:tb, b]) - occ[:tb, b]) / (max(int(L[b]), 1) * B)
    return nll, grad, fin


def torch_ref(lp, tgt, Tb, L, dtype, blank=0):
    """torch's CPU kernel -> nll [B], the batch-mean loss over the finite samples, its gradient (NaN where torch gives
    NaN) and which samples are finite"""
    x = lp.to(dtype).clone().requires_grad_(True)
    nll = torch.nn.functional.ctc_loss(x, tgt, Tb, L, blank=blank, reduction="none", zero_infinity=False)
    fin = torch.isfinite(nll.detach())
    loss = (nll[fin] / L.clamp(min=1)[fin].to(dtype)).sum() / lp.shape[1]
    loss.backward()
    return {"nll": np_(nll).astype(np.float64), "loss": float(loss.detach()), "grad": np_(x.grad).astype(np.float64),
            "fin": np_(fin)}


# ---- the cases ----------------------------------------------------------------------------------------------
# path: (T, B, C, S) -- the smallest shapes that reach each kernel of ctc_amd_blank_loss_grad
SHAPES = {
    "k2_scalar": (40, 4, 13, 6),        # 2 states per lane, C % 4 != 0: scalar rows; three launches only (T < 128)
    "k2": (160, 6, 36, 20),             # 2 states per lane, float4 rows
    "k4": (130, 4, 36, 100),            # 4 states per lane
    "k8": (300, 3, 40, 255),            # 8 states per lane
    "w2": (300, 3, 50, 256),            # wide, two waves
    "w3": (660, 3, 30, 600),            # wide, three waves
}
# the schedules of ctc_amd.set_blank_schedule a shape can be forced through (the wide path has one)
SCHEDULES = {"k2_scalar": (0,), "k2": (0, 1, 2), "k4": (0, 1, 2), "k8": (0, 1, 2), "w2": (None,), "w3": (None,)}
REGIMES = ("rand30", "aligned4", "aligned8", "masked")
CASES = [(p, r) for p in SHAPES for r in REGIMES] + [("k2", "masked_rand30"), ("w2", "masked_rand30")]
DIFFUSE = [(p, "diffuse") for p in SHAPES]
NLL_RTOL = 1e-5


def plain_bound(T, B):
    """the gradient bound of test_blank_vs_torch_cpu"""
    return min(1e-4, 2e-6 * max(1.0, 64.0 / B) * max(1.0, T / 300.0))


def _state_path(tgt_b, Tb, L, g):
    """a valid state path of Tb frames over the 2L+1 extended states -> class per frame, or None when there is none:
    every label state gets a frame, a blank sits between equal neighbours, the other frames are spread at random"""
    n = 2 * L + 1
    count = torch.zeros(n, dtype=torch.int64)
    count[1::2] = 1
    for l in range(1, L):
        if int(tgt_b[l]) == int(tgt_b[l - 1]):
            count[2 * l] = 1
    if L == 0:
        count[0] = 1
    spare = Tb - int(count.sum())
    if spare < 0:
        return None
    if spare:
        count += torch.bincount(torch.randint(0, n, (spare,), generator=g), minlength=n)
    cls = torch.zeros(n, dtype=torch.int64)
    cls[1::2] = tgt_b[:L]
    return torch.repeat_interleave(cls, count)


def _force_lengths(tgt, Tb, L, T):
    """in place: the samples every case holds (make_case)"""
    B, S = tgt.shape
    Tb[0], L[0] = T, S
    L[1] = max(2, min(int(L[1]), 5))
    tgt[1, 1] = tgt[1, 0]
    Tb[1] = min(int(Tb[1]), T - 1) - (min(int(Tb[1]), T - 1) + 1) % 2
    if B >= 4:
        L[2] = 0
    assert int(L[B - 1]) >= 1


def make_case(path, regime):
    """-> (lp, tgt, Tb, L), blank 0.  Lengths and targets are synth_blank's with var_T=True, then: sample 0 full
    (T_b = T, L_b = S); sample 1 short (2..5 labels, so that 1/(L_b B) keeps its gradient large against the bound),
    starting with an adjacent repeat, on an odd T_b < T; sample 2 without labels where B >= 4; sample B-1 with at least
    one label (the masked regimes take every frame of its first label's class away)."""
    T, B, C, S = SHAPES[path]
    seed = T + B + C + S
    lp, tgt, Tb, L = synth_blank(seed, T, B, C, S, var_T=True)
    g = torch.Generator().manual_seed(seed + 1)
    _force_lengths(tgt, Tb, L, T)
    if regime in ("rand30", "masked_rand30"):
        lp = (30.0 * torch.randn(T, B, C, generator=g)).log_softmax(2)
    elif regime.startswith("aligned"):
        M = float(regime[len("aligned"):])
        x = lp.clone()
        for b in range(B):
            cls = _state_path(tgt[b], int(Tb[b]), int(L[b]), g)
            if cls is not None:
                x[torch.arange(int(Tb[b])), b, cls] += M
        lp = x.log_softmax(2)
    else:
        assert regime in ("diffuse", "masked")
    if regime.startswith("masked"):
        lp[3::7, :, 0] = NINF                                   # holes in the blank ...
        lp[2::5, :, int(tgt[0, 0])] = NINF                      # ... and in sample 0's first label; frame 0 keeps both
        lp[:, B - 1, int(tgt[B - 1, 0])] = NINF                 # sample B-1: no alignment, whatever its lengths
    return lp, tgt, Tb.long(), L.long()


def feasible_by_length(tgt, Tb, L):
    """T_b >= L_b + adjacent repeats, per sample"""
    out = []
    for b in range(tgt.shape[0]):
        l = int(L[b])
        out.append(int(Tb[b]) >= l + int((tgt[b, 1:l] == tgt[b, :l - 1]).sum()) if l else True)
    return np.array(out)


@functools.lru_cache(maxsize=None)
def reference(path, regime):
    """computed once per case and shared (read-only) -> dict: inputs, the float64 reference (nll, grad, fin, loss),
    torch's float64 and float32 results, err32 = max |g32 - grad| over the feasible samples where torch's float32
    gradient is finite, the case's gradient bound min(1e-4, max(plain, 2 err32)) and max |grad|"""
    inputs = make_case(path, regime)
    lp, tgt, Tb, L = inputs
    T, B, _ = lp.shape
    nll, grad, fin = blank_loss_grad_ref(lp, tgt, Tb, L)
    t64 = torch_ref(lp, tgt, Tb, L, torch.float64)
    t32 = torch_ref(lp, tgt, Tb, L, torch.float32)
    d32 = np.abs(t32["grad"][:, fin] - grad[:, fin])
    err32 = float(d32[np.isfinite(d32)].max())
    plain = plain_bound(T, B)
    loss = float((nll[fin] / np.maximum(np_(L)[fin], 1)).sum() / B) if fin.all() else float("inf")
    for a in (nll, grad, fin):
        a.setflags(write=False)
    return {"inputs": inputs, "nll": nll, "grad": grad, "fin": fin, "loss": loss, "t64": t64, "t32": t32,
            "err32": err32, "plain": plain, "bound": min(1e-4, max(plain, 2.0 * err32)),
            "gmax": float(np.abs(grad[:, fin]).max())}


def exact_case(path):
    """-> (lp, tgt, Tb, L) drawn with integer arithmetic alone, so that every machine builds the same bits (randn and
    log_softmax need not round alike everywhere): lp = -k/512 - 1.5, k in [0, 4096), about as diffuse as a softmax over
    C classes but not normalised; the lengths of make_case.  The inputs of the recorded outputs under tests/golden/."""
    T, B, C, S = SHAPES[path]
    g = torch.Generator().manual_seed(1000 + T + B + C + S)
    lp = -(torch.randint(0, 4096, (T, B, C), generator=g).float() / 512.0) - 1.5
    tgt = torch.randint(1, C, (B, S), generator=g)
    L = torch.randint(1, S + 1, (B,), generator=g)
    Tb = torch.randint(min(2 * S + 1, T), T + 1, (B,), generator=g)
    _force_lengths(tgt, Tb, L, T)
    return lp, tgt, Tb.long(), L.long()
