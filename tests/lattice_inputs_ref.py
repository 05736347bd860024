"""A float64 reference of the no-blank and the binary lattice that is defined at -inf (loss, gradient, posteriors, best
path), and the peaked / masked / tied input cases of tests/test_lattice_inputs_ref.py (no GPU) and
tests/test_lattice_inputs_gpu.py (the kernels).

oracle/ctc_numpy keeps the reference's -1e13 sentinel and its two-term log-sum-exp, which is NaN on (-inf, -inf); the
lattice here uses true -inf for impossible states and np.logaddexp, so nothing in it depends on the sentinel.  beta is
kept WITHOUT its own emission, so gamma = exp(alpha + beta + nll) never forms -inf - (-inf).  The one rule taken from
the library's contract: a sample whose nll reaches 1e12 has no alignment (a -1e30 emission is "impossible" to every
caller although it is a number); its nll is reported as +inf, its gradient and posteriors as 0, its path as -1."""
import functools
import math

import numpy as np
import torch

from oracle import ctc_numpy
from tests.helpers import np_

NINF = -float("inf")
PAD_LOGIT = -1.0e30                     # ctc_amd.producer.PAD_LOGIT (asserted in tests/test_lattice_inputs_ref.py)
NO_ALIGNMENT = 1e12                     # nll at or beyond: no alignment (include/ctc_amd.h)
NLL_RTOL = 1e-5
GAMMA_ATOL = 2e-4                       # test_noblank_posteriors / test_binary_posteriors
CAP = 2e-3                              # 2 err32 on B * grad and on gamma: 0.2 % of full scale

# ---- shapes: (T, B, C, S), one per kernel the default dispatch can launch ------------------------------------------
# no-blank: the family and chunking are those of noblank_plan() at 256 CUs (tests/test_noblank_plan.py restates the
# rules; tests/test_lattice_inputs_ref.py asks the plan itself).  B = 5 so that a masked batch holds all five kinds.
NOBLANK_SHAPES = {
    "r16": (24, 5, 10, 6),              # r16, chunking (n4, n2) = (0, 1)
    "r16_n4": (24, 5, 64, 6),           # r16, chunking (1, 0)
    "r16_n2": (24, 5, 34, 6),           # r16, chunking (0, 2)
    "r16_c158": (40, 5, 158, 20),       # r16, the flagship's row width
    "r16_s31": (40, 5, 12, 31),         # r16, its last S
    "r16_t168": (168, 5, 6, 8),         # r16, its last T
    "r16_ps": (24, 520, 10, 6),         # r16, the persistent form: B > 2 x 256
    "xr_oddc": (24, 5, 11, 6),          # xr: odd C keeps r16 away
    "xr_s40": (44, 5, 12, 40),          # xr: S > 31
    "pipelined": (110, 5, 12, 64),      # pipelined: the xr arrays no longer fit
    "fused_t": (170, 5, 12, 6),         # fused, one state per lane: T > 168
    "fused_c": (20, 5, 258, 6),         # fused, one state per lane, strided rows: C > 256
    "fused_k2": (90, 5, 12, 70),        # fused, two states per lane
    "fused_k4": (96, 5, 8, 130),        # fused, four states per lane (T = 100 falls into the workspace lattice)
    "glb": (216, 5, 6, 64),             # fused with the lattice in the workspace: (3 T + 8) S floats beyond LDS
    "spans_k4": (88, 5, 8, 130),        # read-outs only: four states per lane within the token spans' LDS bound
}
NOBLANK_FAMILY = {"xr_oddc": "xr", "xr_s40": "xr", "pipelined": "pipelined"}      # others: by prefix (r16 / fused)
NOBLANK_LOSS = [p for p in NOBLANK_SHAPES if p != "spans_k4"]
R16 = [p for p in NOBLANK_LOSS if p.startswith("r16")]

# binary: the kernel is the one binary_plan() names (ctc_amd/csrc/binary.hip; tests/test_binary_plan.py restates the rules
# and asks the plan about every name here, tests/test_lattice_inputs_ref.py asks it too)
BINARY_SHAPES = {
    "flow": (40, 2, 30, 12),            # streamed: S <= 64, T <= 160, C <= 192, its arrays within LDS
    "flow_c158": (40, 2, 158, 20),      # streamed, three column chunks
    "pipe_c": (30, 2, 200, 6),          # pipelined: 192 < C <= 256 (four column chunks)
    "pipe_t": (165, 2, 12, 6),          # pipelined: 160 < T <= 168
    "mfma_k2": (90, 2, 12, 70),         # MFMA, two states per lane: 64 < S <= 128, T <= 160, C <= 256
    "mfma_k4": (80, 2, 12, 130),        # MFMA, four states per lane: 128 < S <= 256 (T = 80: 160 128 of 163 840 bytes)
    "valu_c": (30, 2, 257, 6),          # VALU: C > 256
    "valu_t": (170, 2, 40, 12),         # VALU: T > 168
}
BINARY_KERNEL = {"flow": "flow", "flow_c158": "flow", "pipe_c": "pipe", "pipe_t": "pipe", "mfma_k2": "mfma2",
                 "mfma_k4": "mfma4", "valu_c": "valu1", "valu_t": "valu1"}
SHAPES = {"noblank": NOBLANK_SHAPES, "binary": BINARY_SHAPES}
LOSS_PATHS = {"noblank": NOBLANK_LOSS, "binary": list(BINARY_SHAPES)}
# the read-outs: one, two and four states per lane for the best path and the token spans; the posteriors' own kernels
PATH_SHAPES = {"noblank": ["r16", "fused_k2", "spans_k4"], "binary": ["flow", "mfma_k2", "mfma_k4"]}
POSTERIOR_SHAPES = {"noblank": ["r16", "fused_k2"], "binary": ["flow", "pipe_t"]}     # (r16, fused) / (streamed, pipelined)
REGIMES = ("aligned", "wrongpeak", "masked", "ties")
# wrongpeak, no-blank: randn x k.  k = 30 by default; on the long shapes the largest of 30, 10, 4 that keeps the float32
# port within the cap (measured on the CPU at x 30: 2 err32 B = 3.9e-3 on r16_t168, 2.4e-3 on pipelined, 4.4e-3 on
# fused_t, 2.6e-3 on spans_k4).  The workspace lattice is reached through S = 64 at T = 216, not through T = 700, where
# the port is off by 1.4e-2 already on ties
WRONGPEAK_K = {"r16_t168": 10.0, "pipelined": 10.0, "fused_t": 4.0, "glb": 4.0, "spans_k4": 10.0}
# wrongpeak, binary: (randn x k).clamp(-15, 15), k = 4 wherever the float32 port of the reference keeps nll within the
# 1e-5 the kernels are held to.  Near |x| = 15 the reference's own float32 arithmetic (1 - fl(p) before the logarithm)
# leaves float64 behind: at x 4 the port's nll is off by 1.8e-5 relative on flow_c158, 1.4e-5 on mfma_k2 and valu_c and
# 1.15e-5 on mfma_k4, and 2 err32 on gamma is 3.7e-3 on pipe_t -- no yardstick there; x 2 on those five (pipe_c, at
# 6e-6, and flow and valu_t keep x 4)
BINARY_WRONGPEAK_K = {"pipe_t": 2.0, "flow_c158": 2.0, "mfma_k2": 2.0, "mfma_k4": 2.0, "valu_c": 2.0}
KINDS = "abcde"                          # the samples of a masked no-blank batch, b % 5 (make_case)


def plain_bound(family, B):
    """the gradient bound of test_noblank_vs_oracle_shapes / test_binary_vs_oracle_shapes at this batch size"""
    return (2e-6 if family == "noblank" else 2e-7) * max(1.0, 256.0 / B)


# ---- the float64 lattice -------------------------------------------------------------------------------------------
def lattice(e, Tb, L):
    """e [T,B,S] float64 emissions, -inf allowed -> alpha [T,B,S] (with its emission), beta [T,B,S] (without), nll [B];
    -inf on every impossible state, rows t >= T_b and states l >= L_b are -inf."""
    T, B, S = e.shape
    Tb, L = np.asarray(Tb), np.asarray(L)
    inside = np.arange(S)[None, :] < L[:, None]
    bi = np.arange(B)
    alpha = np.full((T, B, S), NINF)
    beta = np.full((T, B, S), NINF)
    with np.errstate(invalid="ignore"):
        alpha[0, :, 0] = e[0, :, 0]
        for t in range(1, T):
            adv = np.full((B, S), NINF)
            adv[:, 1:] = alpha[t - 1, :, :-1]
            alpha[t] = np.where(inside, np.logaddexp(alpha[t - 1], adv) + e[t], NINF)
        alpha[np.arange(T)[:, None] >= Tb[None, :]] = NINF
        nll = -alpha[Tb - 1, bi, L - 1]
        for t in range(T - 1, -1, -1):
            if t + 1 < T:
                nxt = beta[t + 1] + e[t + 1]
                adv = np.full((B, S), NINF)
                adv[:, :-1] = nxt[:, 1:]
                beta[t] = np.where(inside & (t < Tb - 1)[:, None], np.logaddexp(nxt, adv), NINF)
            last = t == Tb - 1
            beta[t, bi[last], L[last] - 1] = 0.0
    assert not np.isnan(alpha).any() and not np.isnan(beta).any()
    return alpha, beta, nll


def viterbi(e, Tb, L):
    """the max-semiring twin; a tie keeps the state (advance only when adv > stay) -> (path [B,T] int32, score [B])"""
    T, B, S = e.shape
    path = np.full((B, T), -1, np.int32)
    score = np.full(B, NINF)
    for b in range(B):
        tb, l = int(Tb[b]), int(L[b])
        v = np.full(l, NINF)
        v[0] = e[0, b, 0]
        bp = np.zeros((tb, l), bool)
        for t in range(1, tb):
            adv = np.concatenate(([NINF], v[:-1]))
            bp[t] = adv > v
            v = np.where(bp[t], adv, v) + e[t, b, :l]
        if v[l - 1] > -NO_ALIGNMENT:
            score[b] = v[l - 1]
            s = l - 1
            for t in range(tb - 1, -1, -1):
                path[b, t] = s
                if bp[t, s]:
                    s -= 1
    return path, score


def _log_softmax(x):
    with np.errstate(divide="ignore"):
        m = x.max(axis=2, keepdims=True)
        return (x - m) - np.log(np.exp(x - m).sum(axis=2, keepdims=True))


def lattice_ref(family, x, tg, Tb, L):
    """-> dict(nll [B] (+inf without an alignment), grad [T,B,C] of mean_b nll_b, gamma [B,T,S], path [B,T], score [B],
    fin [B]) in float64"""
    x = np.asarray(np_(x), np.float64)
    tg, Tb, L = np_(tg), np_(Tb).astype(np.int64), np_(L).astype(np.int64)
    T, B, C = x.shape
    if family == "noblank":
        lab = tg.astype(np.int64) % C
        lp = _log_softmax(x)
        e = np.take_along_axis(lp, lab[None].repeat(T, 0), axis=2)
    else:
        y = np.asarray(tg, np.float64)
        e = ctc_numpy.binary_emissions(x, y, np.float64)
    S = e.shape[2]
    alpha, beta, nll = lattice(e, Tb, L)
    fin = nll < NO_ALIGNMENT
    nll = np.where(fin, nll, np.inf)
    live = (np.arange(T)[:, None] < Tb[None, :]) & fin[None, :]
    gamma = np.where(live[:, :, None], np.exp(alpha + beta + np.where(fin, nll, 0.0)[None, :, None]), 0.0)
    grad = np.zeros((T, B, C))
    if family == "noblank":
        occ = np.zeros((T, B, C))
        tt, bb, _ = np.meshgrid(np.arange(T), np.arange(B), np.arange(S), indexing="ij")
        np.add.at(occ, (tt, bb, lab[None].repeat(T, 0)), gamma)
        grad = np.where(live[:, :, None], (np.exp(lp) - occ) / B, 0.0)
    else:
        with np.errstate(over="ignore"):
            p = 1.0 / (1.0 + np.exp(-x))
        pq = p * (1.0 - p)
        ratio = pq / np.maximum(pq, 1e-12)            # torch's binary_cross_entropy backward (oracle/ctc_numpy.binary_ctc)
        occ = np.einsum("tbl,blc->tbc", gamma, y)
        grad = np.where(live[:, :, None], (p - occ) * ratio / (B * C), 0.0)
    path, score = viterbi(e, Tb, L)
    assert np.array_equal(np.isfinite(score), fin)
    return {"nll": nll, "grad": grad, "gamma": gamma.transpose(1, 0, 2).copy(), "path": path, "score": score, "fin": fin,
            "e": e}


# ---- closed forms on tied inputs -------------------------------------------------------------------------------------
def ties_closed_form(family, T, C, S, Tb, L):
    """constant emissions -> (nll [B], gamma [B,T,S], path [B,T]): every alignment has the same probability, there are
    binom(T_b - 1, L_b - 1) of them, binom(t, l) binom(T_b-1-t, L_b-1-l) pass through (t, l); ties stay"""
    B = len(Tb)
    per_frame = math.log(C) if family == "noblank" else math.log(2.0)
    nll, gamma, path = np.zeros(B), np.zeros((B, T, S)), np.full((B, T), -1, np.int32)
    for b in range(B):
        tb, l = int(Tb[b]), int(L[b])
        total = math.comb(tb - 1, l - 1)
        nll[b] = tb * per_frame - math.log(total)
        for t in range(tb):
            path[b, t] = min(t, l - 1)
            for s in range(min(l, t + 1)):
                gamma[b, t, s] = math.comb(t, s) * math.comb(tb - 1 - t, l - 1 - s) / total
    return nll, gamma, path


# ---- the cases -------------------------------------------------------------------------------------------------------
def _alignment(tb, l, g):
    """a random monotone alignment of l labels over tb frames -> label position per frame"""
    cuts = torch.sort(torch.randperm(tb - 1, generator=g)[:l - 1] + 1).values
    return torch.searchsorted(cuts, torch.arange(tb), right=True)


def _lengths(T, B, S, g):
    """T_b ragged in [T/2, T], L_b <= T_b; sample 0 is full (T_b = T, L_b = min(S, T)): every lane of a lattice with
    several states per lane holds live states; the last sample has L_b < T_b"""
    Tb = torch.randint(max(2, T // 2), T + 1, (B,), generator=g)
    L = torch.minimum(torch.randint(1, S + 1, (B,), generator=g), Tb)
    Tb[0], L[0] = T, min(S, T)
    if int(L[B - 1]) >= int(Tb[B - 1]):                      # the last sample has a choice of alignments (where S > T
        L[B - 1] = max(1, int(Tb[B - 1]) // 2)               # the draw above mostly ends at L_b = T_b): a tie rule shows
    return Tb.long(), L.long()


def make_case(family, path, regime):
    """-> (x [T,B,C] float32, targets, Tb, L, kinds): seeded by the shape.

    no-blank targets are [B,S] int32 labels padded with -1, binary targets [B,S,C] multi-hot rows (density 0.2).
      aligned    a trained model: no-blank randn + 8 on the class of a random monotone alignment; binary
                 6 (2 y_align - 1) + randn (inside the reference's parity domain |x| <= 15)
      wrongpeak  no-blank randn x k (WRONGPEAK_K, 30 by default); binary (randn x 4).clamp(-15, 15)
      masked     no-blank, sample b is of kind KINDS[b % 5]:
                   a  -inf on two classes outside its transcript on every frame, PAD_LOGIT on a third
                   b  -inf on one of its own label classes on every other frame a random alignment does not give to
                      that class (so the alignment survives)
                   c  as b with -1e4, and one frame with -1e3 on every label class: nll ~ 1e3, feasible (at -1e4 on
                      that frame the float32 port itself leaves the cap: nll ~ 1e4 costs it 1e-3 per step)
                   d  one frame with -inf on every label class: no alignment
                   e  as d with -1e30
                 binary: +inf, -inf, PAD_LOGIT and +-100 scattered (3 % of the entries), a whole column of -inf and one of
                 +inf, a whole row of PAD_LOGIT and one of +100
      ties       no-blank constant logits, binary x = 0
    kinds: the string of the batch's kinds ('-' outside the masked no-blank regime)."""
    T, B, C, S = SHAPES[family][path]
    seed = 7 * T + 5 * B + 3 * C + S + (0 if family == "noblank" else 1000)
    g = torch.Generator().manual_seed(seed)
    Tb, L = _lengths(T, B, S, g)
    x = torch.randn(T, B, C, generator=g)
    kinds = ["-"] * B
    if family == "noblank":
        lab = torch.randint(0, C, (B, S), generator=g, dtype=torch.int32)
        if regime == "masked":
            kinds = [KINDS[b % 5] for b in range(B)]
            for b, k in enumerate(kinds):
                if k == "a":                                       # its transcript leaves classes 0, 2 and C-1 alone
                    free = torch.tensor([c for c in range(C) if c not in (0, 2, C - 1)], dtype=torch.int32)
                    lab[b] = free[torch.randint(0, len(free), (S,), generator=g)]
                else:                                              # class C-1 keeps the masked row's softmax defined
                    lab[b] = torch.randint(0, C - 1, (S,), generator=g, dtype=torch.int32)
                if k in "bc":
                    L[b] = max(int(L[b]), 2)
                    if bool((lab[b, :int(L[b])] == lab[b, 0]).all()):
                        lab[b, 1] = (int(lab[b, 0]) + 1) % (C - 1)
        lab[torch.arange(S)[None, :] >= L[:, None]] = -1
        if regime == "aligned":
            for b in range(B):
                tb = int(Tb[b])
                a = _alignment(tb, int(L[b]), g)
                x[torch.arange(tb), b, lab[b, a].long()] += 8.0
        elif regime == "wrongpeak":
            x = x * WRONGPEAK_K.get(path, 30.0)
        elif regime == "ties":
            x = torch.full((T, B, C), 1.5)
        elif regime == "masked":
            for b, k in enumerate(kinds):
                tb, l = int(Tb[b]), int(L[b])
                own = lab[b, :l].long()
                if k == "a":
                    x[:, b, 0] = NINF
                    x[:, b, 2] = PAD_LOGIT
                    x[:, b, C - 1] = NINF
                if k in "bc":
                    a = _alignment(tb, l, g)
                    c = int(own[l // 2])
                    frames = torch.nonzero(own[a] != c)[::2, 0]
                    assert len(frames)
                    x[frames, b, c] = NINF if k == "b" else -1.0e4
                if k in "cde":
                    x[tb // 3, b, torch.unique(own)] = {"c": -1.0e3, "d": NINF, "e": PAD_LOGIT}[k]
        return x, lab, Tb, L, "".join(kinds)
    y = (torch.rand(B, S, C, generator=g) < 0.2).float()
    y[torch.arange(S)[None, :] >= L[:, None]] = 0.0
    if regime == "aligned":
        for b in range(B):
            tb = int(Tb[b])
            a = _alignment(tb, int(L[b]), g)
            x[:tb, b] += 6.0 * (2.0 * y[b, a] - 1.0)
    elif regime == "wrongpeak":
        x = (x * BINARY_WRONGPEAK_K.get(path, 4.0)).clamp(-15.0, 15.0)
    elif regime == "ties":
        x = torch.zeros(T, B, C)
    elif regime == "masked":
        values = torch.tensor([float("inf"), NINF, PAD_LOGIT, 100.0, -100.0])
        hit = torch.rand(T, B, C, generator=g) < 0.03
        x = torch.where(hit, values[torch.randint(0, 5, (T, B, C), generator=g)], x)
        x[:, 0, 1] = NINF
        x[:, 1, C - 2] = float("inf")
        x[3, 0, :] = PAD_LOGIT
        x[5, 1, :] = 100.0
    return x, y, Tb, L, "".join(kinds)


def _port(family, x, tg, Tb, L, dtype):
    fn = ctc_numpy.noblank_ctc if family == "noblank" else ctc_numpy.binary_ctc
    with np.errstate(all="ignore"):
        r = fn(np_(x), np_(tg), np_(Tb), np_(L), dtype)
    return {"nll": r["nll"].astype(np.float64), "grad": r["grad"].astype(np.float64),
            "gamma": r["gamma"].transpose(1, 0, 2).astype(np.float64)}


def _finite_max(d):
    d = d[np.isfinite(d)]
    return float(d.max()) if d.size else 0.0


@functools.lru_cache(maxsize=None)
def reference(family, path, regime):
    """computed once per case and shared (read-only) -> dict: inputs (x, targets, Tb, L), kinds, the float64 reference
    (nll, grad, gamma, path, score, fin), err32 / err32_gamma / err32_nll = max |port32 - float64| of the gradient / of gamma /
    of nll (relative to max(1, |nll|)) over
    the feasible samples (where the float32 port, oracle/ctc_numpy with np.float32, gives a number: it is NaN on a
    sample with a -inf label class), plain = the existing tests' gradient bound at this B, bound = max(plain, 2 err32),
    gamma_bound = max(2e-4, 2 err32_gamma), gmax = max |grad|."""
    x, tg, Tb, L, kinds = make_case(family, path, regime)
    B = x.shape[1]
    r = lattice_ref(family, x, tg, Tb, L)
    p32 = _port(family, x, tg, Tb, L, np.float32)
    fin = r["fin"]
    ok = fin & np.isfinite(p32["nll"])
    err32 = _finite_max(np.abs(p32["grad"][:, ok] - r["grad"][:, ok]))
    err32_gamma = _finite_max(np.abs(p32["gamma"][ok] - r["gamma"][ok]))
    err32_nll = _finite_max(np.abs(p32["nll"][ok] - r["nll"][ok]) / np.maximum(1.0, np.abs(r["nll"][ok])))
    plain = plain_bound(family, B)
    r.update(inputs=(x, tg, Tb, L), kinds=kinds, err32=err32, err32_gamma=err32_gamma, err32_nll=err32_nll, plain=plain,
             bound=max(plain, 2.0 * err32), gamma_bound=max(GAMMA_ATOL, 2.0 * err32_gamma),
             gmax=float(np.abs(r["grad"]).max()))
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return r


def port64(family, path, regime):
    """oracle/ctc_numpy in float64 on a case (NaN where it is undefined)"""
    x, tg, Tb, L, _ = make_case(family, path, regime)
    return _port(family, x, tg, Tb, L, np.float64)
