"""What the scalar `loss` of a launch must be, given the per-sample nll the same launch returned, and inputs whose nll is
known in closed form -- the reference of tests/test_batch_sum_gpu.py, checked without a GPU by tests/test_batch_sum_ref.py.

Everything here follows the definitions of include/ctc_amd.h alone (the comment on ctc_amd_noblank_loss_grad's `loss`,
blank_ctc_loss's mean_b(nll_b / max(L_b, 1))), never a kernel's answer:

* B <= 4095, no-blank and binary: every nll in [0, 8192) is rounded to a multiple of 2^-F, F = 27 - ceil(log2 B), half to
  even, and those multiples are added exactly; every other value (>= 8192, the 1e13 / 1e30 sentinels, negative, NaN) is
  added in float64; loss = float32(sum * loss_scale).  `expected_sum_loss`.
* B > 4095 and the blank loss: an fp32 sum of the B terms (nll_b, or nll_b / max(L_b, 1)) in some fixed order, times
  loss_scale in fp32.  `expected_ticket_loss`.

The inputs: one label (L_b = 1), so one alignment (no-blank, binary) or a count of equally likely ones (blank), and the
nll is a closed form of one per-sample number the test chooses.
"""
import math
from collections import namedtuple

import numpy as np

ACC_INT_BITS = 13                 # a value fits the packed sum when 0 <= v < 2^13
ACC_LIMIT = float(1 << ACC_INT_BITS)
ACC_MAX_B = 4095                  # beyond: the arrival-ticket form
ACC_SHARDS = 16
SUM_BITS, COUNT_BITS = 40, 12     # [39:0] the sum, [51:40] values that did not fit, [63:52] arrivals
INFEASIBLE = 1.0e12               # nll >= this <=> no alignment (include/ctc_amd.h)

Expected = namedtuple("Expected", "value mean bound slack all_fit")
# value:   the loss predicted from the nll, float32 (exact when all_fit: fixed-point addition has no rounding)
# mean:    float64 loss_scale * sum(nll), unquantised -- what `bound` is measured against
# bound:   the header's contract |loss - mean| <= B 2^-(F+1) loss_scale + 1 ulp(loss) (+ slack)
# slack:   |loss - value| beyond 1 ulp: the float64 additions of the values that did not fit, in an order the launch chooses
#          (the ticket form: the bound of its fp32 sum)


def ceil_log2(B):
    return 0 if B <= 1 else (B - 1).bit_length()


def frac_bits(B):
    """F of include/ctc_amd.h: 27 - ceil(log2 B) fractional bits, B in [1, 4095]"""
    assert 1 <= B <= ACC_MAX_B
    return SUM_BITS - ACC_INT_BITS - ceil_log2(B)


def shard_members(B, sh):
    """samples b < B with b % 16 == sh, as the finishing test of a shard counts them"""
    return (B - sh + ACC_SHARDS - 1) // ACC_SHARDS


def fits(v):
    v = np.asarray(v, np.float32)
    with np.errstate(invalid="ignore"):
        return (v >= 0) & (v < np.float32(ACC_LIMIT))


def quantum(v, F):
    """rint(float64(v) * 2^F) as a Python integer, half to even (the product is exact: a power of two)"""
    return int(np.rint(np.float64(np.float32(v)) * np.float64(2.0 ** F)))


def field_width_problems(B):
    """-> list of strings, empty when no field of the packed word can carry into its neighbour at this B"""
    out = []
    F = frac_bits(B)
    if F < 0:
        out.append("negative fraction")
    largest = np.nextafter(np.float32(ACC_LIMIT), np.float32(0))          # the largest value that fits
    if B * quantum(largest, F) >= 1 << SUM_BITS:
        out.append("B values below 8192 reach 2^40")
    if B >= 1 << COUNT_BITS:
        out.append("arrivals beyond 12 bits")                           # (and so the count of values that did not fit)
    members = [shard_members(B, sh) for sh in range(ACC_SHARDS)]
    if max(members) > 256:
        out.append("a shard of more than 256 members")
    if max(members) * quantum(largest, F) >= 1 << SUM_BITS:
        out.append("a shard's sum reaches 2^40")
    if sum(members) != B:
        out.append("shards do not add up to B")
    return out


def _ulp32(v):
    v = np.float32(abs(v))
    return float(np.spacing(v)) if np.isfinite(v) else 0.0


def _f32(v):
    with np.errstate(over="ignore"):
        return np.float32(v)


def expected_sum_loss(nll32, B, scale32):
    """The packed fixed-point sum of B <= 4095 values -> Expected."""
    nll32 = np.asarray(nll32, np.float32)
    assert nll32.shape == (B,) and 1 <= B <= ACC_MAX_B
    scale = np.float64(np.float32(scale32))
    if np.isnan(nll32).any():
        return Expected(np.float32(np.nan), float("nan"), 0.0, 0.0, False)
    F = frac_bits(B)
    fit = fits(nll32)
    fixed = sum(quantum(v, F) for v in nll32[fit])                        # exact: Python integers
    assert fixed < 1 << SUM_BITS
    rest = [float(v) for v in nll32[~fit]]
    head = fixed * 2.0 ** -F                                              # exact: fixed < 2^40
    if all(math.isfinite(v) for v in rest):
        total = math.fsum([head] + rest)
        mean = math.fsum([float(v) for v in nll32]) * float(scale)
        mag = head + sum(abs(v) for v in rest)
    else:
        with np.errstate(invalid="ignore"):
            total = mean = float(np.sum(np.asarray(rest, np.float64)))    # +inf, -inf or NaN
        mag = 0.0
    value = _f32(np.float64(total) * scale)
    # each of the len(rest) float64 additions rounds by at most 2^-53 of a partial sum <= mag
    slack = len(rest) * 2.0 ** -53 * mag * float(scale) if len(rest) > 1 or (rest and fixed) else 0.0
    bound = int(fit.sum()) * 2.0 ** -(F + 1) * float(scale) + _ulp32(value) + slack
    return Expected(value, mean, bound, slack, bool(fit.all()))


def expected_ticket_loss(terms32, scale32):
    """The arrival-ticket form: the last workgroup adds the B fp32 terms (64 interleaved partial sums and a tree over
    them: ceil(B/64) + 6 roundings on the way of any term) and multiplies by loss_scale in fp32 -> Expected."""
    terms32 = np.asarray(terms32, np.float32)
    B = terms32.shape[0]
    scale = np.float64(np.float32(scale32))
    if np.isnan(terms32).any():
        return Expected(np.float32(np.nan), float("nan"), 0.0, 0.0, False)
    if np.isinf(terms32).any():
        with np.errstate(invalid="ignore"):
            total = float(np.sum(terms32.astype(np.float64)))             # +inf; NaN when both signs are present
        return Expected(_f32(total), total, 0.0, 0.0, False)
    total = math.fsum(float(v) for v in terms32)
    mag = math.fsum(abs(float(v)) for v in terms32)
    value = _f32(np.float64(total) * scale)
    bound = (-(-B // 64) + 6) * 2.0 ** -24 * mag * float(scale) + _ulp32(value)
    return Expected(value, total * float(scale), bound, bound, False)


def expected_loss(family, nll32, B, scale32, L=None):
    """What a launch of `family` ("noblank", "binary", "blank") with these per-sample nll must report as its loss"""
    nll32 = np.asarray(nll32, np.float32)
    if family == "blank":
        with np.errstate(invalid="ignore"):
            terms = nll32 / np.maximum(np.asarray(L), 1).astype(np.float32)          # fp32 division, as the header's formula
        return expected_ticket_loss(terms, scale32)
    if B > ACC_MAX_B:
        return expected_ticket_loss(nll32, scale32)
    return expected_sum_loss(nll32, B, scale32)


def check_loss(loss32, e):
    """-> list of strings: how `loss32` (float32) misses Expected `e`; empty when it meets contract and prediction"""
    loss32 = np.float32(loss32)
    if np.isnan(e.value):
        return [] if np.isnan(loss32) else ["loss %r where NaN is due" % loss32]
    if np.isinf(e.value):
        return [] if loss32 == e.value else ["loss %r where %r is due" % (loss32, e.value)]
    out = []
    if not np.isfinite(loss32):
        return ["loss %r where %r is due" % (loss32, e.value)]
    if abs(float(loss32) - e.mean) > e.bound:
        out.append("loss %.9g is %.3g from the mean %.17g, bound %.3g" % (loss32, abs(float(loss32) - e.mean), e.mean, e.bound))
    if e.all_fit and loss32 != e.value:
        out.append("loss %.9g (%s) is not the fixed-point prediction %.9g (%s)"
                   % (loss32, loss32.tobytes().hex(), e.value, e.value.tobytes().hex()))
    if abs(float(loss32) - float(e.value)) > e.slack + _ulp32(e.value):
        out.append("loss %.9g is %.3g from the prediction %.9g, slack %.3g + 1 ulp"
                   % (loss32, abs(float(loss32) - float(e.value)), e.value, e.slack))
    return out


# ---- inputs with a known nll ----------------------------------------------------------------------------------------
Batch = namedtuple("Batch", "x tgt Tb L nll64 infeasible")
# x [T,B,C] float32 logits (blank: log-probs, used as given); tgt: labels [B,S] int32 / rows [B,S,C] float32 / targets [B,S]
# int64; nll64 [B] the closed form in float64 (inf where `infeasible`)

BIN_SATURATED = 87.0              # a per-frame BCE from here on is asked for as the clamp itself (100): exp() of it leaves fp32


def _per_sample(v, B, dtype):
    return np.broadcast_to(np.asarray(v, dtype), (B,)).copy()


def noblank_batch(T, C, S, Tb, target, no_alignment=None, masked=None, nan=None):
    """No-blank, L_b = 1, label b % C at logit -M_b, every other class at 0: the one alignment has
    nll_b = T_b (M_b + ln(C - 1 + exp(-M_b))); M_b is chosen for nll_b ~ target[b] and rounded to float32.
    `no_alignment`: samples with L_b = 2 > T_b = 1; `masked`: samples whose label logit is -inf; `nan`: samples with one
    NaN logit in their first row."""
    B = len(target)
    Tb = _per_sample(Tb, B, np.int64)
    per = np.asarray(target, np.float64) / Tb
    with np.errstate(over="ignore"):
        M = (per + np.log1p(-np.exp(-per)) - math.log(C - 1)).astype(np.float32)
    M64 = M.astype(np.float64)
    with np.errstate(over="ignore"):
        nll = Tb * (M64 + np.log(C - 1 + np.exp(-M64)))
    lab = np.full((B, S), -1, np.int32)
    lab[:, 0] = np.arange(B) % C
    L = np.ones(B, np.int64)
    x = np.zeros((T, B, C), np.float32)
    x[:, np.arange(B), lab[:, 0]] = -M[None, :]
    bad = np.zeros(B, bool)
    if no_alignment is not None and len(no_alignment):
        i = np.asarray(no_alignment)
        lab[i, 1] = (i + 1) % C
        L[i], Tb[i], bad[i] = 2, 1, True
    if masked is not None and len(masked):
        i = np.asarray(masked)
        x[:, i, lab[i, 0]] = -np.inf
        bad[i] = True
    if nan is not None and len(nan):
        i = np.asarray(nan)
        x[0, i, (lab[i, 0] + 1) % C] = np.nan
    nll = np.where(bad, np.inf, nll)
    return Batch(x, lab, Tb, L, nll, bad)


def binary_frame_bce(m32):
    """BCE of one frame whose C logits are all -m against a target row of ones: ln(1 + exp(m)), clamped at 100"""
    m = np.asarray(m32, np.float32).astype(np.float64)
    with np.errstate(over="ignore"):
        return np.minimum(np.where(m > 30.0, m + np.log1p(np.exp(-np.abs(m))), np.log1p(np.exp(np.minimum(m, 30.0)))), 100.0)


def binary_batch(T, C, S, Tb, target, no_alignment=None, nan=None):
    """Binary, L_b = 1, the label row all ones, every logit of sample b at -m_b: nll_b = T_b min(ln(1 + exp(m_b)), 100).
    A target of BIN_SATURATED per frame or more is asked for as m_b = 200: the clamp itself, 100 per frame."""
    B = len(target)
    Tb = _per_sample(Tb, B, np.int64)
    per = np.asarray(target, np.float64) / Tb
    with np.errstate(over="ignore", invalid="ignore"):
        m = np.where(per >= BIN_SATURATED, 200.0, np.where(per > 30.0, per + np.log1p(-np.exp(-per)), np.log(np.expm1(per))))
    m = m.astype(np.float32)
    nll = Tb * binary_frame_bce(m)
    y = np.zeros((B, S, C), np.float32)
    y[:, 0] = 1.0
    L = np.ones(B, np.int64)
    x = np.broadcast_to(-m[None, :, None], (T, B, C)).copy()
    bad = np.zeros(B, bool)
    if no_alignment is not None and len(no_alignment):
        i = np.asarray(no_alignment)
        y[i, 1] = 1.0
        L[i], Tb[i], bad[i] = 2, 1, True
    if nan is not None and len(nan):
        x[0, np.asarray(nan), 0] = np.nan
    nll = np.where(bad, np.inf, nll)
    return Batch(x, y, Tb, L, nll, bad)


def binary_random_batch(T, C, S, Tb, seed, no_alignment=None):
    """Binary, L_b = 1, random logits (unit normal x 2) against a random multi-hot row: still one alignment, so
    nll_b = sum_{t < T_b} mean_c BCE(sigmoid(x[t,b,c]), y[b,0,c]) in float64.  For the lattice at large batches: on the
    constant logits of binary_batch every frame and class repeats one rounding error, which then adds up T_b C times
    instead of averaging out (the kernels form the emission as a difference of two sums over the classes)."""
    Tb = np.asarray(Tb, np.int64).copy()
    B = len(Tb)
    rng = np.random.RandomState(seed)
    x = (2.0 * rng.randn(T, B, C)).astype(np.float32)
    y = np.zeros((B, S, C), np.float32)
    y[:, 0] = rng.rand(B, C) < 0.3
    x64 = x.astype(np.float64)
    bce = np.where(y[None, :, 0] > 0, np.logaddexp(0.0, -x64), np.logaddexp(0.0, x64)).mean(axis=2)     # [T,B]; |x| < 100: no clamp
    nll = np.where(np.arange(T)[:, None] < Tb[None, :], bce, 0.0).sum(axis=0)
    L = np.ones(B, np.int64)
    bad = np.zeros(B, bool)
    if no_alignment is not None and len(no_alignment):
        i = np.asarray(no_alignment)
        y[i, 1] = y[i, 0]
        L[i], Tb[i], bad[i] = 2, 1, True
    return Batch(x, y, Tb, L, np.where(bad, np.inf, nll), bad)


def blank_batch(T, C, S, Tb, target, L=None, no_alignment=None, masked=None, nan=None):
    """Blank lattice, every log-prob of sample b at -m_b (used as given): each alignment scores -T_b m_b, and there are 1
    (L_b = 0) or T_b (T_b + 1) / 2 (L_b = 1) of them: nll_b = T_b m_b - ln(count).  Label 1 + b % (C - 1), blank 0."""
    B = len(target)
    Tb = _per_sample(Tb, B, np.int64)
    L = _per_sample(np.arange(B) % 2 if L is None else L, B, np.int64)
    count = np.where(L == 0, 1.0, Tb * (Tb + 1) / 2.0)
    m = ((np.asarray(target, np.float64) + np.log(count)) / Tb).astype(np.float32)
    nll = Tb * m.astype(np.float64) - np.log(count)
    tgt = np.zeros((B, S), np.int64)
    tgt[:, 0] = 1 + np.arange(B) % (C - 1)
    x = np.broadcast_to(-m[None, :, None], (T, B, C)).copy()
    bad = np.zeros(B, bool)
    if no_alignment is not None and len(no_alignment):
        i = np.asarray(no_alignment)
        tgt[i, 1] = tgt[i, 0]                                  # a repeat: three frames needed, one given
        L[i], Tb[i], bad[i] = 2, 1, True
    if masked is not None and len(masked):
        i = np.asarray(masked)
        L[i] = 1
        x[:, i, tgt[i, 0]] = -np.inf
        bad[i] = True
    if nan is not None and len(nan):
        x[0, np.asarray(nan), 0] = np.nan
    nll = np.where(bad, np.inf, nll)
    return Batch(x, tgt, Tb, L, nll, bad)


BUILDERS = {"noblank": noblank_batch, "binary": binary_batch, "blank": blank_batch}

# ---- the value regimes ----------------------------------------------------------------------------------------------
BELOW, ABOVE = (0.5, 2.0, 50.0), (0.5, 2.0, 50.0, 800.0)


def ragged_lengths(B, T, lo=None):
    """T_b in [lo, T], every length present once B allows it, a different one on neighbouring samples"""
    lo = max(1, T // 2) if lo is None else lo
    return lo + (np.arange(B) * 7 + 3) % (T - lo + 1)


def regime_targets(regime, B):
    """-> nll to ask for, per sample.  `mixed`: consecutive samples cycle through tiny, above, ordinary, below, above: a
    pattern of period 5, coprime to the 16 shards, so the members b, b + 16, b + 32, ... of every shard run through all
    five kinds -- each shard receives fitting and non-fitting values as soon as it has five members (B >= 80)."""
    b = np.arange(B)
    tiny = 1e-4 * (1.0 + (b % 5))
    ordinary = 1.0 + (b * 37 % 500)
    below = ACC_LIMIT - np.asarray(BELOW)[b // 2 % len(BELOW)]
    above = ACC_LIMIT + np.asarray(ABOVE)[b // 2 % len(ABOVE)]
    if regime == "tiny":
        return tiny
    if regime == "ordinary":
        return ordinary
    if regime == "straddling":
        return np.where(b % 2 == 0, below, above)
    if regime == "mixed":
        return np.choose(b % 5, [tiny, above, ordinary, below, above])
    raise ValueError(regime)
