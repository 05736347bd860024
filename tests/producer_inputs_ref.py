"""The producer's input regimes that a real caller produces and a uniform draw at unit scale never does -- saturated gates,
zero padding, constant batch columns, dead units, fp16's range -- as named cases with their float64 reference and the float32
form of that reference, for tests/test_producer_inputs_ref.py (no GPU) and tests/test_producer_inputs_gpu.py (the kernels).
A helper, no test.

Reference: oracle.ctc_numpy.lstm_cell_series / lstm_cell_series_backward and tests/head_forward_ref.head_forward_ref /
tests/head_backward_ref.head_backward_ref, all float64.  ``err32``: the error of the same restatement carried out in float32
(``dtype=np.float32`` for the recurrence, ``head_restated(d, np.float32)`` -- two passes over the batch, numpy's own sum order --
for the head), reduced as the kernels' error is reduced: max |.| for the recurrence's forward, max |.| / max(1, max |ref|) for
every gradient and every output of the head.

Constant columns (the float64 variance of a frame's column <= 1e-10 max(1, mean^2): a zero-padded frame, a dead Linear row, a
repeated sample): x - mean is the rounding of the mean alone there, times up to 1 / sqrt(eps) = 316, so ``err32`` says nothing
about them (it depends on numpy's sum order); ``const_out_bound`` is the bound derived from fp32 itself, and for the backward
``head_restated(d, dtype, state=...)`` runs reference and restatement on the state the kernel saved."""
import functools
import types
import zlib

import numpy as np
import torch

from oracle import ctc_numpy
from tests.head_backward_ref import MARGIN, head_backward_ref
from tests.head_forward_ref import TOL, head_forward_ref

EPS = 1e-5
INV_MAX = 316.3                          # >= 1 / sqrt(eps): the largest invstd a column can have
U32 = 2.0 ** -24                         # fp32's unit roundoff
CAP = 3e-4                               # err32 of every recurrence case, forward and every gradient, stays below
PLAIN_FWD = 2e-5                         # tests/test_lstm_wide_gpu.py: the recurrence's forward, absolute
PLAIN_GRAD = 2e-5                        # ... and its gradients, of max(1, max |ref|)
HEAD_TOL = TOL                           # tests/head_forward_ref.py, tests/test_head_backward_gpu.py: of max(1, max |ref|)
FUSED_DRIVE = {"saturated": 24.0, "extreme": 90.0}     # fused_case: max v x max |w_ih| (extreme: the regime's own 30 x 3)
EXP_RANGE = 88.7                         # fp32's exp overflows beyond

HEAD_REGIMES = ("backbone", "padded", "duplicates", "alternating", "dead")
REC_REGIMES = ("saturated", "forget_open", "padded_tail", "extreme")
HEAD_OUT = ("out", "lin", "mean", "var", "invstd")
HEAD_GRAD = ("d_feat", "d_weight", "d_bias", "d_bn_weight", "d_bn_bias")
REC_GRAD = ("d_x", "dh0", "dc0", "d_w_ih", "d_w_hh", "d_b_ih", "d_b_hh")
LOWP = {"bf16": torch.bfloat16, "fp16": torch.float16}


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def _through(a, lowp):
    """fp32 values that the 2-byte type holds exactly (rounded to nearest even by torch)"""
    return torch.from_numpy(a).to(LOWP[lowp]).float().numpy()


def _bn_bias(u, n):
    """|bn_bias| in [0.05, 0.2]: on a constant column the ReLU decides on it and not on a rounding"""
    v = u(n)
    return (np.where(v < 0, -1.0, 1.0) * (0.05 + 0.15 * np.abs(u(n)))).astype(np.float32)


# ---- the head ---------------------------------------------------------------------------------------------------------

def constant_columns(lin64):
    """[T,C] bool: the columns of a frame the float64 reference calls constant"""
    mean = lin64.mean(1)
    var = ((lin64 - mean[:, None, :]) ** 2).mean(1)
    return var <= 1e-10 * np.maximum(1.0, mean * mean)


def _ref_args(d, train):
    st = {} if train else dict(running_mean=d["running_mean"], running_var=d["running_var"])
    return (d["feat"], d["weight"], d["bias"], d["bn_weight"], d["bn_bias"]), dict(eps=d["eps"], mask=d["mask"], **st)


def head_restated(d, dtype, state=None):
    """forward and backward of the head in ``dtype``, two passes over the batch -> dict of HEAD_OUT + HEAD_GRAD + dlin.
    ``state``: (lin, mean, invstd) to run the backward on instead of the forward's own (the entry's contract: it computes on
    the state it is handed)"""
    a = lambda x: None if x is None else np.asarray(x, dtype)          # noqa: E731
    feat, w, b, g, be, up, mask = (a(d[k]) for k in ("feat", "weight", "bias", "bn_weight", "bn_bias", "d_out", "mask"))
    T, B, K = feat.shape
    C = w.shape[0]
    eps = dtype(np.float32(d["eps"]))
    one = dtype(1.0)
    lin = (feat.reshape(T * B, K) @ w.T).reshape(T, B, C) + b
    train = d.get("running_mean") is None
    if train:
        mean = lin.mean(1, dtype=dtype)
        var = ((lin - mean[:, None, :]) ** 2).mean(1, dtype=dtype)
        inv = one / np.sqrt(var + eps)
        mu, iv = mean[:, None, :], inv[:, None, :]
    else:
        mean, var = a(d["running_mean"]), a(d["running_var"])
        inv = one / np.sqrt(var + eps)
        mu, iv = mean[None, None, :], inv[None, None, :]
    y = (lin - mu) * iv * g + be
    out = np.maximum(y, dtype(0.0))
    if mask is not None:
        out = out * mask
    r = dict(out=out, lin=lin, mean=mean, var=var, invstd=inv)
    if state is not None:
        lin = a(state[0])
        if train:
            mu, iv = a(state[1])[:, None, :], a(state[2])[:, None, :]
        y = (lin - mu) * iv * g + be
    xhat = (lin - mu) * iv
    dy = up * (one if mask is None else mask) * (y > 0)
    db_t, dg_t = dy.sum(1, keepdims=True, dtype=dtype), (dy * xhat).sum(1, keepdims=True, dtype=dtype)
    dlin = iv * g * (dy - db_t / dtype(B) - xhat * dg_t / dtype(B)) if train else dy * g * iv
    flat = dlin.reshape(T * B, C)
    r.update(d_feat=(flat @ w).reshape(T, B, K), d_weight=flat.T @ feat.reshape(T * B, K), d_bias=flat.sum(0, dtype=dtype),
             d_bn_weight=dg_t.sum((0, 1), dtype=dtype), d_bn_bias=db_t.sum((0, 1), dtype=dtype), dlin=dlin)
    return r


def _draw_head(regime, shape, train, with_mask, lowp):
    T, B, K, C = shape
    rng = _rng("head", regime, shape, train, with_mask, lowp)
    u = lambda *s: rng.uniform(-1.0, 1.0, s).astype(np.float32)          # noqa: E731
    f32 = np.float32
    form = "backbone" if (regime, lowp) == ("range16", "bf16") else regime
    wscale = f32(0.25)
    if form == "backbone":                                   # ReLU-sparse, non-negative, tens in magnitude
        feat = (np.maximum(u(T, B, K) - f32(0.2), 0) * f32(30.0)).astype(f32)
    elif form == "duplicates":                               # every sample of a frame is the same row
        feat = np.broadcast_to(u(T, 1, K), (T, B, K)).copy()
    elif form == "alternating":                              # two distinct rows, alternating
        feat = u(T, 2, K)[:, np.arange(B) % 2, :].copy()
    elif form == "range16":                                  # fp16's largest, its subnormals and both zeros, on a third of the rows
        assert lowp == "fp16"
        feat = u(T, B, K)
        rows = np.nonzero(np.arange(B) % 3 == 0)[0]
        for k, val in enumerate((2.0 ** -24, 1023 * 2.0 ** -24, -0.0, 0.0, -(2.0 ** -24), 2.0 ** -15)):
            feat[:, rows, K // 2 + k] = f32(val)
        # one +-65504 per such row, each at a feature of its own among the first K / 2.  (With all of them at one feature the
        # column of lin is two clusters, which BatchNorm maps to +-1 wherever they lie: d_weight of that feature is a sum that
        # cancels to 4e-5 of its terms, and the float32 restatement itself is off by 2e-4 to 1e-2 of max |ref| there -- no
        # yardstick; measured on the device on that draw: err 1.2e-3, err32 2.2e-4 at (4,37,64,40).)
        for n, b in enumerate(rows):
            feat[:, b, n % (K // 2)] = f32(65504.0 if n % 2 == 0 else -65504.0)
        wscale = f32(0.25 * 2.0 ** -10)                      # lin stays finite: |lin| <= 2 x 65504 x 2^-12 + K 2^-12
    else:
        feat = u(T, B, K)
        if form == "padded":                                 # whole trailing frames of zeros; zeros from a length on for half the samples
            feat[T - max(1, T // 4):] = 0
            for b in range(0, B, 2):
                feat[int(rng.integers(1, T)):, b] = 0
    if lowp:
        feat = _through(feat, lowp)
    d = dict(feat=feat, weight=(u(C, K) * wscale).astype(f32), bias=(u(C) * 0.1).astype(f32),
             bn_weight=(u(C) * 0.5 + 1.0).astype(f32), bn_bias=_bn_bias(u, C), eps=EPS, d_out=u(T, B, C))
    col = np.arange(C)
    if form == "dead":
        d["weight"][col % 5 == 0] = 0                        # a dead Linear row: lin == bias
        d["bn_weight"][col % 5 == 1] = 0
        d["bn_weight"][col % 5 == 2] *= -1
        off = np.nonzero(col % 5 == 1)[0]                    # of the dead channels the first is off (relu(bn_bias) = 0), the second on
        d["bn_bias"][off[0]] = -abs(d["bn_bias"][off[0]])
        d["bn_bias"][off[1:2]] = np.abs(d["bn_bias"][off[1:2]])
    if not train:
        d["running_mean"], d["running_var"] = (u(C) * 0.3).astype(f32), (u(C) * 0.4 + 1.0).astype(f32)
        if form == "backbone":                               # the statistics such a backbone's BatchNorm would hold: near the columns' own
            lin = head_forward_ref(d["feat"], d["weight"], d["bias"], d["bn_weight"], d["bn_bias"])[1].reshape(T * B, C)
            d["running_mean"] = (lin.mean(0) + lin.std(0) * d["running_mean"]).astype(f32)
            d["running_var"] = (lin.var(0) * d["running_var"]).astype(f32)
        if form == "dead":
            d["running_var"][col % 5 == 3] = 0
    d["mask"] = ((u(T, B, C) > -0.4).astype(f32) / f32(0.7)) if with_mask else None
    # no ReLU decision on a non-constant column hangs on a rounding: the columns that hold an output within the margin of
    # the corner get another bn_bias.  The margin is MARGIN where the normalised value is of unit scale and grows with
    # |bn_weight| invstd max |lin|, as the fp32 rounding of lin does once it is multiplied by them
    for _ in range(200):
        a, k = _ref_args(d, train)
        out, lin, mean, var, inv = head_forward_ref(*a, **{**k, "mask": None})
        mu, iv = (mean[:, None, :], inv[:, None, :]) if train else (mean, inv)
        y = (lin - mu) * iv * d["bn_weight"] + d["bn_bias"]
        margin = MARGIN * np.maximum(1.0, np.abs(iv * d["bn_weight"]) * np.abs(lin).max(1, keepdims=True))
        close = np.abs(y) < margin
        if train:
            close &= ~constant_columns(lin)[:, None, :]
        bad = np.nonzero(close.any((0, 1)))[0]
        d["bn_bias"][bad] = _bn_bias(u, len(bad))
        thin = []
        if train and form == "alternating":
            # two rows that a Linear row maps almost onto each other: invstd is 1 / their distance, which the fp32 rounding of
            # lin (1e-6 at K = 1024) moves by more than 1e-4 once it exceeds about 40 (measured on the device: 1.08e-4 at
            # invstd = 42, err32 9e-6) -- such a Linear row is drawn again, so that invstd stays below 10
            thin = np.nonzero((inv > 10.0).any(0))[0]
            d["weight"][thin] = (u(len(thin), K) * wscale).astype(f32)
        if not len(bad) and not len(thin):
            break
    else:
        raise AssertionError("no draw clear of the ReLU's corner: %s %s" % (regime, shape))
    return d


@functools.lru_cache(maxsize=None)
def head_case(regime, shape, train, with_mask, lowp=None):
    """-> namespace: d (the fp32 inputs; ``lowp``: feat holds values the 2-byte type represents exactly), fwd / bwd (float64
    references, dicts), const [T,C] (train mode; all False in eval mode), err32 (dict: HEAD_OUT on the non-constant columns,
    HEAD_GRAD), r32 (the float32 restatement)"""
    c = types.SimpleNamespace(regime=regime, shape=shape, train=train, with_mask=with_mask, lowp=lowp)
    c.d = d = _draw_head(regime, shape, train, with_mask, lowp)
    a, k = _ref_args(d, train)
    c.fwd = dict(zip(HEAD_OUT, head_forward_ref(*a, **k)))
    st = dict(mean=c.fwd["mean"], invstd=c.fwd["invstd"]) if train else dict(running_mean=d["running_mean"],
                                                                             running_var=d["running_var"])
    ref = head_backward_ref(d["d_out"], d["feat"], d["weight"], d["bn_weight"], d["bn_bias"], c.fwd["lin"], eps=d["eps"],
                            mask=d["mask"], **st)
    c.bwd = dict(zip(HEAD_GRAD + ("dlin",), ref))
    T, B, K, C = shape
    c.const = constant_columns(c.fwd["lin"]) if train else np.zeros((T, C), bool)
    c.r32 = head_restated(d, np.float32)
    c.err32 = {}
    for name in HEAD_OUT:
        c.err32[name] = head_err(c.r32[name], c.fwd[name], c.const, train)
    for name in HEAD_GRAD:
        c.err32[name] = rel_err(c.r32[name], c.bwd[name])
    return c


def rel_err(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float(np.abs(got - ref).max()) / max(1.0, float(np.abs(ref).max()))


def head_err(got, ref, const, train):
    """max |got - ref| / max(1, max |ref|) over the non-constant columns of a forward output ([T,B,C] or [T,C]; [C] in eval mode)"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if not train and got.ndim == 1:
        keep = np.ones(got.shape, bool)
    else:
        keep = ~(const[:, None, :] if got.ndim == 3 else const) & np.ones(got.shape, bool)
    if not keep.any():
        return 0.0
    return float(np.abs(got - ref)[keep].max()) / max(1.0, float(np.abs(ref)[keep].max()))


def const_out_bound(c):
    """[T,1,C]: the bound on |out - ref| on a constant column, and its square root form for the saved var.  B equal terms
    summed in fp32 in ANY order lose at most B 2^-24 relative, so |x - mean| <= B 2^-24 max |lin_column|; times invstd <= 316.3
    and |bn_weight| (and the mask's factor, which multiplies the output)"""
    T, B, K, C = c.shape
    dev = B * U32 * np.abs(c.fwd["lin"]).max(1, keepdims=True)                   # [T,1,C]
    bound = np.abs(np.asarray(c.d["bn_weight"], np.float64)) * INV_MAX * dev
    if c.d["mask"] is not None:
        bound = bound * np.asarray(c.d["mask"], np.float64)
    return bound, dev[:, 0, :] ** 2


# ---- the recurrence ---------------------------------------------------------------------------------------------------

def _draw_rec(regime, shape):
    T, B, I, H = shape
    rng = _rng("rec", regime, shape)
    u = lambda *s: rng.uniform(-1.0, 1.0, s).astype(np.float32)          # noqa: E731
    f32 = np.float32
    v = (np.maximum(u(T, B, I), 0) * f32(8.0)).astype(f32)
    k_ih = {"saturated": 1.0, "forget_open": 0.3, "padded_tail": 1.0, "extreme": 3.0}[regime]
    d = dict(v=v, h0=u(B, H), c0=u(B, H), w_ih=(u(4 * H, I) * f32(k_ih)).astype(f32), w_hh=(u(4 * H, H) * f32(0.2)).astype(f32),
             b_ih=(u(4 * H) * 0.1).astype(f32), b_hh=(u(4 * H) * 0.1).astype(f32), d_series=u(T, B, H + 1 + H % 2))
    if regime == "forget_open":
        d["b_ih"][H:2 * H] += f32(6.0)
    if regime == "padded_tail":
        d["v"][T // 2:] = 0                                  # the recurrence runs on its own state
    if regime == "extreme":
        d["v"] = (u(T, B, I) * f32(30.0)).astype(f32)
        d["c0"] = np.where(u(B, H) < 0, f32(-20.0), f32(20.0)).astype(f32)       # tanh(c) is exactly +-1 from frame 0
    return d


REC_KEYS = ("v", "h0", "c0", "w_ih", "w_hh", "b_ih", "b_hh")


def rec_reference(d, dtype=np.float64):
    """-> (series [T,B,H], gates [T,B,4H], cells [T+1,B,H], pre-activations' largest magnitude is in gates' inverse; the seven
    gradients of REC_GRAD) in ``dtype``"""
    a = [d[k] for k in REC_KEYS]
    series = ctc_numpy.lstm_cell_series(*a, dtype=dtype)[0]
    H = d["h0"].shape[1]
    grads = ctc_numpy.lstm_cell_series_backward(np.asarray(d["d_series"], dtype)[:, :, :H], *a, dtype=dtype)
    return series, grads


def rec_state(d):
    """float64 gates [T,B,4H], cells [T+1,B,H] and pre-activations [T,B,4H] of the case"""
    v, h, c, w_ih, w_hh, b_ih, b_hh = (np.asarray(d[k], np.float64) for k in REC_KEYS)
    gates, cells, pres = [], [c], []
    for t in range(len(v)):
        pres.append(v[t] @ w_ih.T + b_ih + h @ w_hh.T + b_hh)
        h, c, g = ctc_numpy.lstm_cell_step(v[t], h, c, w_ih, w_hh, b_ih, b_hh)
        gates.append(g)
        cells.append(c)
    return np.stack(gates), np.stack(cells), np.stack(pres)


def _finish_rec(c):
    c.series, grads = rec_reference(c.d)
    c.grads = dict(zip(REC_GRAD, grads))
    s32, g32 = rec_reference(c.d, np.float32)
    c.err32 = {"series": float(np.abs(s32.astype(np.float64) - c.series).max())}
    for name, g in zip(REC_GRAD, g32):
        c.err32[name] = rel_err(g, c.grads[name])
    return c


@functools.lru_cache(maxsize=None)
def rec_case(regime, shape):
    """-> namespace: d (fp32 inputs, d_series at the padded width), series / grads (float64), err32 (dict: series + REC_GRAD)"""
    return _finish_rec(types.SimpleNamespace(regime=regime, shape=shape, d=_draw_rec(regime, shape)))


@functools.lru_cache(maxsize=None)
def fused_case(head_regime, shape, lowp=None, cell="saturated"):
    """an eval-mode head (no mask) of ``head_regime`` in front of a ``saturated`` (or ``extreme``) cell, (T,B,K,C): ->
    namespace with head (a head_case), d (the cell's inputs: v = the float64 head's output), series (float64), err32 (the
    float32 head in front of the float32 recurrence)"""
    T, B, K, C = shape
    c = types.SimpleNamespace(regime=head_regime, shape=shape, head=head_case(head_regime, shape, False, False, lowp))
    c.d = _draw_rec(cell, (T, B, C, C))
    # the head's output stands in for the regime's v <= 8: behind running_var == 0 it reaches 700, where one ulp of v (6e-5)
    # times a w_ih of 1 is already beyond the forward's 2e-5 -- no fp32 arithmetic survives that (measured on the device with
    # w_ih x 1.0: err 4.6e-5, err32 2.0e-5 at (7,9,64,40) dead fp16).  w_ih is scaled so that the largest single product is
    # FUSED_DRIVE: pre-activations still well beyond the 16.7 at which fp32's sigmoid is exactly 1 (extreme: beyond exp's range).
    vmax = float(c.head.fwd["out"].max())
    c.d["w_ih"] = (c.d["w_ih"] * np.float32(FUSED_DRIVE[cell] / (vmax * float(np.abs(c.d["w_ih"]).max())))).astype(np.float32)
    c.d["v"] = None                                          # (the cell's input is the head's output, not a draw)
    a = [c.d[k] for k in REC_KEYS[1:]]
    c.series = ctc_numpy.lstm_cell_series(c.head.fwd["out"], *a)[0]
    s32 = ctc_numpy.lstm_cell_series(c.head.r32["out"], *a, dtype=np.float32)[0]
    c.err32 = float(np.abs(s32.astype(np.float64) - c.series).max())
    return c
