"""The training step the library exists for -- ``feat.transpose(0, 1)`` -> ``LSTM_cell`` -> a CTC loss -> ``loss.backward()``
-> optimiser step -- as plain torch on the CPU in float64, and the cases of tests/test_train_step_ref.py (no GPU) and
tests/test_train_step_gpu.py (the HIP launches chained as a caller chains them).  A helper, no test.

The reference: ``nn.Linear``, ``nn.BatchNorm1d`` applied frame by frame (the statistics of each frame's batch in train mode,
running statistics updated T times), ReLU, an explicit dropout mask, ``nn.LSTMCell`` stepped T times, the pad column
concatenated as a constant, and the loss as a differentiable torch function: the no-blank lattice with ``logsumexp`` on
``log_softmax`` (with the label-smoothed emission of ``oracle/ctc_numpy.noblank_ctc``), the same lattice on the sigmoid /
BCE-mean emission of ``oracle/ctc_numpy.binary_ctc``, and ``torch.nn.functional.ctc_loss`` on ``series.log_softmax(2)`` with
the reduction of ``ctc_amd.blank_ctc_loss``.  Autograd supplies every gradient.  The same code in float32 is the yardstick
err32; every bound of the GPU file is max(plain, 2 err32), plain an existing constant of the suite (below).

A sum on the device cannot settle a ReLU decision, so every case is drawn from a seed for which no BatchNorm output of the
float64 run lies within ``MARGIN`` of 0 -- the search of tests/test_head_backward_gpu.py, run on the CPU (``find_seed``), the
seed it found a constant here (``SEEDS``); for the tests of several steps the margin holds at every step of the float64
trajectory (``margins``; asserted in tests/test_train_step_ref.py).

One property of the table cannot hold as written: ``c158`` and ``c158_binary`` have T = 6 frames and S = 8 label columns, and
every sample is feasible (L_b <= T_b), so no sample can have L_b = S.  Their fullest sample has L_b = min(S, T) = T_b = 6: one
alignment only.  Every other case has one sample with L_b = S."""
import functools
import math
from typing import NamedTuple, Optional

import numpy as np
import torch

from oracle import ctc_numpy
from tests.head_backward_ref import MARGIN

PAD_LOGIT = -1.0e30                      # ctc_amd.producer.PAD_LOGIT (asserted in tests/test_train_step_ref.py)
NEG = -1.0e13                            # an impossible lattice state: finite (logsumexp's gradient is NaN on (-inf, -inf)), the oracle's
NO_ALIGNMENT = 1e12                      # nll at or beyond: no alignment (include/ctc_amd.h)

# the suite's existing bounds ("plain"), by kind of quantity
SERIES_ATOL = 2e-5                       # tests/test_producer_inputs_gpu.py: the recurrence forward, absolute
NLL_RTOL = 1e-5                          # tests/test_parity_gpu.py, tests/lattice_inputs_ref.py: of max(1, |nll|)
GRAD_TOL = 1e-4                          # TOL of tests/test_head_backward_gpu.py: of max(1, max |ref|)
STAT_ATOL = 1e-5                         # tests/test_producer_gpu.py, tests/test_producer_inputs_gpu.py: running statistics, absolute
NLL_FORWARD_RTOL = 2e-6                  # tests/test_lattice_inputs_gpu.py: a forward-only call against the call with a gradient

GRADS = ("d_feat", "d_weight", "d_bn_weight", "d_bn_bias", "d_w_ih", "d_w_hh", "d_b_ih", "d_b_hh")
PARAMS = ("weight", "bias", "bn_weight", "bn_bias", "w_ih", "w_hh", "b_ih", "b_hh")
STATS = ("running_mean", "running_var")
# what a step is held to; the Linear bias gradient is identically 0 under batch statistics (rounding on both sides) and skipped,
# as tests/test_head_backward_gpu.py and tests/test_producer_inputs_gpu.py skip it
QUANTITIES = ("series", "loss", "nll") + GRADS + STATS
KIND = {"series": "series", "loss": "nll", "nll": "nll", "running_mean": "stat", "running_var": "stat"}
PLAIN = {"series": SERIES_ATOL, "nll": NLL_RTOL, "grad": GRAD_TOL, "stat": STAT_ATOL}


class Case(NamedTuple):
    name: str
    T: int
    B: int
    K: int
    C: int
    S: int
    loss: str = "noblank"                # noblank | binary | blank
    pad: bool = False                    # LSTM_cell(pad_classes=True): odd C gets a pad column
    feat: str = "float32"                # feat's dtype on the device (the reference runs on the rounded values)
    transposed: bool = False             # feat = base[B,T,K].transpose(0, 1), the gradient read on base
    smoothing: Optional[float] = None
    exact_rows: bool = False             # dedup_multihot_targets(rows, exact_rows=True): C > 64

    @property
    def cols(self):
        return self.C + 1 if (self.pad and self.C % 2) else self.C


CASES = {c.name: c for c in (
    Case("ref33_pad", 10, 10, 1024, 33, 5, pad=True),
    Case("ref33_raw", 10, 10, 1024, 33, 5),
    Case("ref33_T", 10, 10, 1024, 33, 5, pad=True, transposed=True),
    Case("ref33_bf16", 10, 10, 1024, 33, 5, pad=True, feat="bfloat16"),
    Case("ref33_binary", 10, 10, 1024, 33, 5, loss="binary"),
    Case("c158", 6, 9, 64, 158, 8),
    Case("c158_binary", 6, 9, 64, 158, 8, loss="binary", exact_rows=True),
    Case("b300", 4, 300, 64, 33, 3, pad=True),
    Case("b520", 3, 520, 32, 34, 2),
    Case("blank38", 30, 4, 64, 38, 6, loss="blank"),
    Case("fallback", 4, 5, 40, 162, 3),
    Case("smooth34", 10, 10, 64, 34, 5, smoothing=0.9),
    # beyond the table: the pad column behind the frame-by-frame recurrence, whose backward is the BPTT loop of torch kernels
    # (the one place where _SeriesFn.backward slices d_series itself)
    Case("fallback_pad", 3, 4, 40, 163, 2, pad=True),
)}

# find_seed(name): the first seed whose margins(name) all reach MARGIN (run on the CPU; asserted in tests/test_train_step_ref.py)
SEEDS = {"ref33_pad": 7, "ref33_raw": 0, "ref33_T": 0, "ref33_bf16": 0, "ref33_binary": 0, "c158": 4, "c158_binary": 4,
         "b300": 8, "b520": 82, "blank38": 0, "fallback": 0, "smooth34": 0, "fallback_pad": 0}

# ---- which C-ABI entries one train-mode step calls, and how often ---------------------------------------------------------
# Read off ctc_amd/producer.py and ctc_amd/functional.py, not off a run.  The size queries (*_bytes) launch nothing and are
# not counted.  Through the Python Functions of functional.py (the C++ autograd node makes the same launches from C++, where
# a spy on _lib.load() does not see them); ctc_amd_scale_grad runs in every backward, also for an upstream gradient of 1.
_HEAD = {"ctc_amd_head_forward": 1, "ctc_amd_head_backward": 1}                     # B <= 256, K % 16 == 0, T B <= 10240
_HEAD_TYPED = {"ctc_amd_head_forward_typed": 1, "ctc_amd_head_backward_typed": 1}   # _feat_call: a 2-byte feat with unit stride
_HEAD_WIDE = {"ctc_amd_head_forward_wide": 1, "ctc_amd_head_backward_wide": 1}      # B > 256, T B <= 20480
_CELL = {"ctc_amd_lstm_series": 1, "ctc_amd_lstm_backward": 1}                      # I + H <= 80, T B <= 38400
# lstm_series is asked first and refuses; then the wide recurrence, I, H <= 160: its backward launch and the bias sums
_CELL_WIDE = {"ctc_amd_lstm_series": 1, "ctc_amd_lstm_series_wide": 1, "ctc_amd_lstm_series_backward_wide": 1,
              "ctc_amd_lstm_bias_grad_wide": 1}
_NOBLANK = {"ctc_amd_noblank_loss_grad": 1, "ctc_amd_scale_grad": 1}
_BINARY = {"ctc_amd_dedup_multihot_targets": 1, "ctc_amd_binary_loss_grad": 1, "ctc_amd_scale_grad": 1}
ENTRIES = {
    "ref33_pad": {**_HEAD, **_CELL, **_NOBLANK},
    "ref33_raw": {**_HEAD, **_CELL, **_NOBLANK},
    "ref33_T": {**_HEAD, **_CELL, **_NOBLANK},
    "ref33_bf16": {**_HEAD_TYPED, **_CELL, **_NOBLANK},
    "ref33_binary": {**_HEAD, **_CELL, **_BINARY},
    "c158": {**_HEAD, **_CELL_WIDE, **_NOBLANK},
    "c158_binary": {**_HEAD, **_CELL_WIDE, **_BINARY},
    "b300": {**_HEAD_WIDE, **_CELL, **_NOBLANK},
    "b520": {**_HEAD_WIDE, **_CELL, **_NOBLANK},
    "blank38": {**_HEAD, **_CELL, "ctc_amd_blank_loss_grad": 1, "ctc_amd_scale_grad": 1},
    # K % 16 != 0: torch's layers frame by frame, no head entry; C > 160: lstm_series refuses, T step launches, BPTT in torch
    "fallback": {"ctc_amd_lstm_series": 1, "ctc_amd_lstm_cell_step": 4, **_NOBLANK},
    "fallback_pad": {"ctc_amd_lstm_series": 1, "ctc_amd_lstm_cell_step": 3, **_NOBLANK},
    "smooth34": {**_HEAD, **_CELL, "ctc_amd_noblank_smoothed_loss_grad": 1, "ctc_amd_scale_grad": 1},
}
# model.eval() under no_grad, 4 T <= 64, B <= 256: one launch from feat to v_series, then the forward-only loss
EVAL_ENTRIES = {"ctc_amd_lstm_forward": 1, "ctc_amd_noblank_loss_grad": 1}
# the no-blank kernel family the loss of each case reaches (asked of the diagnostics build in tests/test_train_step_ref.py):
# even C <= 256, S <= 31, T <= 168 is the four-rows-per-wave kernel (r16), odd C keeps it away (xr); "ps": its persistent form
FAMILY = {"ref33_pad": "r16", "ref33_raw": "xr", "ref33_T": "r16", "ref33_bf16": "r16", "c158": "r16", "b300": "r16",
          "b520": "r16", "fallback": "r16", "fallback_pad": "r16", "smooth34": "r16"}
PERSISTENT = {"b520"}                    # B > 2 x 256 compute units


# ---- the losses, differentiable, in the dtype of `series` -----------------------------------------------------------------
def _lattice_nll(e, Tb, L):
    """e [T,B,S] emissions -> nll [B] = -alpha[T_b - 1, b, L_b - 1] of the stay / advance lattice that starts in state 0"""
    T, B, S = e.shape
    inside = torch.arange(S)[None, :] < L[:, None]
    neg = e.new_full((B, S), NEG)
    alpha = torch.where(torch.arange(S)[None, :] == 0, e[0], neg)
    rows = [alpha]
    for t in range(1, T):
        adv = torch.cat([neg[:, :1], alpha[:, :-1]], dim=1)
        alpha = torch.where(inside, torch.logsumexp(torch.stack([alpha, adv]), dim=0) + e[t], neg)
        rows.append(alpha)
    return -torch.stack(rows)[Tb - 1, torch.arange(B), L - 1]


def noblank_nll(series, lab, Tb, L, smoothing=None):
    T, B, C = series.shape
    lp = series.log_softmax(2)
    idx = lab.long().clamp(min=0)                            # (the -1 of a padding column: a masked cell)
    e = lp.gather(2, idx.unsqueeze(0).expand(T, B, idx.shape[1]))
    if smoothing is not None:                                # oracle/ctc_numpy.noblank_ctc: every column counts as a class
        b = (1.0 - smoothing) / C
        e = (smoothing - b) * e + b * lp.sum(2, keepdim=True)
    return _lattice_nll(e, Tb, L)


def binary_nll(series, y, Tb, L):
    C = series.shape[2]
    y = y.to(series.dtype)
    p = torch.sigmoid(series)
    lpos, lneg = torch.log(p).clamp(min=-100.0), torch.log(1.0 - p).clamp(min=-100.0)
    e = (torch.einsum("tbc,blc->tbl", lpos, y) + torch.einsum("tbc,blc->tbl", lneg, 1.0 - y)) / C
    return _lattice_nll(e, Tb, L)


def blank_nll(series, tg, Tb, L):
    return torch.nn.functional.ctc_loss(series.log_softmax(2), tg.long(), Tb, L, blank=0, reduction="none")


def loss_of(case, series, batch):
    """-> (loss, nll [B]): the mean over the batch (the blank loss: of nll_b / max(L_b, 1), as ctc_amd.blank_ctc_loss)"""
    if case.loss == "noblank":
        nll = noblank_nll(series, batch.targets, batch.Tb, batch.L, case.smoothing)
    elif case.loss == "binary":
        nll = binary_nll(series, batch.y, batch.Tb, batch.L)
    else:
        nll = blank_nll(series, batch.targets, batch.Tb, batch.L)
        return (nll / batch.L.clamp(min=1).to(nll.dtype)).mean(), nll
    return nll.mean(), nll


# ---- the draws ------------------------------------------------------------------------------------------------------------
def draw_params(case, seed):
    """float32 parameters and running statistics, seeded: the scales of tests/test_head_backward_gpu.py"""
    g = torch.Generator().manual_seed(10007 * seed + 1)
    rnd = lambda *s: torch.rand(*s, generator=g) * 2 - 1          # noqa: E731
    C, K = case.C, case.K
    return {"weight": rnd(C, K) * (3.0 / math.sqrt(K)), "bias": rnd(C) * 0.1, "bn_weight": rnd(C) * 0.5 + 1.0,
            "bn_bias": rnd(C) * 0.2, "running_mean": rnd(C) * 0.3, "running_var": rnd(C) * 0.4 + 1.0,
            "w_ih": rnd(4 * C, C) * (2.0 / math.sqrt(C)), "w_hh": rnd(4 * C, C) * (2.0 / math.sqrt(C)),
            "b_ih": rnd(4 * C) * 0.1, "b_hh": rnd(4 * C) * 0.1}


class Batch(NamedTuple):
    leaf: torch.Tensor                   # float32 [T,B,K], or [B,T,K] for a transposed case; already rounded to case.feat
    h0: torch.Tensor
    c0: torch.Tensor
    targets: Optional[torch.Tensor]      # [B,S] int32 labels, -1 padded (no-blank) / classes 1 .. C-1, 0 padded (blank)
    rows: Optional[torch.Tensor]         # binary: [B,S,C] int32 multi-hot rows as the dataset holds them, duplicates included
    y: Optional[torch.Tensor]            # binary: dedup_multihot_targets(rows)[0].clamp(min=0).float()
    Tb: torch.Tensor
    L: torch.Tensor


def _lengths(case, g):
    """ragged: sample 0 is full (T_b = T, L_b = min(S, T)), sample 1 has L_b = 1 and T_b < T, the rest are drawn with
    1 <= L_b <= T_b <= T; the last sample has T_b < T and more than one alignment where the shape allows"""
    T, B, S = case.T, case.B, case.S
    top = min(S, T)
    L = torch.randint(1, top + 1, (B,), generator=g)
    Tb = torch.stack([torch.randint(int(l), T + 1, (1,), generator=g)[0] for l in L])
    L[0], Tb[0] = top, T
    L[1], Tb[1] = 1, max(1, T // 2)
    L[B - 1] = min(int(L[B - 1]), max(1, T - 2))
    Tb[B - 1] = T - 1
    return Tb.long(), L.long()


def draw_batch(case, seed, index=0):
    """batch `index` of a case: features uniform in [-1, 1), states, lengths and targets; seeded by (seed, index)"""
    g = torch.Generator().manual_seed(1000003 * seed + 101 * index + 7)
    rnd = lambda *s: torch.rand(*s, generator=g) * 2 - 1          # noqa: E731
    T, B, K, C, S = case.T, case.B, case.K, case.C, case.S
    leaf = rnd(B, T, K) if case.transposed else rnd(T, B, K)
    leaf = leaf.to(getattr(torch, case.feat)).float()
    h0, c0 = rnd(B, C) * 0.1, rnd(B, C) * 0.1
    targets = rows = y = None
    if case.loss == "blank":                                 # one L_b = 0, one adjacent repeat, one L_b = 1, one L_b = S
        assert B == 4 and S >= 3
        targets = torch.randint(1, C, (B, S), generator=g, dtype=torch.int32)
        L = torch.tensor([S, 0, 1, 3])
        targets[3, 1] = targets[3, 0]                        # (a, a, b): the repeat needs a blank between, T_b >= L_b + 1
        targets[3, 2] = targets[3, 0] % (C - 1) + 1
        Tb = torch.tensor([T, T // 2, T - 7, 3 * T // 5])
        targets[torch.arange(S)[None, :] >= L[:, None]] = 0
    else:
        Tb, L = _lengths(case, g)
        if case.loss == "noblank":
            targets = torch.randint(0, C, (B, S), generator=g, dtype=torch.int32)
            targets[torch.arange(S)[None, :] >= L[:, None]] = -1
        else:                                                # L_b distinct rows, then rows seen before: the dedup leaves L_b
            hot = min(C, 31)                                 # (the reference's int32 row code: classes 0 .. 30 carry it)
            rows = torch.zeros((B, S, C), dtype=torch.int32)
            for b in range(B):
                seen = set()
                for j in range(int(L[b])):
                    while True:
                        r = (torch.rand(C, generator=g) < 0.15).int()
                        code = tuple(r[:hot].tolist())
                        if any(code) and code not in seen:
                            break
                    seen.add(code)
                    rows[b, j] = r
                for j in range(int(L[b]), S):
                    rows[b, j] = rows[b, int(torch.randint(0, int(L[b]), (1,), generator=g))]
            tg, ln = ctc_numpy.dedup_multihot_targets(rows.numpy(), case.exact_rows)
            assert np.array_equal(ln, L.numpy())
            y = torch.from_numpy(tg).clamp(min=0).float()
    return Batch(leaf, h0, c0, targets, rows, y, Tb, L)


# ---- the model and one step -----------------------------------------------------------------------------------------------
class RefModel:
    """torch's own layers on the CPU in `dtype`, the loop of the reference's LSTM_cell.forward"""

    def __init__(self, case, params, dtype):
        self.case, self.dtype = case, dtype
        C, K = case.C, case.K
        self.lin, self.bn, self.cell = torch.nn.Linear(K, C), torch.nn.BatchNorm1d(C), torch.nn.LSTMCell(C, C)
        with torch.no_grad():
            for dst, key in ((self.lin.weight, "weight"), (self.lin.bias, "bias"), (self.bn.weight, "bn_weight"),
                             (self.bn.bias, "bn_bias"), (self.bn.running_mean, "running_mean"),
                             (self.bn.running_var, "running_var"), (self.cell.weight_ih, "w_ih"), (self.cell.weight_hh, "w_hh"),
                             (self.cell.bias_ih, "b_ih"), (self.cell.bias_hh, "b_hh")):
                dst.copy_(params[key])
        for m in (self.lin, self.bn, self.cell):
            m.to(dtype)
        self.ymin = []                                       # min |BatchNorm output| of every forward

    def named(self):
        return dict(zip(PARAMS, (self.lin.weight, self.lin.bias, self.bn.weight, self.bn.bias, self.cell.weight_ih,
                                 self.cell.weight_hh, self.cell.bias_ih, self.cell.bias_hh)))

    def parameters(self):
        return list(self.named().values())

    def zero_grad(self):
        for p in self.parameters():
            p.grad = None

    def forward(self, feat, h0, c0, mask=None, train=True):
        case = self.case
        self.bn.train(train)
        h, c, hs, ymin = h0.to(self.dtype), c0.to(self.dtype), [], float("inf")
        for t in range(case.T):
            y = self.bn(self.lin(feat[t]))
            ymin = min(ymin, float(y.detach().abs().min()))
            v = torch.relu(y)
            if mask is not None:
                v = v * mask[t].to(self.dtype)
            h, c = self.cell(v, (h, c))
            hs.append(h)
        self.ymin.append(ymin)
        series = torch.stack(hs)
        if case.cols > case.C:
            series = torch.cat([series, series.new_full((case.T, case.B, 1), PAD_LOGIT)], dim=2)
        return series


def ref_step(model, case, batch, mask=None, scale=1.0, second_consumer=False, train=True):
    """forward, loss, backward of (scale x objective) on `model` (gradients accumulate into its parameters) -> dict of float64
    arrays: series, loss, nll, d_series, d_feat (on the leaf: [B,T,K] for a transposed case) and the state after the step.
    second_consumer: the objective is loss + 0.1 * series[T-1, :, :C].logsumexp(1).mean()."""
    leaf = batch.leaf.to(model.dtype).requires_grad_(True)
    feat = leaf.transpose(0, 1) if case.transposed else leaf
    series = model.forward(feat, batch.h0, batch.c0, mask, train)
    series.retain_grad()
    loss, nll = loss_of(case, series, batch)
    total = loss
    if second_consumer:
        total = loss + 0.1 * series[case.T - 1, :, :case.C].logsumexp(1).mean()
    (total * scale).backward()
    # "series": the class columns (the pad column is a constant, compared exactly where it matters); "series_cols": all of them
    out = {"series": series[:, :, :case.C], "series_cols": series, "loss": loss, "nll": nll, "d_series": series.grad,
           "d_feat": leaf.grad, "objective": total}
    out.update(state_of(model))
    return {k: v.detach().double().numpy().copy() for k, v in out.items()}


def state_of(model):
    """the parameter gradients, the parameters and the running statistics of a RefModel, by the names of QUANTITIES / PARAMS"""
    out = {}
    for name, p in model.named().items():
        out[name] = p
        if p.grad is not None:
            out["d_" + name] = p.grad
    out["running_mean"], out["running_var"] = model.bn.running_mean, model.bn.running_var
    return out


# ---- errors and bounds ----------------------------------------------------------------------------------------------------
def kind_of(name):
    return KIND.get(name, "grad")


def err_of(name, got, ref):
    """max |got - ref| in the unit of the quantity's plain bound: absolute (series, running statistics), of max(1, |ref_b|) per
    element (loss, nll), of max(1, max |ref|) (gradients, parameters)"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    d = np.abs(got - ref)
    kind = kind_of(name)
    if kind == "nll":
        return float((d / np.maximum(1.0, np.abs(ref))).max())
    if kind == "grad":
        return float(d.max() / max(1.0, float(np.abs(ref).max())))
    return float(d.max())


def bound_of(name, err32):
    """max(plain, 2 err32): the one form of every accuracy bound of tests/test_train_step_gpu.py"""
    return max(PLAIN[kind_of(name)], 2.0 * err32)


def yardstick(ref, r32, names=QUANTITIES):
    """-> {name: (err32, bound, max |ref|)}"""
    out = {}
    for n in names:
        e32 = err_of(n, r32[n], ref[n])
        out[n] = (e32, bound_of(n, e32), float(np.abs(ref[n]).max()))
    return out


def _frozen(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def _run(name, dtype, what, mask=None):
    """the float64 / float32 run behind every shared reference: `what` names the procedure"""
    case, seed = CASES[name], SEEDS[name]
    model = RefModel(case, draw_params(case, seed), dtype)
    if what == "step":
        r = ref_step(model, case, draw_batch(case, seed), mask)
    elif what == "two":
        r = ref_step(model, case, draw_batch(case, seed), second_consumer=True)
    elif what == "eval":
        with torch.no_grad():
            b = draw_batch(case, seed)
            series = model.forward(b.leaf.to(dtype), b.h0, b.c0, train=False)
            loss, nll = loss_of(case, series, b)
        r = {k: v.double().numpy().copy() for k, v in (("series", series[:, :, :case.C]), ("loss", loss), ("nll", nll))}
    elif what == "accum":                                    # three micro-steps of (loss / 3).backward() on batches 0, 1, 2
        losses = [ref_step(model, case, draw_batch(case, seed, i), scale=1.0 / 3.0)["loss"] for i in range(3)]
        r = {k: v.detach().double().numpy().copy() for k, v in state_of(model).items()}
        r["loss"] = np.stack(losses)
    elif what == "sgd":                                      # three steps of SGD, lr 0.1, on batch 0
        opt = torch.optim.SGD(model.parameters(), lr=0.1)
        losses = []
        for _ in range(3):
            model.zero_grad()
            losses.append(ref_step(model, case, draw_batch(case, seed))["loss"])
            opt.step()
        r = {k: v.detach().double().numpy().copy() for k, v in state_of(model).items()}
        r["loss"] = np.stack(losses)
    else:
        raise KeyError(what)
    r["ymin"] = np.asarray(model.ymin)
    return r


@functools.lru_cache(maxsize=None)
def reference(name, what="step"):
    """computed once and shared (read-only) -> dict(ref: the float64 run, r32: the float32 run, batch): `what` is
    step (one train-mode step on batch 0), two (the same with the second consumer), eval (model.eval(), no gradient),
    accum (three micro-steps, the summed gradients), sgd (three optimiser steps: per-step loss, final parameters)"""
    return {"ref": _frozen(_run(name, torch.float64, what)), "r32": _frozen(_run(name, torch.float32, what)),
            "batch": draw_batch(CASES[name], SEEDS[name])}


def masked_reference(name, mask):
    """one train-mode step under a dropout mask [T,B,C] the caller recorded (already scaled by 1 / (1 - p)); not cached"""
    return {"ref": _run(name, torch.float64, "step", mask), "r32": _run(name, torch.float32, "step", mask)}


MULTI_STEP = ("ref33_pad",)              # the case of the dropout, accumulation, two-consumer, SGD and eval tests


def margins(name, seed=None):
    """min |BatchNorm output| of every float64 forward a test of this case compares against float64 -> {label: value}"""
    case = CASES[name]
    seed = SEEDS[name] if seed is None else seed
    params = draw_params(case, seed)
    model = RefModel(case, params, torch.float64)
    ref_step(model, case, draw_batch(case, seed))
    out = {"step": model.ymin[0]}
    if name in MULTI_STEP:
        for i in (1, 2):                                     # accumulation: batches 1 and 2 on the same parameters
            ref_step(model, case, draw_batch(case, seed, i))
            out["accum%d" % i] = model.ymin[i]
        ev = RefModel(case, params, torch.float64)
        with torch.no_grad():
            b = draw_batch(case, seed)
            ev.forward(b.leaf.double(), b.h0, b.c0, train=False)
        out["eval"] = ev.ymin[0]
        sgd = RefModel(case, params, torch.float64)
        opt = torch.optim.SGD(sgd.parameters(), lr=0.1)
        for i in range(3):
            sgd.zero_grad()
            ref_step(sgd, case, draw_batch(case, seed))
            opt.step()
            out["sgd%d" % i] = sgd.ymin[i]
    return out


def find_seed(name, limit=2000):
    """the search of tests/test_head_backward_gpu.py: the first seed for which no ReLU decision hangs on a rounding"""
    for seed in range(limit):
        if min(margins(name, seed).values()) >= MARGIN:
            return seed
    raise AssertionError("no seed below %d keeps %s %g away from the ReLU's corner" % (limit, name, MARGIN))
