"""tests/producer_inputs_ref.py pinned without a GPU, so that the reference of tests/test_producer_inputs_gpu.py is itself
checked: every case against torch's float64 layers and autograd on the CPU (nn.Linear / BatchNorm1d / ReLU frame by frame,
nn.LSTMCell in a loop; the bounds of tests/test_head_backward_abi.py and tests/test_head_wide_abi.py), the cap on err32, the
property each regime is named for, and no warning from the float32 oracle."""
import warnings

import numpy as np
import pytest
import torch

from oracle import ctc_numpy
from tests import producer_inputs_ref as R

IDS = lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else str(s)          # noqa: E731
REC_SHAPES = [(9, 5, 17, 40), (20, 7, 38, 38), (5, 17, 120, 81), (7, 9, 158, 158), (150, 4, 33, 33), (150, 4, 158, 158)]
HEAD_SHAPES = [(4, 37, 64, 40), (5, 10, 1024, 33), (8, 16, 64, 33), (9, 16, 64, 33), (2, 257, 16, 5), (2, 300, 32, 8)]
FUSED_SHAPES = [(3, 6, 48, 17), (7, 9, 64, 40)]


@pytest.mark.parametrize("regime", R.REC_REGIMES)
@pytest.mark.parametrize("shape", REC_SHAPES, ids=IDS)
def test_recurrence_case(shape, regime):
    T, B, I, H = shape
    with warnings.catch_warnings():
        warnings.simplefilter("error")                       # the float32 oracle overflows its exp silently, to the right 0
        c = R.rec_case(regime, shape)
    d = c.d
    # torch's float64 LSTMCell in a loop, autograd
    cell = torch.nn.LSTMCell(I, H).double()
    with torch.no_grad():
        for p, k in ((cell.weight_ih, "w_ih"), (cell.weight_hh, "w_hh"), (cell.bias_ih, "b_ih"), (cell.bias_hh, "b_hh")):
            p.copy_(torch.from_numpy(d[k]).double())
    v, h0, c0 = (torch.from_numpy(d[k]).double().requires_grad_(True) for k in ("v", "h0", "c0"))
    h, cc, rows = h0, c0, []
    for t in range(T):
        h, cc = cell(v[t], (h, cc))
        rows.append(h)
    series = torch.stack(rows)
    (series * torch.from_numpy(d["d_series"]).double()[:, :, :H]).sum().backward()
    assert np.abs(series.detach().numpy() - c.series).max() <= 1e-12
    want = (v.grad, h0.grad, c0.grad, cell.weight_ih.grad, cell.weight_hh.grad, cell.bias_ih.grad, cell.bias_hh.grad)
    for name, w in zip(R.REC_GRAD, want):
        assert np.abs(w.numpy() - c.grads[name]).max() <= 1e-10 * max(1.0, float(np.abs(c.grads[name]).max())), name
    # the cap: a case beyond it has no float32 yardstick
    print("%s %s: err32 fwd %.2e, grads %.2e" % (shape, regime, c.err32["series"], max(c.err32[n] for n in R.REC_GRAD)))
    for name, e in c.err32.items():
        assert e <= R.CAP, (name, e)
    # the property the regime is named for
    gates, cells, pre = R.rec_state(d)
    g32 = gates.astype(np.float32)
    share = float((np.abs(c.series) > 0.99).mean())
    exact = float(np.concatenate([(g32[:, :, :2 * H] == 0) | (g32[:, :, :2 * H] == 1), np.abs(g32[:, :, 2 * H:3 * H]) == 1], 2).mean())
    print("%s %s: |h| > 0.99 %.3f, gates exactly 0 / 1 in fp32 %.3f, max |pre| %.0f, max |c| %.1f"
          % (shape, regime, share, exact, np.abs(pre).max(), np.abs(cells).max()))
    if regime != "forget_open":                              # (its input weights are the mild ones: the bias opens the gate)
        assert np.abs(pre).max() > 16.7 and exact > 0.01     # sigmoid rounds to exactly 1 in fp32 beyond 24 ln 2
    if regime in ("saturated", "forget_open") and T == 150:
        assert share >= 0.02
    if regime == "forget_open":                              # the cell state accumulates: beyond anything tanh resolves
        assert np.abs(cells).max() > (50.0 if T == 150 else 5.0)
        assert float(gates[:, :, H:2 * H].mean()) > 0.75
    if regime == "padded_tail":
        assert not d["v"][T // 2:].any() and d["v"][:T // 2].any()
    if regime == "extreme":
        assert pre.max() > R.EXP_RANGE and pre.min() < -R.EXP_RANGE
        assert bool((np.abs(d["c0"]) == 20).all()) and bool((np.tanh(d["c0"]) == np.sign(d["c0"])).all())
    else:
        assert np.abs(d["w_hh"]).max() <= 0.2


def _torch_head(d, train):
    """torch's float64 layers frame by frame and autograd -> out, lin, (mean, var per frame), gradients"""
    T, B, K = d["feat"].shape
    C = d["weight"].shape[0]
    lin, bn = torch.nn.Linear(K, C).double(), torch.nn.BatchNorm1d(C, eps=float(np.float32(d["eps"]))).double()
    with torch.no_grad():
        lin.weight.copy_(torch.from_numpy(d["weight"])); lin.bias.copy_(torch.from_numpy(d["bias"]))
        bn.weight.copy_(torch.from_numpy(d["bn_weight"])); bn.bias.copy_(torch.from_numpy(d["bn_bias"]))
        if not train:
            bn.running_mean.copy_(torch.from_numpy(d["running_mean"])); bn.running_var.copy_(torch.from_numpy(d["running_var"]))
    bn.train(train)
    f = torch.from_numpy(d["feat"]).double().requires_grad_(True)
    lins = [lin(f[t]) for t in range(T)]
    out = torch.relu(torch.stack([bn(x) for x in lins]))
    if d["mask"] is not None:
        out = out * torch.from_numpy(d["mask"]).double()
    (out * torch.from_numpy(d["d_out"]).double()).sum().backward()
    return out.detach().numpy(), torch.stack(lins).detach().numpy(), [f.grad, lin.weight.grad, lin.bias.grad, bn.weight.grad,
                                                                      bn.bias.grad]


@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("regime", R.HEAD_REGIMES)
@pytest.mark.parametrize("shape", HEAD_SHAPES, ids=IDS)
def test_head_case(shape, regime, train):
    T, B, K, C = shape
    for with_mask in (True, False):
        c = R.head_case(regime, shape, train, with_mask)
        d = c.d
        out, lins, grads = _torch_head(d, train)
        scale = max(1.0, float(np.abs(c.fwd["out"]).max()))
        # (a constant column: both sides round the float64 mean of B equal terms, B 2^-53 relative, times |bn_weight| 316 x mask)
        noise = float(np.abs(d["bn_weight"]).max()) * R.INV_MAX * B * 2.0 ** -53 * float(np.abs(lins).max()) / 0.7 if c.const.any() else 0.0
        assert np.abs(out - c.fwd["out"]).max() <= 1e-12 * scale + 2 * noise
        assert np.abs(lins - c.fwd["lin"]).max() <= 1e-12 * max(1.0, float(np.abs(lins).max()))
        for name, g in zip(R.HEAD_GRAD, grads):
            ref = c.bwd[name]
            scale = max(1.0, float(np.abs(ref).max()))
            if train and name == "d_bias":                   # identically 0 under batch statistics: the scale is that of the summed terms
                scale = max(1.0, float(np.abs(c.bwd["dlin"]).sum((0, 1)).max()))
            assert np.abs(g.numpy() - ref).max() <= 1e-10 * scale, name
        # the restatement written here, carried out in float64, is the reference
        r64 = R.head_restated(d, np.float64)
        for name in R.HEAD_OUT:
            assert np.abs(r64[name] - c.fwd[name]).max() <= 1e-12 * max(1.0, float(np.abs(c.fwd[name]).max())), name
        for name in R.HEAD_GRAD + ("dlin",):
            assert np.abs(r64[name] - c.bwd[name]).max() <= 1e-10 * max(1.0, float(np.abs(c.bwd[name]).max())), name
        # on the non-constant columns the float32 restatement stays at fp32's own error
        for name in R.HEAD_OUT:
            assert c.err32[name] <= R.HEAD_TOL, (name, c.err32[name])
        if not c.const.any() and regime != "alternating":
            for name in R.HEAD_GRAD:
                if not (train and name == "d_bias"):         # identically 0 under batch statistics: rounding noise alone
                    assert c.err32[name] <= 4e-6, (name, c.err32[name])
        assert np.abs(d["bn_bias"]).min() >= 0.05
    # the property the regime is named for
    zeros = float((d["feat"] == 0).mean())
    nconst = int(c.const.sum())
    print("%s %s %s: %d constant columns of %d, %.2f of feat zero, max |lin| %.1f"
          % (shape, regime, "train" if train else "eval", nconst, T * C, zeros, np.abs(c.fwd["lin"]).max()))
    col = np.arange(C)
    if regime == "backbone":
        assert 0.55 <= zeros <= 0.65 and d["feat"].min() == 0 and 20 < d["feat"].max() <= 24 and nconst == 0
        if K == 1024:
            assert np.abs(c.fwd["lin"]).max() > 100
            assert float(np.abs(c.fwd["lin"].mean(1)).mean()) > 5          # a common offset per column
    if regime == "padded":
        tail = max(1, T // 4)
        assert not d["feat"][T - tail:].any()
        assert nconst == (tail * C if train else 0) and (not train or bool(c.const[T - tail:].all()))
        assert bool((c.fwd["lin"][T - tail:] == d["bias"].astype(np.float64)).all())
        assert zeros > 0.25
    if regime == "duplicates":
        assert bool((d["feat"] == d["feat"][:, :1]).all()) and nconst == (T * C if train else 0)
    if regime == "alternating":
        assert bool((d["feat"][:, 2:] == d["feat"][:, :-2]).all()) and not bool((d["feat"][:, 0] == d["feat"][:, 1]).all())
        assert nconst == 0
    if regime == "dead":
        assert not d["weight"][col % 5 == 0].any() and not d["bn_weight"][col % 5 == 1].any()
        assert bool((d["bn_weight"][col % 5 == 2] < 0).all())
        assert nconst == (T * int((col % 5 == 0).sum()) if train else 0)
        if not train:
            assert not d["running_var"][col % 5 == 3].any() and (col % 5 == 3).any()
            assert np.allclose(c.fwd["invstd"][col % 5 == 3], 1.0 / np.sqrt(np.float64(np.float32(R.EPS))))


@pytest.mark.parametrize("lowp", ["fp16", "bf16"])
@pytest.mark.parametrize("shape", [(4, 37, 64, 40), (2, 300, 32, 8)], ids=IDS)
def test_range16_case(shape, lowp):
    for train in (True, False):
        c = R.head_case("range16", shape, train, True, lowp)
        feat = c.d["feat"]
        t = torch.from_numpy(feat).to(R.LOWP[lowp])
        assert torch.equal(t.float(), torch.from_numpy(feat))                # the 2-byte type holds every value exactly
        assert np.isfinite(c.fwd["lin"]).all() and np.isfinite(c.bwd["d_weight"]).all()
        if lowp == "fp16":
            a = np.abs(feat)
            assert (feat == 65504).any() and (feat == -65504).any()
            assert ((a > 0) & (a < 2.0 ** -14)).any() and (a == 2.0 ** -24).any()          # fp16 subnormals, the smallest among them
            assert (np.signbit(feat) & (feat == 0)).any() and (~np.signbit(feat) & (feat == 0)).any()
            assert np.abs(c.fwd["lin"]).max() < 65504
        else:
            assert 0.55 <= float((feat == 0).mean()) <= 0.65 and feat.max() > 20
        for name in R.HEAD_OUT:
            assert c.err32[name] <= R.HEAD_TOL, (name, c.err32[name])


@pytest.mark.parametrize("cell", ["saturated", "extreme"])
@pytest.mark.parametrize("regime", ["dead", "backbone"])
@pytest.mark.parametrize("shape", FUSED_SHAPES, ids=IDS)
def test_fused_case(shape, regime, cell):
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        c = R.fused_case(regime, shape, None, cell)
    print("%s %s: err32 %.2e, max v %.1f" % (shape, regime, c.err32, c.head.fwd["out"].max()))
    assert c.err32 <= R.CAP and np.isfinite(c.series).all()
    assert c.head.d["mask"] is None and not c.head.train
    pre = c.head.fwd["out"] @ c.d["w_ih"].astype(np.float64).T          # the cell behind the head is still a saturated one
    assert np.abs(pre).max() > (16.7 if cell == "saturated" else R.EXP_RANGE)
    assert np.abs(c.head.fwd["out"]).max() * np.abs(c.d["w_ih"]).max() <= R.FUSED_DRIVE[cell] * (1 + 1e-6)


def test_float32_oracle_does_not_warn_and_keeps_its_values():
    """oracle.ctc_numpy.lstm_cell_step in float32 on pre-activations beyond exp's range: no warning, exact 0 / 1 gates, and on
    inputs inside the range the values of the plain expression bit for bit"""
    rng = np.random.default_rng(0)
    u = lambda *s: rng.uniform(-1.0, 1.0, s).astype(np.float32)          # noqa: E731
    x, h, c = u(3, 4) * 100, u(3, 5), u(3, 5)
    w_ih, w_hh, b = u(20, 4) * 3, u(20, 5) * 0.2, u(20) * 0.1
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        hn, cn, g = ctc_numpy.lstm_cell_step(x, h, c, w_ih, w_hh, b, b, dtype=np.float32)
    assert hn.dtype == np.float32 and np.isfinite(hn).all() and np.isfinite(cn).all()
    assert (g[:, :10] == 0).any() and (g[:, :10] == 1).any() and g[:, :10].min() >= 0 and g[:, :10].max() <= 1
    for dtype in (np.float32, np.float64):
        xs = (x * np.float32(0.01)).astype(np.float32)
        hn, cn, g = ctc_numpy.lstm_cell_step(xs, h, c, w_ih, w_hh, b, b, dtype=dtype)
        a = [np.asarray(t, dtype) for t in (xs, h, c, w_ih, w_hh, b, b)]
        pre = a[0] @ a[3].T + a[5] + a[1] @ a[4].T + a[6]
        sig = lambda v: 1.0 / (1.0 + np.exp(-v))          # noqa: E731
        want = np.concatenate([sig(pre[:, :5]), sig(pre[:, 5:10]), np.tanh(pre[:, 10:15]), sig(pre[:, 15:])], axis=1)
        assert g.dtype == dtype and np.array_equal(g, want)
