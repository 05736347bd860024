"""The reference's training step end to end on the device -- ``feat`` (also as the transposed view the reference passes, also
bf16) -> ``ctc_amd.LSTM_cell`` in train mode -> ``noblank_ctc_loss`` / ``binary_ctc_loss`` / ``blank_ctc_loss`` ->
``loss.backward()`` -> ``torch.optim.SGD`` -- through the public Python API only, against the float64 CPU autograd of the same
step (tests/train_step_ref.py; its cases, seeds and recorded entries are pinned without a GPU in tests/test_train_step_ref.py).

Every accuracy bound is max(plain, 2 err32): plain an existing constant of the suite (2e-5 absolute for v_series, 1e-5 of
max(1, |nll|) for nll and loss, 1e-4 of max(1, max |ref|) for gradients and parameters, 1e-5 absolute for the running
statistics), err32 the error of the same reference run in float32 on the CPU.  A bf16 d_feat is allowed one more rounding to
bf16 (2^-8 of max |ref|); the forward-only nll is held to the existing 2e-6 relative.  Everything else is exact: the pad column
is PAD_LOGIT and its loss gradient 0, no gradient changes in a bit when something consumes the pad column, two steps from the
same state give the same bits (through the C++ autograd node and through the Python Functions alike), a captured step replays
the eager bits, and the C-ABI entries that ran are exactly the ones tests/train_step_ref.py read off the dispatch code.

Measured on an MI355X: see MEASURED below.  What the assertions hold in place: see MUTATIONS below."""
import collections
import copy
import types

import numpy as np
import pytest
import torch

from tests import train_step_ref as R
from tests.helpers import np_

pytestmark = pytest.mark.gpu

NAMES = list(R.CASES)

MEASURED = """
On an MI355X, on the tree this file was added in (parent commit c4c91f5, no kernel changed): 38 passed in 6 s.  One line per test x
case: the quantity with the largest err / bound of the (rows) quantities it holds to float64, then the largest err / err32.  Units:
absolute (series, running statistics), of max(1, |ref|) (loss, nll), of max(1, max |ref|) (gradients, parameters).  2 err32 exceeds
plain nowhere: every bound below is the plain constant (the bf16 d_feat: plus its one rounding).
what                      rows  worst err / bound                                                          worst err / err32
one step ref33_pad          13  series       err 7.6e-07  err32 3.0e-07  bound 2.0e-05  max|ref| 6.9e-01   loss          4.06
one step ref33_raw          13  series       err 9.5e-07  err32 4.2e-07  bound 2.0e-05  max|ref| 8.0e-01   series        2.28
one step ref33_T            13  series       err 1.1e-06  err32 4.5e-07  bound 2.0e-05  max|ref| 7.0e-01   series        2.48
one step ref33_bf16         13  d_feat       err 3.0e-05  err32 5.9e-09  bound 1.6e-04  max|ref| 1.5e-02   d_feat        (the rounding to bf16)
one step ref33_binary       13  series       err 9.5e-07  err32 4.2e-07  bound 2.0e-05  max|ref| 8.0e-01   loss         12.46
one step c158               13  running_var  err 2.0e-07  err32 2.8e-07  bound 1.0e-05  max|ref| 1.4e+00   nll           3.24
one step c158_binary        13  running_var  err 2.0e-07  err32 2.8e-07  bound 1.0e-05  max|ref| 1.4e+00   d_w_hh        1.63
one step b300               13  series       err 4.0e-07  err32 3.7e-07  bound 2.0e-05  max|ref| 8.6e-01   nll           1.64
one step b520               13  series       err 5.6e-07  err32 4.7e-07  bound 2.0e-05  max|ref| 7.9e-01   d_bn_weight   1.76
one step blank38            13  running_var  err 3.1e-07  err32 4.6e-07  bound 1.0e-05  max|ref| 1.4e+00   running_mean  1.04
one step fallback           13  running_var  err 2.9e-07  err32 3.6e-07  bound 1.0e-05  max|ref| 1.6e+00   nll           2.01
one step smooth34           13  series       err 3.0e-07  err32 2.4e-07  bound 2.0e-05  max|ref| 7.9e-01   nll           1.68
one step fallback_pad       13  running_var  err 3.1e-07  err32 3.1e-07  bound 1.0e-05  max|ref| 1.6e+00   d_bn_weight   2.06
dropout p = 0.3             13  series       err 7.6e-07  err32 4.3e-07  bound 2.0e-05  max|ref| 8.0e-01   d_w_ih        1.97
accumulation (both paths)   10  running_var  err 3.4e-07  err32 5.1e-07  bound 1.0e-05  max|ref| 1.2e+00   running_mean  1.51
two consumers               14  series       err 7.6e-07  err32 3.0e-07  bound 2.0e-05  max|ref| 6.9e-01   loss          4.06
three SGD steps             11  running_var  err 3.8e-07  err32 5.1e-07  bound 1.0e-05  max|ref| 1.3e+00   loss          1.46
eval series                  1  series       err 8.2e-07  err32 4.0e-07  bound 2.0e-05  max|ref| 7.4e-01   series        2.04
eval forward-only nll: 1.9e-07 of max(1, |nll|) against float64 (err32 6.9e-08, bound 2e-06, max |nll| 31.5), 0 against the call with a
gradient.  The gradients are the small quantities here (max |ref| from 7e-04, d_feat of the binary cases, to 2.4, d_w_ih of blank38),
and their errors are 4e-10 ... 1.1e-06: at most 4.6 err32 (d_bn_bias of ref33_binary), 4e-6 ... 1.1e-2 of the 1e-4 they are held to.
Label smoothing behind the pad column (ref33_pad, lambda = 0.9): nll = T_b x 2.94e27 on every sample (2.94e28 at T_b = 10), loss
2.06e28, every gradient finite.
"""

MUTATIONS = """
Four mutations of a scratch copy of the Python layer (wrong numbers or a Python exception, no faults), each run once against this file:
  _SeriesFn.backward reads d_series[t, :, :H + 1] (the BPTT loop)      3 failed, 35 passed: the three tests of fallback_pad, the one
      case where that loop meets a pad column (test_one_step_against_float64, test_same_step_twice_gives_the_same_bits,
      test_no_gradient_depends_on_the_pad_column: a shape error).  The HIP backward (lstm_backward) takes d_series by pointer and
      pitch and reads H columns whatever slice it is handed.
  the loss's scale = 1 / (B + 1) in functional._launch                27 failed, 11 passed: every test_one_step_against_float64 (loss
      and every gradient), dropout, two consumers, accumulation[python]; test_same_step_twice_gives_the_same_bits on all cases but
      blank38 and smooth34 (the C++ autograd node computes its own scale: its bits no longer match the Python Functions').
  B / (B - 1) dropped from the running variance                        16 failed, 22 passed: running_var of every case whose head is
      a HIP launch (0.08 ... 0.12 against 1e-5), dropout, both accumulations, two consumers, SGD; fallback and fallback_pad pass
      (torch's own BatchNorm runs there).
  ctx.grad handed out without the upstream factor (_scaled_grad)       16 failed, 22 passed: accumulation[python] on the numbers
      (d_weight off by 0.14 against 1e-4); made by dropping the ctc_amd_scale_grad call, so the entry counts of the thirteen steps,
      dropout and two consumers fail as well.  accumulation[default] passes: there the C++ node scales.
"""


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    import ctc_amd  # noqa: F401
    return torch.device("cuda:0")


@pytest.fixture
def python_functions(monkeypatch):
    """the losses through the Python Functions of ctc_amd/functional.py instead of the C++ autograd node (the same launches)"""
    from ctc_amd import functional as F
    monkeypatch.setattr(F, "_host_ext", None)


@pytest.fixture
def calls(monkeypatch, python_functions):
    """the name of every C-ABI entry called through _lib.load(), in order (the spy of tests/test_readout_typed_gpu.py, on every
    entry; the size queries *_bytes launch nothing and are left out)"""
    from ctc_amd import _lib
    seen = []
    real = _lib.load()

    class Spy:
        def __getattr__(self, name):
            fn = getattr(real, name)
            if not name.startswith("ctc_amd_") or name.endswith("_bytes"):
                return fn

            def call(*a):
                seen.append(name)
                return fn(*a)
            return call
    monkeypatch.setattr(_lib, "load", lambda: Spy())
    return seen


# ---- the step on the device -------------------------------------------------------------------------------------------------
def _named(model):
    lin, bn, cell = model.v.layers[0], model.v.layers[1], model.v_cell
    return dict(zip(R.PARAMS, (lin.weight, lin.bias, bn.weight, bn.bias, cell.weight_ih, cell.weight_hh, cell.bias_ih, cell.bias_hh)))


def _model(case, dev, p=0.0):
    """ctc_amd.LSTM_cell in train mode on the case's parameters; dropout off unless p is given"""
    import ctc_amd
    args = types.SimpleNamespace(extract_feat_dim=case.K, v_class=case.C, batch_size=case.B, temporal=case.T)
    model = ctc_amd.LSTM_cell(args, pad_classes=case.pad).train()
    prm = R.draw_params(case, R.SEEDS[case.name])
    with torch.no_grad():
        for name, dst in _named(model).items():
            dst.copy_(prm[name])
        model.v.layers[1].running_mean.copy_(prm["running_mean"])
        model.v.layers[1].running_var.copy_(prm["running_var"])
    model.v.layers[3].p = p
    return model.to(dev)


def _zero(model):
    for p in model.parameters():
        p.grad = None


def _state(model):
    out = {}
    for name, p in _named(model).items():
        out[name] = p.detach().clone()
        if p.grad is not None:
            out["d_" + name] = p.grad.detach().clone()
    bn = model.v.layers[1]
    out["running_mean"], out["running_var"] = bn.running_mean.clone(), bn.running_var.clone()
    return out


def _on(batch, dev):
    return types.SimpleNamespace(h0=batch.h0.to(dev), c0=batch.c0.to(dev), Tb=batch.Tb.to(dev), L=batch.L.to(dev),
                                 targets=None if batch.targets is None else batch.targets.to(dev),
                                 rows=None if batch.rows is None else batch.rows.to(dev))


def _loss(case, series, d):
    """-> (loss, nll) as a caller computes them; the binary targets through the recipe of INTEGRATION.md, section 5"""
    import ctc_amd
    if case.loss == "noblank":
        return ctc_amd.noblank_ctc_loss(series, d.targets, d.Tb, d.L, label_smoothing=case.smoothing)
    if case.loss == "binary":
        d.dedup = ctc_amd.dedup_multihot_targets(d.rows, exact_rows=case.exact_rows)
        return ctc_amd.binary_ctc_loss(series, d.dedup[0].clamp(min=0).float(), d.Tb, d.dedup[1])
    return ctc_amd.blank_ctc_loss(series.log_softmax(2), d.targets, d.Tb, d.L, blank=0)


def _step(model, case, batch, dev, accum=None, objective=None):
    """forward, loss, backward on the device -> dict of tensors by the names of tests/train_step_ref.py.  accum: the reference's
    `(loss / accum).backward()`; objective(loss, series): another consumer of the series on top of the loss"""
    leaf = batch.leaf.to(dev, getattr(torch, case.feat)).requires_grad_(True)
    feat = leaf.transpose(0, 1) if case.transposed else leaf
    d = _on(batch, dev)
    series = model(feat, d.h0, d.c0)
    series.retain_grad()
    loss, nll = _loss(case, series, d)
    total = loss if objective is None else objective(loss, series)
    (total if accum is None else total / accum).backward()
    torch.cuda.synchronize()
    out = {"series": series.detach()[:, :, :case.C], "series_cols": series.detach(), "loss": loss.detach(), "nll": nll.detach(),
           "d_series": series.grad, "d_feat": leaf.grad, "lin_bias_grad": model.v.layers[0].bias.grad, "inputs": d}
    out.update(_state(model))
    return out


def _report(rows):
    """rows: (what, err, err32, bound, max |ref|); print every figure, then assert (tests/test_producer_inputs_gpu.py)"""
    for what, err, e32, bound, scale in rows:
        print("%-44s err %.3e  err32 %.3e  err/err32 %8.2f  bound %.3e  max|ref| %.3e"
              % (what, err, e32, err / e32 if e32 > 0 else float("inf") if err > 0 else 0.0, bound, scale))
    for what, err, e32, bound, scale in rows:
        assert err <= bound, (what, err, e32, bound)


def _against_float64(what, got, r, names, lowp_feat=False):
    """every named quantity of `got` against the float64 run r["ref"], bound max(plain, 2 err32) with err32 from r["r32"]"""
    rows = []
    for q, (e32, bound, scale) in R.yardstick(r["ref"], r["r32"], names).items():
        g = got[q]
        g = np_(g.float()).astype(np.float64) if torch.is_tensor(g) else np.asarray(g, np.float64)
        assert np.isfinite(g).all(), (what, q)
        if q == "d_feat" and lowp_feat:                      # the fp32 value rounded once to bf16: half an ulp, 2^-8 of the value
            bound += 2.0 ** -8 * scale / max(1.0, scale)
        rows.append(("%s %s" % (what, q), R.err_of(q, g, r["ref"][q]), e32, bound, scale))
    _report(rows)


def _same_bits(a, b, names):
    for q in names:
        assert (a[q] is None) == (b[q] is None), q
        if a[q] is not None:
            assert a[q].dtype == b[q].dtype and torch.equal(a[q], b[q]), q


BITS = ("series_cols", "loss", "nll", "d_series", "d_feat", "lin_bias_grad") + tuple("d_" + n for n in R.PARAMS) + R.STATS


# ---- one train-mode step per case ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_one_step_against_float64(dev, calls, name):
    case, r = R.CASES[name], R.reference(name)
    got = _step(_model(case, dev), case, r["batch"], dev)
    assert collections.Counter(calls) == collections.Counter(R.ENTRIES[name]), collections.Counter(calls)
    _against_float64(name, got, r, R.QUANTITIES, lowp_feat=case.feat != "float32")
    assert got["d_feat"].dtype is getattr(torch, case.feat) and got["d_feat"].shape == r["batch"].leaf.shape
    assert got["series_cols"].shape == (case.T, case.B, case.cols) and got["series_cols"].dtype is torch.float32
    assert bool(torch.isfinite(got["lin_bias_grad"]).all())  # (identically 0 under batch statistics: its accuracy is not asserted)
    assert torch.equal(got["d_b_ih"], got["d_b_hh"])
    if case.cols > case.C:                                   # the pad column: the constant, and no gradient from the loss
        assert bool((got["series_cols"][:, :, case.C:] == R.PAD_LOGIT).all())
        assert bool((got["d_series"][:, :, case.C:] == 0).all())
    if case.loss == "binary":                                # the device's dedup gives the targets the reference was run on
        tg, ln = got["inputs"].dedup
        assert torch.equal(tg.clamp(min=0).float().cpu(), r["batch"].y) and torch.equal(ln.cpu(), r["batch"].L)
        assert bool((tg[torch.arange(case.S, device=dev)[None, :] >= ln[:, None]] == -1).all())


@pytest.mark.parametrize("name", NAMES)
def test_same_step_twice_gives_the_same_bits(dev, monkeypatch, name):
    """two models from the same state, the same step: identical bits in every output; a third through the Python Functions
    instead of the C++ autograd node (the same launches) as well"""
    from ctc_amd import functional as F
    case, batch = R.CASES[name], R.reference(name)["batch"]
    a = _step(_model(case, dev), case, batch, dev)
    b = _step(_model(case, dev), case, batch, dev)
    monkeypatch.setattr(F, "_host_ext", None)
    c = _step(_model(case, dev), case, batch, dev)
    _same_bits(a, b, BITS)
    _same_bits(a, c, BITS)


@pytest.mark.parametrize("name", [n for n in NAMES if R.CASES[n].cols > R.CASES[n].C and R.CASES[n].feat == "float32"
                                  and not R.CASES[n].transposed])
def test_no_gradient_depends_on_the_pad_column(dev, name):
    """a consumer of the pad column hands _SeriesFn.backward a d_series whose pad column is not 0: no gradient changes in a bit"""
    case, batch = R.CASES[name], R.reference(name)["batch"]
    g = torch.Generator().manual_seed(3)
    w = (torch.rand(case.T, case.B, case.cols - case.C, generator=g) + 0.5).to(dev)
    plain = _step(_model(case, dev), case, batch, dev)
    fed = _step(_model(case, dev), case, batch, dev, objective=lambda loss, series: loss + (series[:, :, case.C:] * w).sum())
    assert torch.equal(fed["d_series"][:, :, case.C:], w) and torch.equal(fed["d_series"][:, :, :case.C], plain["d_series"][:, :, :case.C])
    _same_bits(plain, fed, ("d_feat", "lin_bias_grad") + tuple("d_" + n for n in R.PARAMS) + R.STATS)


# ---- further tests on ref33_pad ----------------------------------------------------------------------------------------------
def test_dropout_with_the_mask_the_module_drew(dev, calls, monkeypatch):
    """p = 0.3: the mask LSTM_cell._head draws with torch.nn.functional.dropout is recorded and fed to the reference"""
    name = "ref33_pad"
    case, batch = R.CASES[name], R.reference(name)["batch"]
    real, masks = torch.nn.functional.dropout, []

    def recording(x, p=0.5, training=True, inplace=False):
        masks.append(real(x, p, training, inplace))
        return masks[-1]
    monkeypatch.setattr(torch.nn.functional, "dropout", recording)
    torch.manual_seed(1234)
    got = _step(_model(case, dev, p=0.3), case, batch, dev)
    assert len(masks) == 1 and masks[0].shape == (case.T, case.B, case.C)
    mask = masks[0].cpu()
    kept = mask != 0
    assert len(mask[kept].unique()) == 1 and abs(float(mask[kept][0]) - 1.0 / 0.7) < 1e-6      # already scaled by 1 / (1 - p)
    assert bool(kept.any()) and not bool(kept.all())
    assert collections.Counter(calls) == collections.Counter(R.ENTRIES[name])
    _against_float64(name + " p=0.3", got, R.masked_reference(name, mask), R.QUANTITIES)
    assert bool((got["series_cols"][:, :, case.C:] == R.PAD_LOGIT).all()) and bool((got["d_series"][:, :, case.C:] == 0).all())


@pytest.mark.parametrize("path", ["default", "python"])
def test_three_micro_steps_accumulate(dev, monkeypatch, path):
    """(loss / 3).backward() on three batches: the upstream factor goes through ctc_amd_scale_grad (or the C++ node's own
    call of it) into the producer's backward, and the gradients add up in the parameters"""
    from ctc_amd import functional as F
    if path == "python":
        monkeypatch.setattr(F, "_host_ext", None)
    name = "ref33_pad"
    case, r = R.CASES[name], R.reference(name, "accum")
    model = _model(case, dev)
    losses = []
    for i in range(3):
        out = _step(model, case, R.draw_batch(case, R.SEEDS[name], i), dev, accum=3)
        losses.append(np_(out["loss"]))
    got = dict(_state(model), loss=np.stack(losses))
    _against_float64("%s accum %s" % (name, path), got, r, ("loss",) + R.GRADS[1:] + R.STATS)


def test_two_consumers_of_the_series(dev, calls):
    """loss + 0.1 * series[T-1, :, :C].logsumexp(1).mean(): d_series arrives at _SeriesFn.backward as autograd's sum"""
    name = "ref33_pad"
    case, r = R.CASES[name], R.reference(name, "two")
    got = _step(_model(case, dev), case, r["batch"], dev,
                objective=lambda loss, series: loss + 0.1 * series[case.T - 1, :, :case.C].logsumexp(1).mean())
    assert collections.Counter(calls) == collections.Counter(R.ENTRIES[name])
    _against_float64(name + " two consumers", got, r, R.QUANTITIES + ("d_series",))
    assert bool((got["d_series"][:, :, case.C:] == 0).all())


def test_three_sgd_steps(dev):
    """torch.optim.SGD, lr 0.1, three steps on one batch: per-step loss, the final parameters and the running statistics against
    the float64 trajectory from the same state (err32: the float32 CPU trajectory); the loss falls"""
    name = "ref33_pad"
    case, r = R.CASES[name], R.reference(name, "sgd")
    model = _model(case, dev)
    opt = torch.optim.SGD(model.parameters(), lr=0.1)
    losses = []
    for _ in range(3):
        opt.zero_grad(set_to_none=True)
        losses.append(np_(_step(model, case, r["batch"], dev)["loss"]))
        opt.step()
    got = dict(_state(model), loss=np.stack(losses))
    _against_float64(name + " sgd", got, r, ("loss",) + R.PARAMS + R.STATS)
    assert losses[0] > losses[1] > losses[2] and r["ref"]["loss"][0] > r["ref"]["loss"][1] > r["ref"]["loss"][2]
    assert int(model.v.layers[1].num_batches_tracked) == 3 * case.T


@pytest.mark.parametrize("name", ["ref33_pad", "b520"])
def test_captured_step_replays_the_eager_bits(dev, name):
    """forward + loss + backward captured into one torch.cuda.graph after two warm-ups on the side stream, replayed on two new
    feat copied into the static input: series, loss, every gradient and the running statistics are those of an eager clone of
    the model stepped through the same inputs"""
    import ctc_amd
    case, seed = R.CASES[name], R.SEEDS[name]
    batch = R.reference(name)["batch"]
    d = _on(batch, dev)
    feats = [R.draw_batch(case, seed, i).leaf.to(dev) for i in range(3)]
    captured_model = _model(case, dev)
    eager_model = copy.deepcopy(captured_model)

    def step(model, leaf):
        _zero(model)
        leaf.grad = None
        series = model(leaf, d.h0, d.c0)
        loss, nll = _loss(case, series, d)
        loss.backward()
        return series, loss, nll

    static = feats[0].clone().requires_grad_(True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step(captured_model, static)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    _zero(captured_model)
    static.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        cap = step(captured_model, static)
    for _ in range(2):
        step(eager_model, feats[0].clone().requires_grad_(True))
    for i in (1, 2):
        with torch.no_grad():
            static.copy_(feats[i])
        graph.replay()
        torch.cuda.synchronize()
        leaf = feats[i].clone().requires_grad_(True)
        eag = step(eager_model, leaf)
        torch.cuda.synchronize()
        for a, b in zip(cap, eag):
            assert torch.equal(a.detach(), b.detach())
        assert torch.equal(static.grad, leaf.grad)
        _same_bits(_state(captured_model), _state(eager_model), tuple("d_" + n for n in R.PARAMS) + R.PARAMS + R.STATS)
        assert int(captured_model.v.layers[1].num_batches_tracked) == int(eager_model.v.layers[1].num_batches_tracked) == (2 + i) * case.T
    assert ctc_amd.workspace_status() == 0


def _levenshtein(a, b):
    row = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        prev, row[0] = row[0], i
        for j, y in enumerate(b, 1):
            prev, row[j] = row[j], min(row[j] + 1, row[j - 1] + 1, prev + (x != y))
    return row[-1]


def test_eval_loop(dev, calls):
    """model.eval() under no_grad at T = 10: one launch from feat to v_series; the forward-only loss; the greedy decode and the
    label error rate on the device against a Python loop over the device's own argmax"""
    import ctc_amd
    name = "ref33_pad"
    case, r = R.CASES[name], R.reference(name, "eval")
    batch = R.reference(name)["batch"]
    d = _on(batch, dev)
    model = _model(case, dev).eval()
    with torch.no_grad():
        series = model(batch.leaf.to(dev), d.h0, d.c0)
        loss, nll = ctc_amd.noblank_ctc_loss(series, d.targets, d.Tb, d.L)
    torch.cuda.synchronize()
    assert collections.Counter(calls) == collections.Counter(R.EVAL_ENTRIES), collections.Counter(calls)
    assert not series.requires_grad and bool((series[:, :, case.C:] == R.PAD_LOGIT).all())
    _against_float64(name + " eval", {"series": series[:, :, :case.C]}, r, ("series",))
    with_grad = ctc_amd.noblank_ctc_loss(series.clone().requires_grad_(True), d.targets, d.Tb, d.L)[1].detach()
    ref, r32 = r["ref"]["nll"], r["r32"]["nll"]
    rel = lambda a, b: float((np.abs(a - b) / np.maximum(1.0, np.abs(b))).max())          # noqa: E731
    for what, err in (("forward-only nll against float64", rel(np_(nll).astype(np.float64), ref)),
                      ("forward-only nll against the call with a gradient", rel(np_(nll).astype(np.float64), np_(with_grad).astype(np.float64)))):
        print("%s eval %-52s err %.3e  err32 %.3e  bound %.3e  max|ref| %.3e"
              % (name, what, err, rel(r32, ref), R.NLL_FORWARD_RTOL, float(np.abs(ref).max())))
        assert err <= R.NLL_FORWARD_RTOL, (what, err)
    assert bool(torch.isfinite(loss))
    # series.argmax(-1) -> collapse_frames(blank=None) -> label_error_rate
    frames = series.argmax(-1)                                # [T,B]; the pad column (-1e30) is never the argmax
    hyp = ctc_amd.collapse_frames(frames.t(), d.Tb, blank=None)
    ler, dist = ctc_amd.label_error_rate(hyp.tokens, hyp.lengths, d.targets, d.L)
    fr, Tb, L, tg = np_(frames), np_(batch.Tb), np_(batch.L), np_(batch.targets)
    assert fr.max() < case.C
    want = []
    for b in range(case.B):
        seq = [int(fr[0, b])]
        for t in range(1, int(Tb[b])):
            if int(fr[t, b]) != seq[-1]:
                seq.append(int(fr[t, b]))
        assert int(hyp.lengths[b]) == len(seq) and np_(hyp.tokens)[b, :len(seq)].tolist() == seq
        want.append(_levenshtein(seq, tg[b, :int(L[b])].tolist()))
    assert np_(dist).tolist() == want
    assert float(ler) == float(np.float32(sum(want)) / np.float32(max(int(L.sum()), 1)))


# ---- label smoothing behind a padded producer ---------------------------------------------------------------------------------
def test_label_smoothing_on_a_padded_series_shows_in_the_loss(dev):
    """Every column counts as a class in the smoothed emission, the pad column's lp = -1e30 included (the float64 fact:
    tests/test_train_step_ref.py): behind LSTM_cell(pad_classes=True) every sample reports nll >= 1e12, the library's "no
    alignment", and the gradients stay finite -- a caller's loss log shows the combination; it is not silently wrong.
    (Such a sample's rows of the loss's gradient are exactly 0, as for every sample without an alignment -- asserted in
    tests/test_smoothing_gpu.py; they were (1 - b) softmax - a occupancy - b before that rule reached the smoothed loss.)"""
    import ctc_amd
    name = "ref33_pad"
    case, batch = R.CASES[name], R.reference(name)["batch"]
    d = _on(batch, dev)
    model = _model(case, dev)
    feat = batch.leaf.to(dev).requires_grad_(True)
    series = model(feat, d.h0, d.c0)
    series.retain_grad()
    assert series.shape[2] == case.C + 1
    loss, nll = ctc_amd.noblank_ctc_loss(series, d.targets, d.Tb, d.L, label_smoothing=0.9)
    loss.backward()
    torch.cuda.synchronize()
    print("smoothed nll behind the pad column:", np_(nll).tolist(), "loss", float(loss.detach()))
    assert bool((nll >= R.NO_ALIGNMENT).all()) and not bool(torch.isnan(nll).any())
    for g in (series.grad, feat.grad, *(p.grad for p in model.parameters())):
        assert g is not None and bool(torch.isfinite(g).all())
    with pytest.raises(ctc_amd.CtcAmdError):                 # and the unpadded odd C is outside the smoothed kernel
        ctc_amd.noblank_ctc_loss(series.detach()[:, :, :case.C].contiguous(), d.targets, d.Tb, d.L, label_smoothing=0.9)
