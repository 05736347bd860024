"""The eval-mode producer as ONE launch (ctc_amd_lstm_forward): feat -> v_series with the head's output kept
in LDS.  Bit for bit the two launches it replaces (ctc_amd_head_forward on the running statistics, ctc_amd_lstm_series),
at the smallest shapes that reach each seam of the tiling; the reference's own module through the stored fixture; when
LSTM_cell.forward takes the path and when it must not; the shapes the entry refuses; stream capture."""
import types

import numpy as np
import pytest
import torch

from tests.helpers import np_

pytestmark = pytest.mark.gpu

# (T, B, K, C): one frame / one sample / a single 16-block of k (odd block count) / a column tile that is mostly padding;
# B not a multiple of 4, three 16-blocks, C = one tile + 1, 12 < 16 rows; an exact column tile, one full row tile + a
# partial one; the reference's sizes; the largest C the entry takes (2 C = 80)
SHAPES = [(1, 1, 16, 5), (3, 6, 48, 17), (5, 4, 32, 16), (10, 10, 1024, 33), (7, 9, 64, 40)]
REF = (10, 10, 1024, 33)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    import ctc_amd  # noqa: F401
    return torch.device("cuda:0")


def _inputs(dev, T, B, K, C, seed=None):
    """random parameters, running statistics of a trained head (means != 0, variances in [0.5, 2])"""
    g = torch.Generator().manual_seed(sum((T, B, K, C)) if seed is None else seed)
    rnd = lambda *s: (torch.rand(*s, generator=g) * 2 - 1).to(dev)          # noqa: E731
    head = dict(weight=rnd(C, K) * (3.0 / K) ** 0.5, bias=rnd(C), bn_weight=0.5 + rnd(C).abs(), bn_bias=0.3 * rnd(C),
                running_mean=0.5 * rnd(C) + 0.1, running_var=(0.5 + 1.5 * torch.rand(C, generator=g)).to(dev), eps=1e-5)
    cell = dict(h0=rnd(B, C), c0=rnd(B, C), w_ih=0.4 * rnd(4 * C, C), w_hh=0.4 * rnd(4 * C, C), b_ih=rnd(4 * C), b_hh=rnd(4 * C))
    return rnd(T, B, K), head, cell


def _two_launches(feat, head, cell, cols, want_backward_state=False):
    import ctc_amd
    v_all = ctc_amd.head_forward(feat, head["weight"], head["bias"], head["bn_weight"], head["bn_bias"],
                                 head["running_mean"], head["running_var"], head["eps"])[0]
    return ctc_amd.lstm_series(v_all, *cell.values(), cols, want_backward_state=want_backward_state)


def _one_launch(feat, head, cell, cols):
    import ctc_amd
    return ctc_amd.lstm_forward(feat, *head.values(), *cell.values(), cols)


@pytest.mark.parametrize("shape", SHAPES)
def test_bit_identical_to_the_two_launches(dev, shape):
    from ctc_amd import producer
    T, B, K, C = shape
    feat, head, cell = _inputs(dev, *shape)
    for cols in (C, C + 1):
        got = _one_launch(feat, head, cell, cols)
        assert got is not None and got.shape == (T, B, cols), shape
        want = _two_launches(feat, head, cell, cols)[0]
        torch.cuda.synchronize()
        assert torch.equal(got, want), (shape, cols, float((got - want).abs().max()))
        assert torch.isfinite(got[:, :, :C]).all() and float(got[:, :, :C].abs().max()) > 0
        if cols > C:
            assert (got[:, :, C:] == producer.PAD_LOGIT).all()


def test_strided_feat_view(dev):
    """feat = big[:T, ::2] of a [T + 2, 2 B, K] tensor: both strides differ from the dense ones, nothing is copied"""
    T, B, K, C = 3, 6, 48, 17
    _, head, cell = _inputs(dev, T, B, K, C)
    big = torch.randn(T + 2, 2 * B, K, generator=torch.Generator().manual_seed(11)).to(dev)
    view = big[:T, ::2]
    assert view.stride() == (2 * B * K, 2 * K, 1)
    got = _one_launch(view, head, cell, C)
    torch.cuda.synchronize()
    assert torch.equal(got, _two_launches(view, head, cell, C)[0])
    assert torch.equal(got, _one_launch(view.contiguous(), head, cell, C))


@pytest.mark.parametrize("shape", [(3, 6, 48, 17), REF])
def test_final_state_through_the_c_abi(dev, shape):
    """h_out / c_out: the last row of v_series and the cell state after the last frame, bit for bit"""
    from ctc_amd import _lib
    from ctc_amd import functional as F
    T, B, K, C = shape
    feat, head, cell = _inputs(dev, *shape)
    series = torch.empty(T, B, C + 1, device=dev)
    h_out, c_out = torch.full((B, C), 7.0, device=dev), torch.full((B, C), 7.0, device=dev)
    ptrs = [head[k].data_ptr() for k in ("weight", "bias", "bn_weight", "bn_bias", "running_mean", "running_var")]
    rc = _lib.load().ctc_amd_lstm_forward(feat.data_ptr(), feat.stride(0), feat.stride(1), *ptrs, head["eps"],
                                          *(t.data_ptr() for t in cell.values()), T, B, K, C, series.data_ptr(), series.stride(0),
                                          series.stride(1), C + 1, -1.0e30, h_out.data_ptr(), c_out.data_ptr(), F._stream_handle(dev))
    assert rc == 0
    want, _, cells = _two_launches(feat, head, cell, C + 1, want_backward_state=True)
    torch.cuda.synchronize()
    assert torch.equal(series, want)
    assert torch.equal(h_out, series[-1, :, :C]) and torch.equal(c_out, cells[T])


# ---- the module -----------------------------------------------------------------------------------------------------

def _args(feat=1024, C=33, B=10, T=10):
    return types.SimpleNamespace(extract_feat_dim=feat, v_class=C, batch_size=B, temporal=T)


def _module(dev, shape, seed=5, **kw):
    """an LSTM_cell with non-trivial BatchNorm state, its inputs"""
    from ctc_amd import producer
    T, B, K, C = shape
    with torch.random.fork_rng():
        torch.manual_seed(seed)
        m = producer.LSTM_cell(_args(K, C, B, T), **kw)
        bn = m.v.layers[1] if hasattr(m.v, "layers") else None
        with torch.no_grad():
            if bn is not None:
                bn.weight.uniform_(0.5, 1.5); bn.bias.normal_(0.0, 0.2)
                bn.running_mean.normal_(0.0, 0.3); bn.running_var.uniform_(0.5, 2.0)
        feat, h0, c0 = torch.randn(T, B, K), 0.1 * torch.randn(B, C), 0.1 * torch.randn(B, C)
    return m.to(dev), feat.to(dev), h0.to(dev), c0.to(dev)


class _Counter:
    """wraps a function of ctc_amd.producer: counts the calls; `off`: answers None (the caller's two-launch path)"""

    def __init__(self, monkeypatch, name, off=False):
        from ctc_amd import producer
        self.calls, self.off, self.fn = 0, off, getattr(producer, name)
        monkeypatch.setattr(producer, name, self)

    def __call__(self, *a, **k):
        self.calls += 1
        return None if self.off else self.fn(*a, **k)


def _open_gate(monkeypatch):
    from ctc_amd import producer
    monkeypatch.setattr(producer, "FUSED_FORWARD_MAX_WG_ROWS", 1 << 30)


def test_reference_fixture_through_the_module(dev, golden, monkeypatch):
    """tests/golden/lstm_series.npz is the reference's own LSTM_cell in eval mode (make_golden.py F7).  It stores the cell's
    parameters, the initial state and v_series, not the head's: the module and feat are drawn again from the fixture's seed in
    the fixture's order, and the cell's parameters and (h0, c0) that come out must BE the stored ones, bit for bit.  Tolerance:
    test_lstm_series_golden's, 5e-6."""
    from ctc_amd import producer
    f = golden("lstm_series")
    with torch.random.fork_rng():
        torch.manual_seed(7)
        m = producer.LSTM_cell(_args()).eval()
        with torch.no_grad():
            m.v.layers[1].running_mean.normal_(0.0, 0.3)
            m.v.layers[1].running_var.uniform_(0.5, 1.5)
            feat = torch.randn(10, 10, 1024)
            h0, c0 = 0.1 * torch.randn(10, 33), 0.1 * torch.randn(10, 33)
    cell = m.v_cell
    for got, key in ((cell.weight_ih, "w_ih"), (cell.weight_hh, "w_hh"), (cell.bias_ih, "b_ih"), (cell.bias_hh, "b_hh"), (h0, "h0"), (c0, "c0")):
        assert np.array_equal(np_(got), f[key]), "the fixture's state did not come back from its seed: " + key
    m, feat, h0, c0 = m.to(dev), feat.to(dev), h0.to(dev), c0.to(dev)
    with torch.no_grad():
        shipped = m(feat, h0, c0)                            # (the gate as shipped)
        _open_gate(monkeypatch)
        one = _Counter(monkeypatch, "lstm_forward")
        fused = m(feat, h0, c0)
        assert one.calls == 1
        one.off = True
        two = m(feat, h0, c0)
        assert one.calls == 2
    torch.cuda.synchronize()
    assert fused.shape == (10, 10, 33) and np.abs(np_(fused) - f["v_series"]).max() < 5e-6
    assert torch.equal(fused, two) and torch.equal(shipped, two)


def test_module_takes_the_one_launch_path_in_eval_without_grad(dev, monkeypatch):
    """eval() + no_grad at the reference's sizes: 4 T = 40 head rows per workgroup lie inside the measured gate of 64
    (profiles/r13_lstm_forward.md: 50 us against 70 us there), so forward is ONE launch -- lstm_forward once, head_forward never"""
    from ctc_amd import producer
    assert producer.FUSED_FORWARD_MAX_WG_ROWS == 64
    m, feat, h0, c0 = _module(dev, REF)
    m.eval()
    one, head = _Counter(monkeypatch, "lstm_forward"), _Counter(monkeypatch, "head_forward")
    with torch.no_grad():
        got = m(feat, h0, c0)
    assert one.calls == 1 and head.calls == 0
    # grad mode on, but nothing requires a gradient: still one launch
    for prm in m.parameters():
        prm.requires_grad_(False)
    got2 = m(feat, h0, c0)
    assert one.calls == 2 and head.calls == 0
    one.off = True
    with torch.no_grad():
        want = m(feat, h0, c0)
    assert one.calls == 3 and head.calls == 1
    assert torch.equal(got, want) and torch.equal(got2, want)
    # pad_classes: the pad column comes out of the same launch
    mp, feat, h0, c0 = _module(dev, REF, pad_classes=True)
    one.off = False
    with torch.no_grad():
        got = mp.eval()(feat, h0, c0)
        one.off = True
        want = mp(feat, h0, c0)
    assert got.shape == (10, 10, 34) and torch.equal(got, want) and (got[:, :, 33] == producer.PAD_LOGIT).all()


def test_module_outside_the_gate_keeps_the_two_launches(dev, monkeypatch):
    """T = 17 frames are 68 head rows per workgroup: beyond the measured bound, whatever B is (T = 16 is the last inside)"""
    one = _Counter(monkeypatch, "lstm_forward")
    for shape, calls in (((17, 2, 32, 17), 0), ((17, 9, 32, 17), 0), ((16, 9, 32, 17), 1)):
        m, feat, h0, c0 = _module(dev, shape)
        with torch.no_grad():
            m.eval()(feat, h0, c0)
        assert one.calls == calls, shape


def _grads(m, feat, h0, c0, R):
    for prm in m.parameters():
        prm.grad = None
    f, h, c = (t.detach().clone().requires_grad_(True) for t in (feat, h0, c0))
    out = m(f, h, c)
    (out * R).sum().backward()
    return [out.detach()] + [t.grad.clone() for t in (f, h, c)] + [prm.grad.clone() for prm in m.parameters()]


def test_module_stays_on_two_launches_where_it_must(dev, monkeypatch):
    """train mode, a call that needs a gradient, a custom head: lstm_forward is not entered, and outputs and gradients are
    what they are with the path forced off"""
    from ctc_amd import producer
    _open_gate(monkeypatch)
    shape = (6, 5, 64, 17)
    T, B, K, C = shape
    R = torch.randn(T, B, C, generator=torch.Generator().manual_seed(2)).to(dev)

    class Custom(torch.nn.Module):
        def __init__(self, i, o):
            super().__init__()
            self.lin = torch.nn.Linear(i, o)

        def forward(self, x):
            return torch.tanh(self.lin(x))

    cases = [("train", {}, True), ("eval with feat.requires_grad", {}, False), ("custom head", dict(_BaseModule=Custom), False)]
    for name, kw, train in cases:
        m, feat, h0, c0 = _module(dev, shape, **kw)
        m.train(train)
        state = {k: v.clone() for k, v in m.state_dict().items()}
        results = []
        for off in (False, True):
            m.load_state_dict(state)                         # (train mode moves the running statistics)
            one = _Counter(monkeypatch, "lstm_forward", off=off)
            with torch.random.fork_rng(devices=[0]):
                torch.manual_seed(3)                         # (the dropout mask)
                if name == "custom head":
                    with torch.no_grad():
                        results.append([m(feat, h0, c0)])
                else:
                    results.append(_grads(m, feat, h0, c0, R))
            assert one.calls == 0, name
            monkeypatch.undo()
            _open_gate(monkeypatch)
        assert len(results[0]) == len(results[1])
        for a, b in zip(*results):
            assert torch.equal(a, b), name


@pytest.mark.parametrize("shape", [(4, 5, 64, 41), (4, 5, 24, 17)])
def test_refused_shapes_fall_back_in_the_module(dev, monkeypatch, shape):
    """C = 41 (2 C > 80) and K = 24: the entry answers CTC_AMD_ERR_UNSUPPORTED_SHAPE, lstm_forward returns None, and
    LSTM_cell.forward in eval mode goes on as before"""
    _open_gate(monkeypatch)
    m, feat, h0, c0 = _module(dev, shape)
    m.eval()
    one = _Counter(monkeypatch, "lstm_forward")
    with torch.no_grad():
        got = m(feat, h0, c0)
        assert one.calls == 1
        one.off = True
        want = m(feat, h0, c0)
    torch.cuda.synchronize()
    assert got.shape == (shape[0], shape[1], shape[3]) and torch.equal(got, want)


def test_capture_and_replay(dev):
    """no workspace, no host synchronisation: one torch.cuda.graph capture after an eager warm-up, replayed once"""
    feat, head, cell = _inputs(dev, *REF)
    eager = _one_launch(feat, head, cell, 34)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _one_launch(feat, head, cell, 34)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = _one_launch(feat, head, cell, 34)
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
