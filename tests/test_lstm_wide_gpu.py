"""The recurrence for up to 160 classes on the device (ctc_amd_lstm_series_wide / ctc_amd_lstm_series_backward_wide and the
wide path of _SeriesFn): the forward's bits against T calls of ctc_amd_lstm_cell_step, the backward against torch autograd
through nn.LSTMCell and against the float64 restatement (oracle.ctc_numpy), determinism, the closed gate, a train-mode
LSTM_cell step at 158 classes, and stream capture.

Bounds: the forward against the float64 restatement < 2e-5 absolute, the gradients <= 3e-5 max(1, max|ref|) against torch's
fp32 autograd and <= 2e-5 max(1, max|ref|) against float64 -- what tests/test_producer_gpu.py holds the narrow launches to."""
import copy
import types

import numpy as np
import pytest
import torch

from oracle import ctc_numpy

pytestmark = pytest.mark.gpu

# (T, B, I, H): the benchmark's class count with B no multiple of the samples per workgroup and an odd T; one past the narrow
# bound; the upper bound with one sample and T = 2; I != H with an odd H; small I, large H; T = 1; a narrow shape; the
# workload's frame count at a small batch
SHAPES = [(7, 9, 158, 158), (3, 5, 65, 65), (2, 1, 160, 160), (5, 17, 120, 81), (4, 6, 16, 160), (1, 4, 33, 120), (9, 5, 17, 40),
          (150, 4, 158, 158)]
NAMES = ("dv", "dh0", "dc0", "dW_ih", "dW_hh", "db_ih", "db_hh")
IDS = lambda s: "x".join(map(str, s))          # noqa: E731
OPEN = 1 << 30


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    import ctc_amd  # noqa: F401
    return torch.device("cuda:0")


def np_(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _counting(monkeypatch, name):
    """wrap a bound entry in a counter (the ctypes function object is per library handle: put the wrapper on the handle)"""
    from ctc_amd import _lib
    lib = _lib.load()
    real = getattr(lib, name)
    calls = []

    def wrapped(*a):
        calls.append(1)
        return real(*a)
    monkeypatch.setattr(lib, name, wrapped)
    return calls


def _draw(shape, dev):
    """inputs as test_lstm_series_one_launch_is_bit_identical_to_the_steps draws them (weights x 0.3)"""
    T, B, I, H = shape
    g = torch.Generator().manual_seed(sum(shape))
    rnd = lambda *s: (torch.rand(*s, generator=g) * 2 - 1).to(dev)          # noqa: E731
    v_all, h0, c0 = rnd(T, B, I), rnd(B, H), rnd(B, H)
    w_ih, w_hh, b_ih, b_hh = rnd(4 * H, I) * 0.3, rnd(4 * H, H) * 0.3, rnd(4 * H) * 0.1, rnd(4 * H) * 0.1
    return v_all, h0, c0, w_ih, w_hh, b_ih, b_hh


_STEPS = {}


def _steps(shape, cols, dev):
    """T calls of lstm_cell_step (once per shape and width): series with its pad columns, gates, cells"""
    if (shape, cols) in _STEPS:
        return _STEPS[(shape, cols)]
    import ctc_amd
    T, B, I, H = shape
    v_all, h0, c0, w_ih, w_hh, b_ih, b_hh = _draw(shape, dev)
    series = torch.empty((T, B, cols), dtype=torch.float32, device=dev)
    h, c, gates, cells = h0, c0, [], [c0]
    for t in range(T):
        h, c, gt = ctc_amd.lstm_cell_step(v_all[t], h, c, w_ih, w_hh, b_ih, b_hh, series[t], want_gates=True)
        gates.append(gt)
        cells.append(c)
    torch.cuda.synchronize()
    _STEPS[(shape, cols)] = (series, torch.stack(gates), torch.stack(cells))
    return _STEPS[(shape, cols)]


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_forward_is_bit_identical_to_the_steps(dev, shape):
    import ctc_amd
    T, B, I, H = shape
    args = _draw(shape, dev)
    for cols in (H, H + 1 + H % 2):
        ref_series, ref_gates, ref_cells = _steps(shape, cols, dev)
        whole = ctc_amd.lstm_series_wide(*args, cols, want_backward_state=True)
        assert whole is not None, shape
        series, gates, cells = whole
        torch.cuda.synchronize()
        assert series.shape == (T, B, cols) and gates.shape == (T, B, 4 * H) and cells.shape == (T + 1, B, H)
        assert torch.equal(series, ref_series), (shape, cols)                # (pad columns included)
        if cols > H:
            assert bool((series[:, :, H:] == ctc_amd.producer.PAD_LOGIT).all())
        assert torch.equal(gates, ref_gates), (shape, cols)
        assert torch.equal(cells, ref_cells), (shape, cols)
        assert torch.equal(cells[0], args[2])
        if shape == (9, 5, 17, 40):                                          # a narrow shape: the narrow launch's bits as well
            narrow = ctc_amd.lstm_series(*args, cols, want_backward_state=True)
            assert narrow is not None
            for a, b in zip(whole, narrow):
                assert torch.equal(a, b)
    want = ctc_numpy.lstm_cell_series(*(np_(t) for t in args))[0]
    err = float(np.abs(np_(series)[:, :, :H] - want).max())
    print("forward %s: max|got - float64| = %.3e" % (shape, err))
    assert err < 2e-5


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_forward_without_state(dev, shape):
    import ctc_amd
    T, B, I, H = shape
    args = _draw(shape, dev)
    for cols in (H, H + 1 + H % 2):
        series, gates, cells = ctc_amd.lstm_series_wide(*args, cols, want_backward_state=False)
        torch.cuda.synchronize()
        assert gates is None and cells is None
        assert torch.equal(series, _steps(shape, cols, dev)[0]), (shape, cols)


def _check(got, ref, bound, what):
    worst = {}
    for name, a, b in zip(NAMES, got, ref):
        assert a.shape == b.shape, (name, a.shape, b.shape)
        err, scale = float(np.abs(a - b).max()), max(1.0, float(np.abs(b).max()))
        worst[name] = err / scale
        print("%s %s: max|got - ref| = %.3e, scale %.3e" % (what, name, err, scale))
    for name, v in worst.items():
        assert v <= bound, (what, name, v)


_AUTOGRAD = {}


def _autograd_case(shape, dev):
    """nn.LSTMCell (default init) on the device, leaves, a random upstream gradient at H + 1 columns, torch autograd's
    gradients and the float64 restatement's (once per shape)"""
    if shape in _AUTOGRAD:
        return _AUTOGRAD[shape]
    T, B, I, H = shape
    torch.manual_seed(100 + sum(shape))
    g = torch.Generator().manual_seed(sum(shape))
    rnd = lambda *s: (torch.rand(*s, generator=g) * 2 - 1).to(dev)          # noqa: E731
    c = types.SimpleNamespace()
    c.cell = torch.nn.LSTMCell(I, H).to(dev)
    c.leaves = [rnd(T, B, I), rnd(B, H), rnd(B, H)]
    c.up = rnd(T, B, H + 1)
    v_all, h0, c0 = (t.clone().requires_grad_(True) for t in c.leaves)
    c.cell.zero_grad()
    h, cc, rows = h0, c0, []
    for t in range(T):
        h, cc = c.cell(v_all[t], (h, cc))
        rows.append(h)
    (torch.stack(rows) * c.up[:, :, :H]).sum().backward()
    c.torch = [np_(t.grad) for t in (v_all, h0, c0, c.cell.weight_ih, c.cell.weight_hh, c.cell.bias_ih, c.cell.bias_hh)]
    c.cell.zero_grad()
    c.f64 = ctc_numpy.lstm_cell_series_backward(np_(c.up)[:, :, :H], *(np_(t) for t in c.leaves), np_(c.cell.weight_ih),
                                                np_(c.cell.weight_hh), np_(c.cell.bias_ih), np_(c.cell.bias_hh))
    _AUTOGRAD[shape] = c
    return c


def _seriesfn(c, H):
    """_SeriesFn forward and backward on the case's cell -> (series, grad_fn, gradients as numpy)"""
    from ctc_amd import producer
    v_all, h0, c0 = (t.clone().requires_grad_(True) for t in c.leaves)
    cell = c.cell
    cell.zero_grad()
    series = producer._SeriesFn.apply(v_all, h0, c0, cell.weight_ih, cell.weight_hh, cell.bias_ih, cell.bias_hh, H + 1,
                                      producer.PAD_LOGIT)
    fn = series.grad_fn
    (series * c.up).sum().backward()
    torch.cuda.synchronize()
    grads = [np_(t.grad) for t in (v_all, h0, c0, cell.weight_ih, cell.weight_hh, cell.bias_ih, cell.bias_hh)]
    cell.zero_grad()
    return series.detach(), fn, grads


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_backward_matches_torch_autograd(dev, monkeypatch, shape):
    from ctc_amd import producer
    T, B, I, H = shape
    c = _autograd_case(shape, dev)
    monkeypatch.setattr(producer, "SERIES_WIDE_MAX_ROWS", OPEN)
    if shape == (9, 5, 17, 40):                              # (a narrow shape: only with the narrow launch out of the way
        monkeypatch.setattr(producer, "lstm_series", lambda *a, **k: None)    # does _SeriesFn reach the wide one)
    fwd = _counting(monkeypatch, "ctc_amd_lstm_series_wide")
    bwd = _counting(monkeypatch, "ctc_amd_lstm_series_backward_wide")
    steps = _counting(monkeypatch, "ctc_amd_lstm_cell_step")
    bias = _counting(monkeypatch, "ctc_amd_lstm_bias_grad_wide")
    series, fn, grads = _seriesfn(c, H)
    assert fn.wide and not fn.one_launch and not fn.in_place
    assert len(fwd) == 1 and len(bwd) == 1 and len(bias) == 1 and len(steps) == 0
    _check(grads, c.torch, 3e-5, "autograd %s" % (shape,))
    _check(grads, c.f64, 2e-5, "float64 %s" % (shape,))


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_backward_is_deterministic(dev, shape):
    import ctc_amd
    T, B, I, H = shape
    args = _draw(shape, dev)
    _, gates, cells = _steps(shape, H + 1 + H % 2, dev)
    g = torch.Generator().manual_seed(7 + sum(shape))
    up = (torch.rand(T, B, H + 1, generator=g) * 2 - 1).to(dev)
    a = ctc_amd.lstm_series_backward_wide(up, gates, cells, args[4])
    b = ctc_amd.lstm_series_backward_wide(up, gates, cells, args[4])
    torch.cuda.synchronize()
    assert a is not None and b is not None
    for x, y in zip(a, b):
        assert x.data_ptr() != y.data_ptr() and torch.equal(x, y) and bool(torch.isfinite(x).all())


def test_gate_closed(dev, monkeypatch):
    from ctc_amd import producer
    shape = (7, 9, 158, 158)
    H = shape[3]
    c = _autograd_case(shape, dev)
    fwd = _counting(monkeypatch, "ctc_amd_lstm_series_wide")
    bwd = _counting(monkeypatch, "ctc_amd_lstm_series_backward_wide")
    steps = _counting(monkeypatch, "ctc_amd_lstm_cell_step")
    monkeypatch.setattr(producer, "SERIES_WIDE_MAX_ROWS", 0)
    closed, fn, grads = _seriesfn(c, H)
    assert not fn.wide and not fn.one_launch
    assert len(fwd) == 0 and len(bwd) == 0 and len(steps) == shape[0]
    _check(grads, c.torch, 3e-5, "closed, autograd")
    _check(grads, c.f64, 2e-5, "closed, float64")
    monkeypatch.setattr(producer, "SERIES_WIDE_MAX_ROWS", OPEN)
    opened, fn, _ = _seriesfn(c, H)
    assert fn.wide and len(fwd) == 1 and len(bwd) == 1 and len(steps) == shape[0]
    assert torch.equal(opened, closed)


def test_module_at_158_classes(dev, monkeypatch):
    """LSTM_cell(v_class=158) in train mode with dropout: the wide path against the same seeded step with the gate closed"""
    import ctc_amd
    from ctc_amd import producer
    from tests.test_head_backward_gpu import TOL
    T, B, K, C = 4, 6, 64, 158
    args = types.SimpleNamespace(extract_feat_dim=K, v_class=C, batch_size=B, temporal=T)
    torch.manual_seed(31)
    model = ctc_amd.LSTM_cell(args).to(dev).train()
    g = torch.Generator().manual_seed(32)
    rnd = lambda *s: (torch.rand(*s, generator=g) * 2 - 1).to(dev)          # noqa: E731
    feat0, h0, c0, up = rnd(T, B, K), rnd(B, C) * 0.1, rnd(B, C) * 0.1, rnd(T, B, C)
    fwd = _counting(monkeypatch, "ctc_amd_lstm_series_wide")
    state = copy.deepcopy(model.state_dict())                # (BatchNorm's running statistics move with every train step)
    out = {}
    for gate in (OPEN, 0):
        monkeypatch.setattr(producer, "SERIES_WIDE_MAX_ROWS", gate)
        model.load_state_dict(state)
        model.train()
        model.zero_grad(set_to_none=True)
        feat = feat0.clone().requires_grad_(True)
        torch.manual_seed(33)                                # (the dropout mask)
        before = len(fwd)
        series = model(feat, h0, c0)
        (series * up).sum().backward()
        torch.cuda.synchronize()
        assert len(fwd) - before == (1 if gate else 0)
        grads = {name: p.grad.clone() for name, p in model.named_parameters()}
        grads["feat"] = feat.grad.clone()
        model.eval()
        with torch.no_grad():
            ev = model(feat0, h0, c0)
        torch.cuda.synchronize()
        assert len(fwd) - before == (2 if gate else 0)
        out[gate] = (series.detach().clone(), grads, ev.clone())
    assert torch.equal(out[OPEN][0], out[0][0])
    assert torch.equal(out[OPEN][2], out[0][2])
    assert set(out[OPEN][1]) == set(out[0][1]) and len(out[0][1]) == 9
    for name, b in out[0][1].items():
        a = out[OPEN][1][name]
        v = float((a - b).abs().max()) / max(1.0, float(b.abs().max()))
        print("LSTM_cell(158) %s: %.3e" % (name, v))
        assert v <= TOL, (name, v)


@pytest.mark.parametrize("rows,H", [(1, 1), (15, 160), (16, 33), (17, 158), (255, 81), (256, 16), (257, 17), (1500, 158), (4099, 96)],
                         ids=lambda v: str(v))
def test_bias_grad_column_sums(dev, rows, H):
    """ctc_amd_lstm_bias_grad_wide: the column sums of dpre [rows, 4H] -- one row, fewer rows than waves, one past a round of the
    sixteen waves, one past sixteen rounds, the bench's 1500; 4H below, at and above a multiple of 64 -- against a float64 sum,
    within 2e-5 max(1, max|ref|) (fp32 sums of at most 4099 terms of magnitude <= 1: 4099 * 2^-24 * max|partial sum| is far
    inside), two tensors with the same bits, two calls the same bits"""
    import ctc_amd
    g = torch.Generator().manual_seed(rows + H)
    dpre = (torch.rand(rows, 1, 4 * H, generator=g) * 2 - 1).to(dev)
    a0, a1 = ctc_amd.lstm_bias_grad_wide(dpre)
    b0, b1 = ctc_amd.lstm_bias_grad_wide(dpre)
    torch.cuda.synchronize()
    assert a0.shape == (4 * H,) and a0.data_ptr() != a1.data_ptr()
    assert torch.equal(a0, a1) and torch.equal(a0, b0) and torch.equal(a0, b1)
    ref = np_(dpre).reshape(rows, 4 * H).sum(0)
    err = float(np.abs(np_(a0) - ref).max()) / max(1.0, float(np.abs(ref).max()))
    print("bias grad (%d, %d): %.3e" % (rows, H, err))
    assert err <= 2e-5


@pytest.mark.parametrize("shape", [(7, 9, 158, 158), (150, 10, 158, 158)], ids=IDS)
def test_capture(dev, monkeypatch, shape):
    """one forward and backward captured into a torch.cuda.graph on a side stream and replayed twice gives the eager bits
    (every launch goes to the one capture stream: a single chain, no parallel branches).  (150, 10, 158, 158) is the shape at
    which a replay once returned wrong bias gradients while torch's column sum was still behind the recurrence launch."""
    from ctc_amd import producer
    T, B, I, H = shape
    monkeypatch.setattr(producer, "SERIES_WIDE_MAX_ROWS", OPEN)
    fwd = _counting(monkeypatch, "ctc_amd_lstm_series_wide")
    bwd = _counting(monkeypatch, "ctc_amd_lstm_series_backward_wide")
    g = torch.Generator().manual_seed(5)
    up = (torch.rand(T, B, H + 1, generator=g) * 2 - 1).to(dev)
    leaves = [t.clone().requires_grad_(True) for t in _draw(shape, dev)]

    def step():
        series = producer._SeriesFn.apply(*leaves, H + 1, producer.PAD_LOGIT)
        return (series,) + torch.autograd.grad((series * up).sum(), leaves)

    eager = [t.detach().clone() for t in step()]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                            # warm-up on the capture stream
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        captured = step()
    assert len(fwd) == 3 and len(bwd) == 3
    for _ in range(2):
        for x in captured:
            x.detach().fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(eager, captured):
            assert torch.equal(a, b.detach())
