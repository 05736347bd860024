"""The recurrence's backward on the HIP path, whole (ctc_amd_lstm_backward / ctc_amd.lstm_backward) on the device: the entry
against the float64 restatement of the back-propagation (oracle.ctc_numpy.lstm_cell_series_backward), the recurrence's bits
against ctc_amd_lstm_series_backward, the layout and determinism contract, the path through the gate of _SeriesFn, a
train-mode LSTM_cell step, shapes the entry does not take, and stream capture.

Bound: 2e-5 max(1, max|ref|), what tests/test_producer_gpu.py holds the torch-GEMM path to on these shape families."""
import types

import numpy as np
import pytest
import torch

from oracle import ctc_numpy
from tests.head_backward_ref import MARGIN

pytestmark = pytest.mark.gpu

NAMES = ("d_x", "dh0", "dc0", "d_w_ih", "d_w_hh", "d_b_ih", "d_b_hh")
# (T, B, I, H), the smallest at which each mechanism can go wrong: T = 1 (h_{t-1} is h0 alone); 4H = 256 and I = 64 at the
# edges; I != H, neither a multiple of 16; 140 rows, the first row-range split (two ranges of 80 rows: the cut falls inside
# frame 11); 768 rows; 9600 rows (60 ranges of 160 rows: the rule's cap of 128 rows per range no longer holds)
SHAPES = [(1, 1, 16, 16), (3, 1, 64, 16), (2, 3, 16, 64), (9, 5, 17, 40), (20, 7, 38, 38), (12, 64, 33, 33), (150, 64, 33, 33)]
TOL = 2e-5
IDS = lambda s: "x".join(map(str, s))          # noqa: E731


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    import ctc_amd  # noqa: F401
    return torch.device("cuda:0")


def np_(t):
    return t.detach().cpu().numpy().astype(np.float64)


_CASES = {}


def _case(shape, dev):
    """inputs on the device, the forward's saved state at a padded pitch, and the float64 reference (once per shape)"""
    if shape in _CASES:
        return _CASES[shape]
    import ctc_amd
    T, B, I, H = shape
    g = torch.Generator().manual_seed(4000 + sum(shape))
    rnd = lambda *s: (torch.rand(*s, generator=g) * 2 - 1).to(dev)          # noqa: E731
    c = types.SimpleNamespace()
    c.v_all, c.h0, c.c0 = rnd(T, B, I), rnd(B, H), rnd(B, H)
    c.w_ih, c.w_hh, c.b_ih, c.b_hh = rnd(4 * H, I) * 0.3, rnd(4 * H, H) * 0.3, rnd(4 * H) * 0.1, rnd(4 * H) * 0.1
    c.cols = H + 1 + H % 2
    c.up = rnd(T, B, c.cols)                                 # the upstream gradient at the padded width: ds_stride_b > H
    whole = ctc_amd.lstm_series(c.v_all, c.h0, c.c0, c.w_ih, c.w_hh, c.b_ih, c.b_hh, c.cols, want_backward_state=True)
    assert whole is not None, shape
    c.series, c.gates, c.cells = whole
    torch.cuda.synchronize()
    c.ref = ctc_numpy.lstm_cell_series_backward(np_(c.up)[:, :, :H], np_(c.v_all), np_(c.h0), np_(c.c0), np_(c.w_ih), np_(c.w_hh),
                                                np_(c.b_ih), np_(c.b_hh))
    _CASES[shape] = c
    return c


def _check(got, ref, what):
    worst = {}
    for name, a, b in zip(NAMES, got, ref):
        a = np_(a) if torch.is_tensor(a) else np.asarray(a, np.float64)
        b = np_(b) if torch.is_tensor(b) else np.asarray(b, np.float64)
        assert a.shape == b.shape, (name, a.shape, b.shape)
        err, scale = float(np.abs(a - b).max()), max(1.0, float(np.abs(b).max()))
        worst[name] = err / scale
        print("%s %s: max|got - ref| = %.3e, scale %.3e" % (what, name, err, scale))
    for name, v in worst.items():
        assert v <= TOL, (what, name, v)


def _entry(c, need_dx=True):
    import ctc_amd
    return ctc_amd.lstm_backward(c.up, c.gates, c.cells, c.v_all, c.h0, c.series, c.w_ih, c.w_hh, need_dx)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_entry_against_the_oracle(dev, shape):
    from ctc_amd import producer
    c = _case(shape, dev)
    got = _entry(c)
    assert got is not None
    torch.cuda.synchronize()
    _check(got, c.ref, "entry %s" % (shape,))
    # the same recurrence launch: dh0 and dc0 carry ctc_amd_lstm_series_backward's bits
    _, dh0, dc0 = producer.lstm_series_backward(c.up, c.gates, c.cells, c.w_hh)
    assert torch.equal(got[1], dh0) and torch.equal(got[2], dc0)
    assert got[5].data_ptr() != got[6].data_ptr() and torch.equal(got[5], got[6])


def _raw_call(c, shape, d_x, outs, scratch_ptr, nbytes):
    """the C entry itself on caller-made buffers; outs: dh0, dc0, d_w_ih, d_w_hh, d_b_ih, d_b_hh views"""
    from ctc_amd import _lib
    from ctc_amd import functional as F
    T, B, I, H = shape
    dev = c.up.device
    with F._on_device(dev):
        rc = _lib.load().ctc_amd_lstm_backward(
            c.up.data_ptr(), c.up.stride(0), c.up.stride(1), c.gates.data_ptr(), c.cells.data_ptr(),
            c.v_all.data_ptr(), c.v_all.stride(0), c.v_all.stride(1), c.h0.data_ptr(),
            c.series.data_ptr(), c.series.stride(0), c.series.stride(1), c.w_ih.data_ptr(), c.w_hh.data_ptr(), T, B, I, H,
            None if d_x is None else d_x.data_ptr(), 0 if d_x is None else d_x.stride(0), 0 if d_x is None else d_x.stride(1),
            *(o.data_ptr() for o in outs), scratch_ptr, nbytes, F._stream_handle(dev))
    assert rc == 0, rc


@pytest.mark.parametrize("shape", [(20, 7, 38, 38), (9, 5, 17, 40)], ids=IDS)
def test_layout_and_contract(dev, shape):
    from ctc_amd import _lib
    T, B, I, H = shape
    c = _case(shape, dev)
    nbytes = _lib.load().ctc_amd_lstm_backward_scratch_bytes(T, B, I, H)
    assert nbytes > 0
    SENT, GUARD = -12345.0, 8
    sizes = (B * H, B * H, 4 * H * I, 4 * H * H, 4 * H, 4 * H)
    views = ((B, H), (B, H), (4 * H, I), (4 * H, H), (4 * H,), (4 * H,))

    def run(want_dx, offset):
        # the scratch at exactly the query's size, every byte 0xFF (NaN as floats), at the given byte offset (any alignment)
        scratch = torch.full((nbytes + offset,), 0xFF, dtype=torch.uint8, device=dev)
        dx_buf = torch.full((T, B, I + 3), float("nan"), device=dev) if want_dx else None
        bufs = [torch.full((n + 2 * GUARD,), SENT, device=dev) for n in sizes]
        _raw_call(c, shape, dx_buf[:, :, :I] if want_dx else None, [b[GUARD:] for b in bufs], scratch.data_ptr() + offset, nbytes)
        torch.cuda.synchronize()
        for b in bufs:                                       # the guards on both sides are untouched
            assert bool((b[:GUARD] == SENT).all()) and bool((b[-GUARD:] == SENT).all())
        if want_dx:                                          # d_x rows are written in columns [0, I) only
            assert bool(torch.isnan(dx_buf[:, :, I:]).all()) and not bool(torch.isnan(dx_buf[:, :, :I]).any())
        outs = [b[GUARD:-GUARD].clone().reshape(v) for b, v in zip(bufs, views)]
        return (dx_buf[:, :, :I].clone() if want_dx else None), outs

    dx_a, outs_a = run(True, 0)
    _check([dx_a] + outs_a, c.ref, "layout %s" % (shape,))
    assert torch.equal(outs_a[4], outs_a[5])                 # d_b_ih and d_b_hh: two buffers, the same bits
    dx_b, outs_b = run(True, 0)                              # a second call gives the same bits
    dx_c, outs_c = run(True, 1)                              # the scratch at an odd address
    _, outs_d = run(False, 0)                                # d_x = NULL: the other six unchanged
    for other_dx, other in ((dx_b, outs_b), (dx_c, outs_c), (None, outs_d)):
        if other_dx is not None:
            assert torch.equal(dx_a, other_dx)
        for a, b in zip(outs_a, other):
            assert torch.equal(a, b)


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


@pytest.mark.parametrize("shape", [(20, 7, 38, 38), (9, 5, 17, 40)], ids=IDS)
def test_seriesfn_through_the_gate(dev, monkeypatch, shape):
    from ctc_amd import producer
    T, B, I, H = shape
    c = _case(shape, dev)
    calls = _counting(monkeypatch, "ctc_amd_lstm_backward")
    cats = []
    real_cat = torch.cat

    def counting_cat(*a, **k):
        cats.append(1)
        return real_cat(*a, **k)
    res = {}
    for gate in (1 << 30, 0):
        monkeypatch.setattr(producer, "SERIES_BACKWARD_MAX_ROWS", gate)
        leaves = [t.clone().requires_grad_(True) for t in (c.v_all, c.h0, c.c0, c.w_ih, c.w_hh, c.b_ih, c.b_hh)]
        before = len(calls)
        monkeypatch.setattr(producer.torch, "cat", counting_cat)
        ncat = len(cats)
        series = producer._SeriesFn.apply(*leaves, c.cols, producer.PAD_LOGIT)
        in_forward = len(cats) - ncat
        monkeypatch.setattr(producer.torch, "cat", real_cat)
        assert series.grad_fn.one_launch
        assert in_forward == (0 if gate else 1)              # gate open: h_{t-1} is read from v_series, no concatenated copy
        (series * c.up).sum().backward()
        torch.cuda.synchronize()
        assert len(calls) - before == (1 if gate else 0)     # gate 0: the entry is not reached
        res[gate] = [t.grad for t in leaves]
        assert res[gate][5].data_ptr() != res[gate][6].data_ptr()
    _check(res[1 << 30], c.ref, "SeriesFn open %s" % (shape,))
    _check(res[0], c.ref, "SeriesFn closed %s" % (shape,))


@pytest.mark.parametrize("over", [(1,), (0, 1)], ids=["sum_b", "sum_tb"])
@pytest.mark.parametrize("shape", [(20, 7, 38, 38), (9, 5, 17, 40)], ids=IDS)
def test_broadcast_upstream_gradient(dev, monkeypatch, shape, over):
    """a loss that sums v_series over the batch (or over frames and batch) first: autograd hands _SeriesFn.backward an
    EXPANDED d_series (row pitch 0, frame pitch 0 as well in the second case).  Gate open and closed, and the Python entry
    on such a view directly, against the oracle fed with the same gradient written out."""
    import ctc_amd
    from ctc_amd import producer
    T, B, I, H = shape
    c = _case(shape, dev)
    g = torch.Generator().manual_seed(77 + sum(shape) + len(over))
    m = (torch.rand(*(c.up.sum(over).shape), generator=g) * 2 - 1).to(dev)          # [T, cols] or [cols]
    full = (m.unsqueeze(1) if len(over) == 1 else m).expand(T, B, c.cols)
    assert full.stride(1) == 0
    ref = ctc_numpy.lstm_cell_series_backward(np_(full)[:, :, :H], np_(c.v_all), np_(c.h0), np_(c.c0), np_(c.w_ih), np_(c.w_hh),
                                              np_(c.b_ih), np_(c.b_hh))
    calls = _counting(monkeypatch, "ctc_amd_lstm_backward")
    for gate in (1 << 30, 0):
        monkeypatch.setattr(producer, "SERIES_BACKWARD_MAX_ROWS", gate)
        leaves = [t.clone().requires_grad_(True) for t in (c.v_all, c.h0, c.c0, c.w_ih, c.w_hh, c.b_ih, c.b_hh)]
        before = len(calls)
        series = producer._SeriesFn.apply(*leaves, c.cols, producer.PAD_LOGIT)
        (series.sum(over) * m).sum().backward()
        torch.cuda.synchronize()
        assert len(calls) - before == (1 if gate else 0)
        _check([t.grad for t in leaves], ref, "broadcast %s %s gate %d" % (shape, over, gate))
    got = ctc_amd.lstm_backward(full, c.gates, c.cells, c.v_all, c.h0, c.series, c.w_ih, c.w_hh)
    torch.cuda.synchronize()
    _check(got, ref, "broadcast entry %s %s" % (shape, over))


def test_lstm_cell_train_step_both_gates_open(dev, monkeypatch):
    """a train-mode LSTM_cell step (dropout off) against the float64 CPU autograd of the same layers and nn.LSTMCell, both
    backward gates open: the construction, the seed search and the bound of test_lstm_cell_train_step_through_the_gate
    (tests/test_head_backward_gpu.py), extended to the four v_cell parameter gradients"""
    import ctc_amd
    from ctc_amd import producer
    from tests.test_head_backward_gpu import TOL as HEAD_TOL
    T, B, K, C = 5, 10, 1024, 33
    args = types.SimpleNamespace(extract_feat_dim=K, v_class=C, batch_size=B, temporal=T)
    for seed in range(200):
        torch.manual_seed(9000 + seed)
        model = ctc_amd.LSTM_cell(args).train()
        model.v.layers[3].p = 0.0
        g = torch.Generator().manual_seed(seed)
        rnd = lambda *s: (torch.rand(*s, generator=g) * 2 - 1)          # noqa: E731
        with torch.no_grad():
            model.v.layers[1].weight.copy_(rnd(C) * 0.5 + 1.0); model.v.layers[1].bias.copy_(rnd(C) * 0.2)
        leaves, h0, c0, up = rnd(T, B, K), rnd(B, C) * 0.1, rnd(B, C) * 0.1, rnd(T, B, C)
        lin, bn = model.v.layers[0], model.v.layers[1]
        l64, b64, c64 = torch.nn.Linear(K, C).double(), torch.nn.BatchNorm1d(C).double(), torch.nn.LSTMCell(C, C).double()
        l64.load_state_dict({k: v.double() for k, v in lin.state_dict().items()})
        b64.load_state_dict({k: (v.double() if v.is_floating_point() else v) for k, v in bn.state_dict().items()})
        c64.load_state_dict({k: v.double() for k, v in model.v_cell.state_dict().items()})
        f = leaves.double().requires_grad_(True)
        ys = [b64(l64(f[t])) for t in range(T)]
        if float(torch.stack(ys).detach().abs().min()) >= MARGIN:
            break
    assert float(torch.stack(ys).detach().abs().min()) >= MARGIN
    h, c, hs = h0.double(), c0.double(), []
    for t in range(T):
        h, c = c64(torch.relu(ys[t]), (h, c))
        hs.append(h)
    (torch.stack(hs) * up.double()).sum().backward()
    ref = {"d_feat": f.grad, "d_weight": l64.weight.grad, "d_bn_weight": b64.weight.grad, "d_bn_bias": b64.bias.grad,
           "d_w_ih": c64.weight_ih.grad, "d_w_hh": c64.weight_hh.grad, "d_b_ih": c64.bias_ih.grad, "d_b_hh": c64.bias_hh.grad}
    model = model.to(dev)
    head_calls = _counting(monkeypatch, "ctc_amd_head_backward")
    cell_calls = _counting(monkeypatch, "ctc_amd_lstm_backward")
    monkeypatch.setattr(producer, "HEAD_BACKWARD_MAX_ROWS", 1 << 30)
    monkeypatch.setattr(producer, "SERIES_BACKWARD_MAX_ROWS", 1 << 30)
    feat = leaves.to(dev).requires_grad_(True)
    series = model(feat, h0.to(dev), c0.to(dev))
    (series * up.to(dev)).sum().backward()
    torch.cuda.synchronize()
    assert len(head_calls) == 1 and len(cell_calls) == 1
    lin, bn, cell = model.v.layers[0], model.v.layers[1], model.v_cell
    got = {"d_feat": feat.grad, "d_weight": lin.weight.grad, "d_bn_weight": bn.weight.grad, "d_bn_bias": bn.bias.grad,
           "d_w_ih": cell.weight_ih.grad, "d_w_hh": cell.weight_hh.grad, "d_b_ih": cell.bias_ih.grad, "d_b_hh": cell.bias_hh.grad}
    worst = {}
    for name in ref:                                         # (the Linear bias: identically 0 under batch statistics, skipped there too)
        a, b = np_(got[name]), np_(ref[name])
        worst[name] = float(np.abs(a - b).max()) / max(1.0, float(np.abs(b).max()))
        print("LSTM_cell %s: %.3e" % (name, worst[name]))
    for name, v in worst.items():
        assert v <= HEAD_TOL, (name, v)


def test_shapes_the_entry_does_not_take(dev, monkeypatch):
    """H = 158 (I + H > 80): lstm_backward returns None; _SeriesFn with the gate open steps frame by frame, forward and
    backward, and still returns finite gradients"""
    import ctc_amd
    from ctc_amd import producer
    T, B, H = 3, 4, 158
    g = torch.Generator().manual_seed(5)
    rnd = lambda *s: (torch.rand(*s, generator=g) * 2 - 1).to(dev)          # noqa: E731
    assert ctc_amd.lstm_backward(rnd(T, B, H), rnd(T, B, 4 * H), rnd(T + 1, B, H), rnd(T, B, H), rnd(B, H), rnd(T, B, H),
                                 rnd(4 * H, H), rnd(4 * H, H)) is None
    assert ctc_amd.lstm_backward(rnd(T, B, H), rnd(T, B, 4 * H), rnd(T + 1, B, H), rnd(T, B, H), rnd(B, H), rnd(T, B, H),
                                 rnd(4 * H, H), rnd(4 * H, H), need_dx=False) is None
    monkeypatch.setattr(producer, "SERIES_BACKWARD_MAX_ROWS", 1 << 30)
    calls = _counting(monkeypatch, "ctc_amd_lstm_backward")
    leaves = [t.requires_grad_(True) for t in (rnd(T, B, H), rnd(B, H), rnd(B, H), rnd(4 * H, H) * 0.1, rnd(4 * H, H) * 0.1,
                                               rnd(4 * H) * 0.1, rnd(4 * H) * 0.1)]
    series = producer._SeriesFn.apply(*leaves, H, producer.PAD_LOGIT)
    assert not series.grad_fn.one_launch
    series.sum().backward()
    torch.cuda.synchronize()
    assert len(calls) == 0
    assert all(t.grad is not None and bool(torch.isfinite(t.grad).all()) for t in leaves)


def test_capture(dev):
    """one call captured into a torch.cuda.graph on a side stream and replayed twice gives the eager call's bits (the call is
    three launches on one stream: a single chain, no parallel branches)"""
    c = _case((12, 64, 33, 33), dev)
    eager = _entry(c)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                            # warm-up on the capture stream
        _entry(c)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        captured = _entry(c)
    for _ in range(2):
        for x in captured:
            x.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(eager, captured):
            assert torch.equal(a, b)
