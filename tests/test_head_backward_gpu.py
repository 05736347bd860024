"""The head's backward on the HIP path (ctc_amd_head_backward / ctc_amd.head_backward) on the device: the entry against the
float64 restatement (tests/head_backward_ref.py), its layout and determinism contract, the module path through the gate,
and stream capture.

Measured maxima of |got - ref| / max(1, max|ref|) over all cases (bound 1e-4): see profiles/r14_head_backward.md."""
import types

import numpy as np
import pytest
import torch

from tests.head_backward_ref import MARGIN, draw_case, head_backward_ref

pytestmark = pytest.mark.gpu

NAMES = ("d_feat", "d_weight", "d_bias", "d_bn_weight", "d_bn_bias")
# (T, B, K, C): the smallest at which something can go wrong.  The last three are named from the host's rule for the row-range
# splits of the weight gradient, S = min(64, ceil(T B / 128)): 128 rows is the last shape with one range, 144 the first with
# two, 38400 takes all 64
SHAPES = [(2, 2, 16, 5), (1, 17, 32, 16), (7, 16, 48, 17), (4, 37, 64, 40), (5, 10, 1024, 33), (3, 256, 1024, 158),
          (8, 16, 64, 33), (9, 16, 64, 33), (150, 256, 64, 33)]
TOL = 1e-4


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    import ctc_amd  # noqa: F401
    return torch.device("cuda:0")


def _to(d, dev):
    return {k: (torch.from_numpy(v).to(dev) if isinstance(v, np.ndarray) else v) for k, v in d.items()}


def _entry(t, need_dfeat=True):
    import ctc_amd
    return ctc_amd.head_backward(t["d_out"], t["feat"], t["weight"], t["bn_weight"], t["bn_bias"], t["lin"], t.get("mean"),
                                 t.get("invstd"), t.get("running_mean"), t.get("running_var"), t["eps"], t["mask"], need_dfeat)


def _check(got, ref, what, skip=()):
    worst = {}
    for name, a, b in zip(NAMES, got, ref):
        if name in skip:
            continue
        a = a.detach().cpu().numpy().astype(np.float64) if torch.is_tensor(a) else np.asarray(a, np.float64)
        b = b.detach().cpu().numpy().astype(np.float64) if torch.is_tensor(b) else np.asarray(b, np.float64)
        assert a.shape == b.shape, (name, a.shape, b.shape)
        err, scale = float(np.abs(a - b).max()), max(1.0, float(np.abs(b).max()))
        worst[name] = err / scale
        print("%s %s: max|got - ref| = %.3e, scale %.3e" % (what, name, err, scale))
    for name, v in worst.items():
        assert v <= TOL, (what, name, v)


@pytest.mark.parametrize("with_mask", [True, False], ids=["mask", "nomask"])
@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_entry_against_the_restatement(dev, shape, train, with_mask):
    d = draw_case(shape, train, with_mask, seed=sum(shape) * 4 + 2 * int(train) + int(with_mask))
    ref = head_backward_ref(d["d_out"], d["feat"], d["weight"], d["bn_weight"], d["bn_bias"], d["lin"], d.get("mean"),
                            d.get("invstd"), d.get("running_mean"), d.get("running_var"), d["eps"], d["mask"])
    got = _entry(_to(d, dev))
    assert got is not None
    torch.cuda.synchronize()
    _check(got, ref[:5], "entry %s %s %s" % (shape, "train" if train else "eval", "mask" if with_mask else "nomask"))


def test_split_rule_named_shapes(dev):
    """the shapes above that are named from the split rule do straddle it: the scratch query grows by exactly the partial
    weight gradients, S [C][K] tiles, once there is more than one row range"""
    from ctc_amd import _lib
    q = _lib.load().ctc_amd_head_backward_scratch_bytes
    up = lambda v: (v + 255) // 256 * 256          # noqa: E731
    base = lambda T, B: up(4 * T * B * 48) + up(4 * 3 * T * 48) + 256          # noqa: E731
    assert q(8, 16, 64, 33) == base(8, 16)
    assert q(9, 16, 64, 33) == base(9, 16) + up(4 * 2 * 33 * 64)
    assert q(150, 256, 64, 33) == base(150, 256) + up(4 * 64 * 33 * 64)


def _raw_call(t, T, B, K, C, dout, feat, d_feat, outs, scratch, train):
    """the C entry itself on caller-made buffers; outs: d_weight, d_bias, d_bn_weight, d_bn_bias views"""
    from ctc_amd import _lib
    from ctc_amd import functional as F
    ptr = lambda x: None if x is None else x.data_ptr()          # noqa: E731
    dev = dout.device
    st = (t["mean"], t["invstd"], None, None) if train else (None, None, t["running_mean"], t["running_var"])
    with F._on_device(dev):
        rc = _lib.load().ctc_amd_head_backward(
            dout.data_ptr(), dout.stride(0), dout.stride(1), feat.data_ptr(), feat.stride(0), feat.stride(1),
            t["weight"].data_ptr(), t["bn_weight"].data_ptr(), t["bn_bias"].data_ptr(), t["lin"].data_ptr(),
            *(ptr(x) for x in st), float(t["eps"]), ptr(t["mask"]), T, B, K, C,
            ptr(d_feat), d_feat.stride(0) if d_feat is not None else 0, d_feat.stride(1) if d_feat is not None else 0,
            *(o.data_ptr() for o in outs), scratch.data_ptr(), scratch.numel(), F._stream_handle(dev))
    assert rc == 0, rc


@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("shape", [(4, 37, 64, 40), (7, 16, 48, 17)], ids=lambda s: "x".join(map(str, s)))
def test_layout_and_contract(dev, shape, train):
    from ctc_amd import _lib
    T, B, K, C = shape
    d = draw_case(shape, train, True, seed=1000 + sum(shape) + int(train))
    ref = head_backward_ref(d["d_out"], d["feat"], d["weight"], d["bn_weight"], d["bn_bias"], d["lin"], d.get("mean"),
                            d.get("invstd"), d.get("running_mean"), d.get("running_var"), d["eps"], d["mask"])
    t = _to(d, dev)
    SENT, GUARD = -12345.0, 8
    dout_buf = torch.full((T, B, C + 3), 7.0, device=dev)
    dout_buf[:, :, :C] = t["d_out"]
    dout = dout_buf[:, :, :C]                                # row pitch C + 3
    feat_buf = torch.full((T, B, K + 16), 3.0, device=dev)
    feat_buf[:, :, :K] = t["feat"]
    feat = feat_buf[:, :, :K]                                # row pitch K + 16
    nbytes = _lib.load().ctc_amd_head_backward_scratch_bytes(T, B, K, C)
    assert nbytes > 0
    sizes = (C * K, C, C, C)

    def run(want_dfeat, scratch_fill):
        scratch = torch.full((nbytes,), scratch_fill, dtype=torch.uint8, device=dev)
        dfeat_buf = torch.full((T, B, K + 4), SENT, device=dev) if want_dfeat else None
        bufs = [torch.full((n + 2 * GUARD,), SENT, device=dev) for n in sizes]
        _raw_call(t, T, B, K, C, dout, feat, dfeat_buf[:, :, :K] if want_dfeat else None, [b[GUARD:] for b in bufs], scratch, train)
        torch.cuda.synchronize()
        for b in bufs:                                       # the guards on both sides are untouched
            assert bool((b[:GUARD] == SENT).all()) and bool((b[-GUARD:] == SENT).all())
        if want_dfeat:                                       # the pad columns keep the sentinel bit for bit
            assert bool((dfeat_buf[:, :, K:] == SENT).all())
        outs = [b[GUARD:-GUARD].clone() for b in bufs]
        outs[0] = outs[0].reshape(C, K)
        return (dfeat_buf[:, :, :K].clone() if want_dfeat else None), outs

    df_a, outs_a = run(True, 0xFF)
    _check([df_a] + outs_a, ref[:5], "layout %s" % (shape,))
    df_b, outs_b = run(True, 0x00)                           # scratch contents are irrelevant; a second call gives the same bits
    df_c, outs_c = run(True, 0xFF)
    _, outs_d = run(False, 0xFF)                             # d_feat = NULL: the other four unchanged
    for other_df, other in ((df_b, outs_b), (df_c, outs_c), (None, outs_d)):
        if other_df is not None:
            assert torch.equal(df_a, other_df)
        for a, b in zip(outs_a, other):
            assert torch.equal(a, b)


def _layers_f64(lin, bn, feat, mask, up, train):
    """torch's float64 CPU autograd of the layers applied frame by frame, times the mask -> gradients and min |y|"""
    l64, b64 = torch.nn.Linear(lin.in_features, lin.out_features).double(), torch.nn.BatchNorm1d(bn.num_features).double()
    l64.load_state_dict({k: v.detach().cpu().double() for k, v in lin.state_dict().items()})
    b64.load_state_dict({k: (v.detach().cpu().double() if v.is_floating_point() else v.detach().cpu())
                         for k, v in bn.state_dict().items()})
    b64.train(train)
    f = feat.detach().cpu().double().requires_grad_(True)
    ys = [b64(l64(f[t])) for t in range(f.shape[0])]
    out = torch.relu(torch.stack(ys))
    if mask is not None:
        out = out * mask.cpu().double()
    (out * up.cpu().double()).sum().backward()
    ymin = float(torch.stack(ys).detach().abs().min())
    return [f.grad, l64.weight.grad, l64.bias.grad, b64.weight.grad, b64.bias.grad], ymin


def _counting(monkeypatch):
    """wrap the bound entry in a counter (the ctypes function object is per library handle: put the wrapper on the handle)"""
    from ctc_amd import _lib
    lib = _lib.load()
    real = lib.ctc_amd_head_backward
    calls = []

    def wrapped(*a):
        calls.append(1)
        return real(*a)
    monkeypatch.setattr(lib, "ctc_amd_head_backward", wrapped)
    return calls


# seeds for which no BatchNorm output of the float64 layers lies within MARGIN of the ReLU's corner (asserted below)
@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("shape", [(5, 10, 1024, 33), (2, 2, 16, 5)], ids=lambda s: "x".join(map(str, s)))
def test_headfn_through_the_gate(dev, monkeypatch, shape, train):
    from ctc_amd import producer
    T, B, K, C = shape
    for seed in range(200):
        g = torch.Generator().manual_seed(7000 + seed)
        rnd = lambda *s: (torch.rand(*s, generator=g) * 2 - 1)          # noqa: E731
        lin, bn = torch.nn.Linear(K, C), torch.nn.BatchNorm1d(C)
        with torch.no_grad():
            lin.weight.copy_(rnd(C, K) * 0.1); lin.bias.copy_(rnd(C) * 0.1)
            bn.weight.copy_(rnd(C) * 0.5 + 1.0); bn.bias.copy_(rnd(C) * 0.2)
            bn.running_mean.copy_(rnd(C) * 0.3); bn.running_var.copy_(rnd(C) * 0.4 + 1.0)
        mask = (rnd(T, B, C) > -0.4).float() / 0.7
        up, leaves = rnd(T, B, C), rnd(T, B, K)
        ref, ymin = _layers_f64(lin, bn, leaves, mask, up, train)
        if ymin >= MARGIN:
            break
    assert ymin >= MARGIN                                    # no ReLU decision hangs on a rounding
    lin, bn = lin.to(dev), bn.to(dev)
    mask, up, leaves = mask.to(dev), up.to(dev), leaves.to(dev)
    calls = _counting(monkeypatch)
    res = {}
    for gate in (1 << 30, 0):
        monkeypatch.setattr(producer, "HEAD_BACKWARD_MAX_ROWS", gate)
        feat = leaves.clone().requires_grad_(True)
        lin.zero_grad(); bn.zero_grad()
        before = len(calls)
        st = (None, None) if train else (bn.running_mean, bn.running_var)
        out = producer._HeadFn.apply(feat, lin.weight, lin.bias, bn.weight, bn.bias, st[0], st[1], bn.eps, mask)[0]
        (out * up).sum().backward()
        torch.cuda.synchronize()
        assert len(calls) - before == (1 if gate else 0)     # gate 0: the entry is not reached
        res[gate] = [feat.grad, lin.weight.grad.clone(), lin.bias.grad.clone(), bn.weight.grad.clone(), bn.bias.grad.clone()]
    skip = ("d_bias",) if train else ()                      # identically 0 under batch statistics: rounding noise on both sides
    _check(res[1 << 30], ref, "HeadFn open %s" % (shape,), skip)
    _check(res[0], ref, "HeadFn closed %s" % (shape,), skip)
    _check(res[1 << 30], res[0], "HeadFn open against closed %s" % (shape,), skip)


@pytest.mark.parametrize("shape", [(5, 10, 1024, 33), (2, 2, 16, 5)], ids=lambda s: "x".join(map(str, s)))
def test_lstm_cell_train_step_through_the_gate(dev, monkeypatch, shape):
    """a train-mode LSTM_cell step (dropout off: the mask is torch's own draw otherwise) against the float64 CPU autograd of
    the same layers and nn.LSTMCell, with the gate open"""
    import ctc_amd
    from ctc_amd import producer
    T, B, K, C = shape
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
        # float64 on the CPU: the layers frame by frame, then the cell
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
    ref = [f.grad, l64.weight.grad, l64.bias.grad, b64.weight.grad, b64.bias.grad]
    model = model.to(dev)
    calls = _counting(monkeypatch)
    monkeypatch.setattr(producer, "HEAD_BACKWARD_MAX_ROWS", 1 << 30)
    feat = leaves.to(dev).requires_grad_(True)
    series = model(feat, h0.to(dev), c0.to(dev))
    (series * up.to(dev)).sum().backward()
    torch.cuda.synchronize()
    assert len(calls) == 1
    lin, bn = model.v.layers[0], model.v.layers[1]
    _check([feat.grad, lin.weight.grad, lin.bias.grad, bn.weight.grad, bn.bias.grad], ref, "LSTM_cell %s" % (shape,), ("d_bias",))


def test_shapes_the_entry_does_not_take(dev, monkeypatch):
    """B = 300 and K = 24: head_backward returns None; the module's backward (whose forward takes neither shape: the layers
    themselves run) still returns gradients with the gate open"""
    import ctc_amd
    from ctc_amd import producer
    g = torch.Generator().manual_seed(11)
    rnd = lambda *s: (torch.rand(*s, generator=g) * 2 - 1).to(dev)          # noqa: E731
    for (T, B, K, C) in ((2, 300, 32, 8), (2, 4, 24, 8)):
        assert ctc_amd.head_backward(rnd(T, B, C), rnd(T, B, K), rnd(C, K), rnd(C), rnd(C), rnd(T, B, C), mean=rnd(T, C),
                                     invstd=rnd(T, C) * 0.4 + 1.0) is None
        assert ctc_amd.head_backward(rnd(T, B, C), rnd(T, B, K), rnd(C, K), rnd(C), rnd(C), rnd(T, B, C), running_mean=rnd(C),
                                     running_var=rnd(C) * 0.4 + 1.0, need_dfeat=False) is None
        monkeypatch.setattr(producer, "HEAD_BACKWARD_MAX_ROWS", 1 << 30)
        model = ctc_amd.LSTM_cell(types.SimpleNamespace(extract_feat_dim=K, v_class=C, batch_size=B, temporal=T)).to(dev).train()
        feat = rnd(T, B, K).requires_grad_(True)
        model(feat, rnd(B, C), rnd(B, C)).sum().backward()
        grads = [feat.grad, model.v.layers[0].weight.grad, model.v.layers[0].bias.grad, model.v.layers[1].weight.grad,
                 model.v.layers[1].bias.grad]
        assert all(x is not None and bool(torch.isfinite(x).all()) for x in grads)


def test_capture(dev):
    """one call captured into a torch.cuda.graph on a side stream and replayed twice gives the eager call's bits (the call is
    two launches on one stream: a single chain, no parallel branches)"""
    shape = (5, 10, 1024, 33)
    t = _to(draw_case(shape, True, True, seed=77), dev)
    eager = _entry(t)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                            # warm-up on the capture stream
        _entry(t)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        captured = _entry(t)
    for _ in range(2):
        for x in captured:
            x.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(eager, captured):
            assert torch.equal(a, b)
