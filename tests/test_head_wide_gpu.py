"""The head for batches beyond 256 samples (ctc_amd_head_forward_wide / ctc_amd_head_backward_wide and their wrappers) on the
device: the forward against the narrow entry's bits (Linear output, eval mode) and against the float64 restatement
(tests/head_forward_ref.py: train mode), the backward against tests/head_backward_ref.py, the layout and determinism
contract, stream capture, and the module path through the two gates.

Measured maxima of |got - ref| / max(1, max|ref|) over all cases (bound 1e-4): see profiles/r18_head_wide.md."""
import copy
import functools
import types

import numpy as np
import pytest
import torch

from tests.head_backward_ref import draw_case, head_backward_ref
from tests.head_forward_ref import OFFSET, OFFSET_SHAPE, TOL, draw_forward_case, head_forward_ref

pytestmark = pytest.mark.gpu

CORNER = 1e-5                                                # test_lstm_cell_through_the_gates: distance from the ReLU's corner
ROWS = 256                                                   # rows of a row block (kHeadWideRows), the narrow entry's bound on B
# (T, B, K, C): the smallest at which something can go wrong.
#   (2, 257, 16, 5)     the first B with a second row block, which holds one row; one k-block (head_dot adds its zero second
#                       batch); C below one column tile
#   (1, 512, 32, 16)    two full row blocks, T = 1, one exact column tile
#   (2, 300, 32, 8)     the shape of the existing fall-back tests
#   (3, 511, 48, 17)    the last block one row short, the second column tile holds one column, an odd count of k-blocks
#   (2, 2048, 64, 33)   BASELINE config 4's batch at the reference's class count (three column tiles: one group of three)
#   (2, 2048, 1024, 33) the same at the reference's K
#   (1, 1000, 64, 158)  the benchmark's C: ten column tiles in four groups of 3, 3, 3, 1
#   (2, 300, 16, 50)    four column tiles: two groups of two (the host's rule: NG = ceil(CT / 3), N = ceil(CT / NG))
#   (4, 37, 64, 40), (2, 2, 16, 5)   B <= 256 through the wide entry
SHAPES = [(2, 257, 16, 5), (1, 512, 32, 16), (2, 300, 32, 8), (3, 511, 48, 17), (2, 2048, 64, 33), (2, 2048, 1024, 33),
          (1, 1000, 64, 158), (2, 300, 16, 50), (4, 37, 64, 40), (2, 2, 16, 5)]
BWD_NAMES = ("d_feat", "d_weight", "d_bias", "d_bn_weight", "d_bn_bias")
ids = lambda s: "x".join(map(str, s))          # noqa: E731


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    import ctc_amd  # noqa: F401
    return torch.device("cuda:0")


def _to(d, dev):
    return {k: (torch.from_numpy(v).to(dev) if isinstance(v, np.ndarray) else v) for k, v in d.items()}


@functools.lru_cache(maxsize=None)
def _fwd_case(shape, train, with_mask, offset=0.0):
    """inputs and the float64 restatement, computed once per case and left unchanged"""
    d = draw_forward_case(shape, train, with_mask, seed=sum(shape) * 4 + 2 * int(train) + int(with_mask), offset=offset)
    ref = head_forward_ref(d["feat"], d["weight"], d["bias"], d["bn_weight"], d["bn_bias"], d.get("running_mean"),
                           d.get("running_var"), d["eps"], d["mask"])
    return d, ref


@functools.lru_cache(maxsize=None)
def _bwd_case(shape, train, with_mask):
    d = draw_case(shape, train, with_mask, seed=sum(shape) * 4 + 2 * int(train) + int(with_mask))
    ref = head_backward_ref(d["d_out"], d["feat"], d["weight"], d["bn_weight"], d["bn_bias"], d["lin"], d.get("mean"),
                            d.get("invstd"), d.get("running_mean"), d.get("running_var"), d["eps"], d["mask"])
    return d, ref[:5]


def _forward(t, wide=True, state=True, feat=None, mask=None):
    import ctc_amd
    f = ctc_amd.head_forward_wide if wide else ctc_amd.head_forward
    return f(t["feat"] if feat is None else feat, t["weight"], t["bias"], t["bn_weight"], t["bn_bias"], t.get("running_mean"),
             t.get("running_var"), t["eps"], t["mask"] if mask is None else mask, want_backward_state=state)


def _backward(t, need_dfeat=True):
    import ctc_amd
    return ctc_amd.head_backward_wide(t["d_out"], t["feat"], t["weight"], t["bn_weight"], t["bn_bias"], t["lin"], t.get("mean"),
                                      t.get("invstd"), t.get("running_mean"), t.get("running_var"), t["eps"], t["mask"],
                                      need_dfeat)


def _check(names, got, ref, what, skip=()):
    worst = {}
    for name, a, b in zip(names, got, ref):
        if name in skip or (a is None and b is None):
            continue
        a = a.detach().cpu().numpy().astype(np.float64) if torch.is_tensor(a) else np.asarray(a, np.float64)
        b = b.detach().cpu().numpy().astype(np.float64) if torch.is_tensor(b) else np.asarray(b, np.float64)
        assert a.shape == b.shape, (name, a.shape, b.shape)
        err, scale = float(np.abs(a - b).max()), max(1.0, float(np.abs(b).max()))
        worst[name] = err / scale
        print("%s %s: max|got - ref| = %.3e, scale %.3e" % (what, name, err, scale))
    for name, v in worst.items():
        assert v <= TOL, (what, name, v)


# ------------------------------------------------------------------------------------------------------------- forward

@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_linear_output_is_the_narrow_entry_bit_for_bit(dev, shape):
    """lin has no cross-row term and shares head_dot: the wide entry's lin (train mode and eval mode) equals the narrow entry's
    on every batch slice of 256 rows (the narrow entry in eval mode: a slice may hold one row)"""
    T, B, K, C = shape
    t_train = _to(_fwd_case(shape, True, False)[0], dev)
    t_eval = _to(_fwd_case(shape, False, False)[0], dev)
    t_eval.update(feat=t_train["feat"], weight=t_train["weight"], bias=t_train["bias"])
    lin_train, lin_eval = _forward(t_train)[1], _forward(t_eval)[1]
    assert lin_train.shape == lin_eval.shape == (T, B, C)
    for i in range(0, B, ROWS):
        narrow = _forward(t_eval, wide=False, feat=t_eval["feat"][:, i:i + ROWS])
        assert narrow is not None
        assert torch.equal(lin_train[:, i:i + ROWS], narrow[1]), (shape, i, "train")
        assert torch.equal(lin_eval[:, i:i + ROWS], narrow[1]), (shape, i, "eval")


@pytest.mark.parametrize("with_mask", [True, False], ids=["mask", "nomask"])
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_eval_mode_is_the_narrow_entry_bit_for_bit(dev, shape, with_mask):
    T, B, K, C = shape
    d, ref = _fwd_case(shape, False, with_mask)
    t = _to(d, dev)
    for state in (False, True):                              # (without and with linear_out)
        got = _forward(t, state=state)
        assert got is not None and got[2] is None and got[3] is None and got[4] is None
        for i in range(0, B, ROWS):
            narrow = _forward(t, wide=False, feat=t["feat"][:, i:i + ROWS],
                              mask=t["mask"][:, i:i + ROWS] if with_mask else None)
            assert torch.equal(got[0][:, i:i + ROWS], narrow[0]), (shape, i)
    _check(("out", "lin"), got[:2], ref[:2], "forward eval %s" % (shape,))


@pytest.mark.parametrize("with_mask", [True, False], ids=["mask", "nomask"])
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_train_mode_against_the_restatement(dev, shape, with_mask):
    d, ref = _fwd_case(shape, True, with_mask)
    t = _to(d, dev)
    got = _forward(t)
    assert got is not None
    torch.cuda.synchronize()
    _check(("out", "lin", "mean", "var", "invstd"), got, ref, "forward train %s %s" % (shape, "mask" if with_mask else "nomask"))
    # without linear_out the Linear output lives in the scratch: the same bits
    bare = _forward(t, state=False)
    assert bare[1] is None
    for i in (0, 2, 3, 4):
        assert torch.equal(got[i], bare[i]), i


def test_train_mode_with_a_common_offset(dev):
    """lin ~ 1000 + noise: the variance is the centred second moment of a second pass; E[x^2] - mean^2 in fp32 is off by ~1
    here (tests/test_head_wide_abi.py shows both on the CPU).  Held to the bound: lin and the statistics.  Not out: an fp32 lin
    near 1000 is rounded to 6.1e-5, which BatchNorm multiplies by invstd gamma ~ 3 -- the bound itself, whatever the kernel."""
    d, ref = _fwd_case(OFFSET_SHAPE, True, False, OFFSET)
    got = _forward(_to(d, dev))
    torch.cuda.synchronize()
    assert abs(float(got[2].mean()) - OFFSET) < 1.0
    _check(("lin", "mean", "var", "invstd"), got[1:], ref[1:], "forward train offset %s" % (OFFSET_SHAPE,))


def _raw_forward(t, T, B, K, C, feat, out, lin, stats, scratch):
    from ctc_amd import _lib
    from ctc_amd import functional as F
    ptr = lambda x: None if x is None else x.data_ptr()          # noqa: E731
    dev = out.device
    with F._on_device(dev):
        rc = _lib.load().ctc_amd_head_forward_wide(
            feat.data_ptr(), feat.stride(0), feat.stride(1), t["weight"].data_ptr(), t["bias"].data_ptr(),
            t["bn_weight"].data_ptr(), t["bn_bias"].data_ptr(), ptr(t.get("running_mean")), ptr(t.get("running_var")),
            float(t["eps"]), ptr(t["mask"]), T, B, K, C, out.data_ptr(), out.stride(0), out.stride(1), ptr(lin),
            *(ptr(s) for s in stats), scratch.data_ptr(), scratch.numel(), F._stream_handle(dev))
    assert rc == 0, rc


@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("shape", [(2, 300, 32, 8), (3, 511, 48, 17)], ids=ids)
def test_forward_layout_and_contract(dev, shape, train):
    """strided feat and out rows, the bytes between out rows untouched, guards around every other output, scratch contents
    irrelevant (0xFF bytes: NaN), every element of every output written, a second call gives the same bits"""
    from ctc_amd import _lib
    T, B, K, C = shape
    d, ref = _fwd_case(shape, train, True)
    t = _to(d, dev)
    SENT, GUARD = -12345.0, 8
    feat_buf = torch.full((T, B, K + 16), 3.0, device=dev)
    feat_buf[:, :, :K] = t["feat"]
    nbytes = _lib.load().ctc_amd_head_forward_wide_scratch_bytes(T, B, K, C)
    assert nbytes > 0
    sizes = (T * B * C,) + ((T * C,) * 3 if train else ())

    def run(fill, offset):
        scratch = torch.full((nbytes + offset,), fill, dtype=torch.uint8, device=dev)[offset:]     # (any alignment)
        out_buf = torch.full((T, B, C + 3), SENT, device=dev)
        bufs = [torch.full((n + 2 * GUARD,), SENT, device=dev) for n in sizes]
        views = [b[GUARD:] for b in bufs]
        _raw_forward(t, T, B, K, C, feat_buf[:, :, :K], out_buf[:, :, :C], views[0], views[1:] if train else (None,) * 3, scratch)
        torch.cuda.synchronize()
        assert bool((out_buf[:, :, C:] == SENT).all())
        for b in bufs:
            assert bool((b[:GUARD] == SENT).all()) and bool((b[-GUARD:] == SENT).all())
            assert not bool((b[GUARD:-GUARD] == SENT).any())
        outs = [out_buf[:, :, :C].clone()] + [b[GUARD:-GUARD].clone() for b in bufs]
        outs[1] = outs[1].reshape(T, B, C)
        return [o.reshape(T, C) if o.numel() == T * C and o.dim() == 1 else o for o in outs]

    a = run(0xFF, 0)
    _check(("out", "lin", "mean", "var", "invstd"), a, ref, "forward layout %s" % (shape,))
    for other in (run(0x00, 4), run(0xFF, 1)):
        for x, y in zip(a, other):
            assert torch.equal(x, y)


# ------------------------------------------------------------------------------------------------------------ backward

@pytest.mark.parametrize("need_dfeat", [True, False], ids=["dfeat", "nodfeat"])
@pytest.mark.parametrize("with_mask", [True, False], ids=["mask", "nomask"])
@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_backward_against_the_restatement(dev, shape, train, with_mask, need_dfeat):
    d, ref = _bwd_case(shape, train, with_mask)
    got = _backward(_to(d, dev), need_dfeat)
    assert got is not None and (got[0] is None) == (not need_dfeat)
    torch.cuda.synchronize()
    _check(BWD_NAMES, got, ref, "backward %s %s %s" % (shape, "train" if train else "eval", "mask" if with_mask else "nomask"),
           skip=() if need_dfeat else ("d_feat",))


def _raw_backward(t, T, B, K, C, dout, feat, d_feat, outs, scratch, train):
    from ctc_amd import _lib
    from ctc_amd import functional as F
    ptr = lambda x: None if x is None else x.data_ptr()          # noqa: E731
    dev = dout.device
    st = (t["mean"], t["invstd"], None, None) if train else (None, None, t["running_mean"], t["running_var"])
    with F._on_device(dev):
        rc = _lib.load().ctc_amd_head_backward_wide(
            dout.data_ptr(), dout.stride(0), dout.stride(1), feat.data_ptr(), feat.stride(0), feat.stride(1),
            t["weight"].data_ptr(), t["bn_weight"].data_ptr(), t["bn_bias"].data_ptr(), t["lin"].data_ptr(),
            *(ptr(x) for x in st), float(t["eps"]), ptr(t["mask"]), T, B, K, C,
            ptr(d_feat), d_feat.stride(0) if d_feat is not None else 0, d_feat.stride(1) if d_feat is not None else 0,
            *(o.data_ptr() for o in outs), scratch.data_ptr(), scratch.numel(), F._stream_handle(dev))
    assert rc == 0, rc


@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("shape", [(2, 300, 32, 8), (3, 511, 48, 17)], ids=ids)
def test_backward_layout_and_contract(dev, shape, train):
    """tests/test_head_backward_gpu.py's layout test on the wide entry: unrelated bytes around strided d_feat rows stay
    untouched, the scratch may be pre-filled with NaN (0xFF bytes), two calls give the same bits"""
    from ctc_amd import _lib
    T, B, K, C = shape
    d, ref = _bwd_case(shape, train, True)
    t = _to(d, dev)
    SENT, GUARD = -12345.0, 8
    dout_buf = torch.full((T, B, C + 3), 7.0, device=dev)
    dout_buf[:, :, :C] = t["d_out"]
    feat_buf = torch.full((T, B, K + 16), 3.0, device=dev)
    feat_buf[:, :, :K] = t["feat"]
    nbytes = _lib.load().ctc_amd_head_backward_wide_scratch_bytes(T, B, K, C)
    assert nbytes > 0
    sizes = (C * K, C, C, C)

    def run(want_dfeat, fill, offset=0):
        scratch = torch.full((nbytes + offset,), fill, dtype=torch.uint8, device=dev)[offset:]
        dfeat_buf = torch.full((T, B, K + 4), SENT, device=dev) if want_dfeat else None
        bufs = [torch.full((n + 2 * GUARD,), SENT, device=dev) for n in sizes]
        _raw_backward(t, T, B, K, C, dout_buf[:, :, :C], feat_buf[:, :, :K], dfeat_buf[:, :, :K] if want_dfeat else None,
                      [b[GUARD:] for b in bufs], scratch, train)
        torch.cuda.synchronize()
        for b in bufs:
            assert bool((b[:GUARD] == SENT).all()) and bool((b[-GUARD:] == SENT).all())
        if want_dfeat:
            assert bool((dfeat_buf[:, :, K:] == SENT).all())
        outs = [b[GUARD:-GUARD].clone() for b in bufs]
        outs[0] = outs[0].reshape(C, K)
        return (dfeat_buf[:, :, :K].clone() if want_dfeat else None), outs

    df_a, outs_a = run(True, 0xFF)
    _check(BWD_NAMES, [df_a] + outs_a, ref, "backward layout %s" % (shape,))
    df_b, outs_b = run(True, 0x00, 4)
    df_c, outs_c = run(True, 0xFF, 1)
    _, outs_d = run(False, 0xFF)
    for other_df, other in ((df_b, outs_b), (df_c, outs_c), (None, outs_d)):
        if other_df is not None:
            assert torch.equal(df_a, other_df)
        for a, b in zip(outs_a, other):
            assert torch.equal(a, b)


# --------------------------------------------------------------------------------------------- determinism and capture

def _equal(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert (x is None and y is None) or torch.equal(x, y)


@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
def test_two_eager_calls_give_equal_bits(dev, train):
    shape = (3, 511, 48, 17)
    tf, tb = _to(_fwd_case(shape, train, True)[0], dev), _to(_bwd_case(shape, train, True)[0], dev)
    _equal(_forward(tf), _forward(tf))
    _equal(_backward(tb), _backward(tb))


def _captured(call):
    """one call captured into a torch.cuda.graph on a side stream and replayed twice gives the eager call's bits (each entry is
    a single chain of launches on one stream)"""
    eager = call()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                            # warm-up on the capture stream
        call()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        captured = call()
    for _ in range(2):
        for x in captured:
            if x is not None:
                x.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        _equal(eager, captured)


@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
def test_forward_capture(dev, train):
    t = _to(_fwd_case((3, 511, 48, 17), train, True)[0], dev)
    _captured(lambda: _forward(t))


@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
def test_backward_capture(dev, train):
    t = _to(_bwd_case((3, 511, 48, 17), train, True)[0], dev)
    _captured(lambda: _backward(t))


# --------------------------------------------------------------------------------------------------------- the module

def _spies(monkeypatch):
    from ctc_amd import producer
    calls = {"head_forward_wide": 0, "head_backward_wide": 0}

    def spy(name):
        real = getattr(producer, name)

        def wrapped(*a, **kw):
            calls[name] += 1
            res = real(*a, **kw)
            assert res is not None
            return res
        monkeypatch.setattr(producer, name, wrapped)
    for name in calls:
        spy(name)
    return calls


@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("B", [300, 512])
def test_lstm_cell_through_the_gates(dev, monkeypatch, B, train):
    """LSTM_cell at B > 256 (train mode with dropout off: the mask is torch's own draw otherwise; eval mode) with both gates
    open and with both at 0, against torch's own layers applied frame by frame on the device in front of the same recurrence:
    v_series, the gradients and the BatchNorm buffers after the step.  d_bias is skipped in train mode: identically 0 under
    batch statistics, rounding noise on both sides."""
    import ctc_amd
    from ctc_amd import producer
    T, K, C = 3, 64, 33
    args = types.SimpleNamespace(extract_feat_dim=K, v_class=C, batch_size=B, temporal=T)
    # a draw with no BatchNorm output within CORNER of the ReLU's corner: the fp32 paths differ by ~1e-7 K |x w| <= 1e-6 there
    # (K = 64, |x w| <= 1 / 8), so 1e-5 leaves a factor of ten (MARGIN = 1e-4 has no such draw at 50688 outputs in eval mode)
    for seed in range(400):
        torch.manual_seed(31000 + seed)
        base = ctc_amd.LSTM_cell(args).train(train)
        base.v.layers[3].p = 0.0
        g = torch.Generator().manual_seed(seed)
        rnd = lambda *s: (torch.rand(*s, generator=g) * 2 - 1)          # noqa: E731
        lin, bn = base.v.layers[0], base.v.layers[1]
        with torch.no_grad():
            bn.weight.copy_(rnd(C) * 0.5 + 1.0); bn.bias.copy_(rnd(C) * 0.2)
            bn.running_mean.copy_(rnd(C) * 0.3); bn.running_var.copy_(rnd(C) * 0.4 + 1.0)
        leaves, h0, c0, up = rnd(T, B, K), rnd(B, C) * 0.1, rnd(B, C) * 0.1, rnd(T, B, C)
        l64, b64 = copy.deepcopy(lin).double(), copy.deepcopy(bn).double()
        with torch.no_grad():
            ymin = float(torch.stack([b64(l64(leaves[t].double())) for t in range(T)]).abs().min())
        if ymin >= CORNER:
            break
    assert ymin >= CORNER                                   # no ReLU decision hangs on a rounding
    h0, c0, up, leaves = h0.to(dev), c0.to(dev), up.to(dev), leaves.to(dev)

    def grads_and_buffers(model, feat, series):
        (series * up).sum().backward()
        torch.cuda.synchronize()
        lin, bn = model.v.layers[0], model.v.layers[1]
        return [series.detach(), feat.grad, lin.weight.grad, lin.bias.grad, bn.weight.grad, bn.bias.grad,
                bn.running_mean.clone(), bn.running_var.clone(), bn.num_batches_tracked.clone().double()]

    names = ("v_series", "d_feat", "d_weight", "d_bias", "d_bn_weight", "d_bn_bias", "running_mean", "running_var",
             "num_batches_tracked")
    # torch's layers frame by frame, then the recurrence the module runs behind its head
    model = copy.deepcopy(base).to(dev)
    feat = leaves.clone().requires_grad_(True)
    v_all = torch.stack([model.v(feat[t]) for t in range(T)])
    cell = model.v_cell
    ref = grads_and_buffers(model, feat, producer._SeriesFn.apply(v_all, h0, c0, cell.weight_ih, cell.weight_hh, cell.bias_ih,
                                                                  cell.bias_hh, C, producer.PAD_LOGIT))
    assert int(ref[-1]) == (T if train else 0)
    calls = _spies(monkeypatch)
    skip = ("d_bias",) if train else ()
    for gate in (1 << 30, 0):
        monkeypatch.setattr(producer, "HEAD_WIDE_MAX_ROWS", gate)
        monkeypatch.setattr(producer, "HEAD_WIDE_BACKWARD_MAX_ROWS", gate)
        before = dict(calls)
        model = copy.deepcopy(base).to(dev)
        feat = leaves.clone().requires_grad_(True)
        got = grads_and_buffers(model, feat, model(feat, h0, c0))
        for name in calls:                                   # open: each wide entry exactly once; 0: not reached
            assert calls[name] - before[name] == (1 if gate else 0), (name, gate)
        _check(names, got, ref, "LSTM_cell B=%d %s gates %s" % (B, "train" if train else "eval", "open" if gate else "0"), skip)
        assert int(got[-1]) == int(ref[-1])


def test_lstm_cell_backward_gate_alone(dev, monkeypatch):
    """the forward's gate open and the backward's at 0: the wide forward's saved state feeds _head_backward_torch"""
    import ctc_amd
    from ctc_amd import producer
    T, B, K, C = 2, 300, 32, 8
    calls = _spies(monkeypatch)
    monkeypatch.setattr(producer, "HEAD_WIDE_MAX_ROWS", 1 << 30)
    monkeypatch.setattr(producer, "HEAD_WIDE_BACKWARD_MAX_ROWS", 0)
    torch.manual_seed(5)
    base = ctc_amd.LSTM_cell(types.SimpleNamespace(extract_feat_dim=K, v_class=C, batch_size=B, temporal=T)).to(dev).train()
    base.v.layers[3].p = 0.0
    g = torch.Generator().manual_seed(12)
    rnd = lambda *s: (torch.rand(*s, generator=g) * 2 - 1).to(dev)          # noqa: E731
    leaves, h0, c0 = rnd(T, B, K), rnd(B, C), rnd(B, C)
    res = []
    for open_bwd in (False, True):
        monkeypatch.setattr(producer, "HEAD_WIDE_BACKWARD_MAX_ROWS", (1 << 30) if open_bwd else 0)
        model = copy.deepcopy(base)
        feat = leaves.clone().requires_grad_(True)
        model(feat, h0, c0).sum().backward()
        torch.cuda.synchronize()
        res.append([feat.grad, model.v.layers[0].weight.grad, model.v.layers[1].weight.grad, model.v.layers[1].bias.grad])
    assert calls == {"head_forward_wide": 2, "head_backward_wide": 1}
    _check(("d_feat", "d_weight", "d_bn_weight", "d_bn_bias"), res[1], res[0], "backward gate alone")
