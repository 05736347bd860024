"""The producer's head on bf16 / fp16 features read natively (the *_typed entries behind head_forward, head_forward_wide,
lstm_forward, head_backward, head_backward_wide) on the device.  The contract is bitwise, no tolerances: every
forward output and the four parameter gradients equal the fp32 entry's on feat.float(), d_feat equals the fp32 entry's d_feat
rounded once to feat's dtype.  Shapes: the smallest at which the typed path can go wrong -- K / 16 = 1 and 3 (the odd count's
zero second batch) and 2, B and C off the 16-row and 16-column tiles, one and two row ranges of the weight gradient, the
wide entries' second row block -- plus views that are 8-byte but not 16-byte aligned, fp16 subnormals, the module, stream
capture, and the views the typed entries refuse (the cast path)."""
import copy
import functools
import types

import numpy as np
import pytest
import torch

from tests.head_backward_ref import draw_case
from tests.head_forward_ref import draw_forward_case

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
dt_id = lambda d: str(d).split(".")[-1]        # noqa: E731
ids = lambda s: "x".join(map(str, s))          # noqa: E731
FWD_NAMES = ("out", "lin", "mean", "var", "invstd")
BWD_NAMES = ("d_feat", "d_weight", "d_bias", "d_bn_weight", "d_bn_bias")
# fp16 values below 2^-14: a widening that flushed them would change lin by up to 3e-5 * |w| ~ 1e-5, a hundred ulps of lin ~ 1
SUBNORMALS = [6e-8, -1.2e-7, 9e-7, -4e-6, 1.7e-5, 3e-5, -3e-5, 2.4e-7]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    import ctc_amd  # noqa: F401
    return torch.device("cuda:0")


@pytest.fixture
def calls(monkeypatch):
    """(entry, typed) of every head call: which of them read feat natively"""
    from ctc_amd import producer
    seen = []
    real = producer._feat_call

    def spy(name, feat, pre, post):
        rc, typed = real(name, feat, pre, post)
        seen.append((name, typed))
        return rc, typed
    monkeypatch.setattr(producer, "_feat_call", spy)
    return seen


def _to(d, dev):
    return {k: (torch.from_numpy(v).to(dev) if isinstance(v, np.ndarray) else v) for k, v in d.items()}


@functools.lru_cache(maxsize=None)
def _fwd_case(shape, train, with_mask):
    return draw_forward_case(shape, train, with_mask, seed=sum(shape) * 4 + 2 * int(train) + int(with_mask))


@functools.lru_cache(maxsize=None)
def _bwd_case(shape, train, with_mask):
    return draw_case(shape, train, with_mask, seed=sum(shape) * 4 + 2 * int(train) + int(with_mask))


def _lowp(feat, dtype, layout="dense"):
    """feat [T,B,K] fp32 -> the 2-byte operand.  fp16: the first eight features of every third row are subnormals.
    layout "view": row pitch K + 4 at a storage offset of 4 elements (8-byte aligned, not 16-byte aligned);
    "odd": storage offset 1 element (address = 2 mod 8); "pitch2": row pitch K + 2 (a stride that is no multiple of 4)."""
    T, B, K = feat.shape
    f = feat.to(dtype)
    if dtype is torch.float16:
        sub = torch.tensor(SUBNORMALS, dtype=torch.float16, device=feat.device)
        assert bool((sub != 0).all()) and float(sub.abs().max()) < 2.0 ** -14
        f.view(T * B, K)[::3, :8] = sub
    if layout == "dense":
        return f
    pad, off = {"view": (4, 4), "odd": (0, 1), "pitch2": (2, 0)}[layout]
    buf = torch.full((T * B * (K + pad) + off,), 3.0, dtype=dtype, device=feat.device)
    v = buf[off:].view(T, B, K + pad)[:, :, :K]
    v.copy_(f)
    assert v.data_ptr() % 16 == (2 * off) % 16 and v.stride() == (B * (K + pad), K + pad, 1)
    return v


def _bits(t):
    return t.detach().contiguous().view(torch.int32 if t.dtype is torch.float32 else torch.int16)


def _assert_bitwise(names, got, want, what):
    assert len(got) == len(want)
    for name, a, b in zip(names, got, want):
        if a is None or b is None:
            assert a is None and b is None, (what, name)
            continue
        assert a.dtype is b.dtype and a.shape == b.shape, (what, name, a.dtype, b.dtype, a.shape, b.shape)
        same = torch.equal(_bits(a), _bits(b))
        assert same, (what, name, float((a.float() - b.float()).abs().max()))


def _forward(f, t, feat, state=True):
    return f(feat, t["weight"], t["bias"], t["bn_weight"], t["bn_bias"], t.get("running_mean"), t.get("running_var"), t["eps"],
             t["mask"], want_backward_state=state)


def _backward(f, t, feat, need_dfeat):
    return f(t["d_out"], feat, t["weight"], t["bn_weight"], t["bn_bias"], t["lin"], t.get("mean"), t.get("invstd"),
             t.get("running_mean"), t.get("running_var"), t["eps"], t["mask"], need_dfeat)


def _rounded(res, dtype):
    """the fp32 entry's results with d_feat rounded once to the features' dtype"""
    return (None if res[0] is None else res[0].to(dtype),) + tuple(res[1:])


# ------------------------------------------------------------------------------------------------------------- forward

@pytest.mark.parametrize("layout", ["dense", "view"])
@pytest.mark.parametrize("with_mask", [True, False], ids=["mask", "nomask"])
@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("shape", [(2, 10, 16, 8), (3, 17, 48, 33), (2, 64, 32, 17)], ids=ids)
@pytest.mark.parametrize("dtype", DTYPES, ids=dt_id)
def test_forward_narrow(dev, calls, dtype, shape, train, with_mask, layout):
    import ctc_amd
    t = _to(_fwd_case(shape, train, with_mask), dev)
    feat = _lowp(t["feat"], dtype, layout)
    got = _forward(ctc_amd.head_forward, t, feat)
    assert got is not None and calls == [("ctc_amd_head_forward", True)]
    want = _forward(ctc_amd.head_forward, t, feat.float())
    torch.cuda.synchronize()
    _assert_bitwise(FWD_NAMES, got, want, "forward %s %s" % (shape, layout))
    assert all(x is None or x.dtype is torch.float32 for x in got)
    assert (got[2] is None) == (not train) and float(got[0].abs().max()) > 0


def test_fp16_subnormals_reach_the_product(dev):
    """the case the subnormals are there for: with them zeroed (what a flushing conversion would make of them) lin changes"""
    import ctc_amd
    t = _to(_fwd_case((2, 10, 16, 8), False, False), dev)
    feat = _lowp(t["feat"], torch.float16)
    flushed = torch.where(feat.abs() < 2.0 ** -14, torch.zeros_like(feat), feat)
    assert int((flushed != feat).sum()) >= 8
    a, b = _forward(ctc_amd.head_forward, t, feat)[1], _forward(ctc_amd.head_forward, t, flushed)[1]
    assert not torch.equal(a, b)


@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("shape", [(2, 300, 32, 8), (3, 511, 48, 17)], ids=ids)
@pytest.mark.parametrize("dtype", DTYPES, ids=dt_id)
def test_forward_wide(dev, calls, dtype, shape, train):
    import ctc_amd
    t = _to(_fwd_case(shape, train, True), dev)
    for layout, state in (("dense", True), ("view", False)):
        feat = _lowp(t["feat"], dtype, layout)
        got = _forward(ctc_amd.head_forward_wide, t, feat, state)
        assert got is not None and calls[-1] == ("ctc_amd_head_forward_wide", True)
        want = _forward(ctc_amd.head_forward_wide, t, feat.float(), state)
        torch.cuda.synchronize()
        _assert_bitwise(FWD_NAMES, got, want, "forward wide %s %s" % (shape, layout))


def _cell_inputs(dev, T, B, K, C):
    g = torch.Generator().manual_seed(sum((T, B, K, C)))
    rnd = lambda *s: (torch.rand(*s, generator=g) * 2 - 1).to(dev)          # noqa: E731
    head = dict(weight=rnd(C, K) * (3.0 / K) ** 0.5, bias=rnd(C), bn_weight=0.5 + rnd(C).abs(), bn_bias=0.3 * rnd(C),
                running_mean=0.5 * rnd(C) + 0.1, running_var=(0.5 + 1.5 * torch.rand(C, generator=g)).to(dev), eps=1e-5)
    cell = dict(h0=rnd(B, C), c0=rnd(B, C), w_ih=0.4 * rnd(4 * C, C), w_hh=0.4 * rnd(4 * C, C), b_ih=rnd(4 * C), b_hh=rnd(4 * C))
    return rnd(T, B, K), head, cell


@pytest.mark.parametrize("shape", [(3, 5, 32, 8), (4, 6, 48, 33)], ids=ids)
@pytest.mark.parametrize("dtype", DTYPES, ids=dt_id)
def test_one_launch_eval(dev, calls, dtype, shape):
    import ctc_amd
    T, B, K, C = shape
    feat32, head, cell = _cell_inputs(dev, *shape)
    for layout, cols in (("dense", C), ("view", C + 1)):
        feat = _lowp(feat32, dtype, layout)
        got = ctc_amd.lstm_forward(feat, *head.values(), *cell.values(), cols)
        assert got is not None and calls[-1] == ("ctc_amd_lstm_forward", True)
        want = ctc_amd.lstm_forward(feat.float(), *head.values(), *cell.values(), cols)
        torch.cuda.synchronize()
        _assert_bitwise(("v_series",), (got,), (want,), "one launch %s %s" % (shape, layout))
        assert got.dtype is torch.float32 and got.shape == (T, B, cols)


# ------------------------------------------------------------------------------------------------------------ backward

@pytest.mark.parametrize("need_dfeat", [True, False], ids=["dfeat", "nodfeat"])
@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("shape", [(2, 10, 16, 8), (5, 28, 48, 33), (2, 300, 32, 8)], ids=ids)
@pytest.mark.parametrize("dtype", DTYPES, ids=dt_id)
def test_backward(dev, calls, dtype, shape, train, need_dfeat):
    """(2, 10, 16, 8): one row range of the weight gradient; (5, 28, 48, 33): T B = 140, two ranges of 80 and the reduce launch;
    (2, 300, 32, 8): the wide entry (five ranges)"""
    import ctc_amd
    wide = shape[1] > 256
    f = ctc_amd.head_backward_wide if wide else ctc_amd.head_backward
    t = _to(_bwd_case(shape, train, True), dev)
    for layout in ("dense", "view"):
        feat = _lowp(t["feat"], dtype, layout)
        got = _backward(f, t, feat, need_dfeat)
        assert got is not None and calls[-1] == ("ctc_amd_head_backward_wide" if wide else "ctc_amd_head_backward", True)
        want = _rounded(_backward(f, t, feat.float(), need_dfeat), dtype)
        torch.cuda.synchronize()
        assert (got[0] is None) == (not need_dfeat)
        if need_dfeat:
            assert got[0].dtype is dtype and got[0].shape == feat.shape
        _assert_bitwise(BWD_NAMES, got, want, "backward %s %s" % (shape, layout))


# --------------------------------------------------------------------------------------------------------- the module

def _module_run(base, feat, h0, c0, up, grad):
    """one step of a copy of `base` (the same dropout draw every time) -> (v_series, feat.grad, parameter gradients, buffers)"""
    model = copy.deepcopy(base)
    x = feat.clone().requires_grad_(grad)
    torch.manual_seed(77)
    with torch.set_grad_enabled(grad):
        series = model(x, h0, c0)
    grads = []
    if grad:
        (series * up).sum().backward()
        grads = [p.grad for p in model.parameters()]
    torch.cuda.synchronize()
    bn = model.v.layers[1]
    return series.detach(), x.grad, grads, [bn.running_mean.clone(), bn.running_var.clone()]


@pytest.mark.parametrize("mode", ["eval_one_launch", "train_narrow", "train_wide"])
@pytest.mark.parametrize("dtype", DTYPES, ids=dt_id)
def test_module(dev, calls, dtype, mode):
    """LSTM_cell on the 2-byte features against the same module on feat.float(): v_series, the parameter gradients and the
    running statistics bit for bit; feat.grad in feat's dtype, the fp32 run's rounded once"""
    import ctc_amd
    T, K, C = 3, 32, 8
    B = {"eval_one_launch": 5, "train_narrow": 10, "train_wide": 300}[mode]
    train = mode != "eval_one_launch"
    torch.manual_seed(4100 + B)
    base = ctc_amd.LSTM_cell(types.SimpleNamespace(extract_feat_dim=K, v_class=C, batch_size=B, temporal=T)).to(dev).train(train)
    g = torch.Generator().manual_seed(B)
    rnd = lambda *s: (torch.rand(*s, generator=g) * 2 - 1).to(dev)          # noqa: E731
    feat, h0, c0, up = _lowp(rnd(T, B, K), dtype), rnd(B, C) * 0.1, rnd(B, C) * 0.1, rnd(T, B, C)
    got = _module_run(base, feat, h0, c0, up, train)
    entries = [c for c in calls]
    want = _module_run(base, feat.float(), h0, c0, up, train)
    assert got[0].dtype is torch.float32
    _assert_bitwise(("v_series",), got[:1], want[:1], mode)
    _assert_bitwise(("running_mean", "running_var"), got[3], want[3], mode)
    if not train:
        assert entries == [("ctc_amd_lstm_forward", True)]
        return
    w = "_wide" if B > 256 else ""
    assert entries == [("ctc_amd_head_forward" + w, True), ("ctc_amd_head_backward" + w, True)]
    assert got[1].dtype is dtype and want[1].dtype is torch.float32
    _assert_bitwise(("feat.grad",), (got[1],), (want[1].to(dtype),), mode)
    _assert_bitwise(["grad%d" % i for i in range(len(got[2]))], got[2], want[2], mode)
    assert float(got[1].float().abs().max()) > 0


def test_module_makes_no_fp32_image_of_the_features(dev, calls):
    """T = 4, B = 64, K = 1024, C = 33, train mode, bf16 features as a backbone hands them over (no gradient asked of them:
    d_feat in bf16 alone would be half the bound): forward + backward raise the peak of allocated memory by less than the
    T B K 4 bytes = 1 MiB of one fp32 image of feat.  What the step does allocate is the head's and the recurrence's saved state,
    their scratch and the parameter gradients (the figure is printed: 645120 bytes when this was written, of which the scratch
    of the head's backward is 322 KB and d_weight 135 KB); a cast, in either direction, would add 1 MiB to it."""
    import ctc_amd
    T, B, K, C = 4, 64, 1024, 33
    torch.manual_seed(9)
    model = ctc_amd.LSTM_cell(types.SimpleNamespace(extract_feat_dim=K, v_class=C, batch_size=B, temporal=T)).to(dev).train()
    feat = torch.randn(T, B, K, device=dev).to(torch.bfloat16)
    h0, c0 = torch.zeros(B, C, device=dev), torch.zeros(B, C, device=dev)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    model(feat, h0, c0).sum().backward()
    torch.cuda.synchronize()
    raised = torch.cuda.max_memory_allocated() - before
    print("forward + backward at (%d, %d, %d, %d) raise max_memory_allocated by %d bytes; one fp32 image of feat: %d"
          % (T, B, K, C, raised, T * B * K * 4))
    assert calls == [("ctc_amd_head_forward", True), ("ctc_amd_head_backward", True)]
    assert raised < T * B * K * 4


# ------------------------------------------------------------------------------------------------------------- capture

def _captured(call):
    """one call captured into a torch.cuda.graph behind an eager warm-up on the capture stream, replayed twice: the eager bits"""
    eager = call()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
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
        for a, b in zip(eager, captured):
            assert (a is None and b is None) or torch.equal(_bits(a), _bits(b))


@pytest.mark.parametrize("dtype", DTYPES, ids=dt_id)
def test_capture(dev, calls, dtype):
    import ctc_amd
    shape = (5, 28, 48, 33)
    tf, tb = _to(_fwd_case(shape, True, True), dev), _to(_bwd_case(shape, True, True), dev)
    ff, fb = _lowp(tf["feat"], dtype), _lowp(tb["feat"], dtype, "view")
    _captured(lambda: _forward(ctc_amd.head_forward, tf, ff))
    _captured(lambda: _backward(ctc_amd.head_backward, tb, fb, True))
    assert all(typed for _, typed in calls) and len(calls) == 6


# ------------------------------------------------------------------------------------------------------------ fallback

@pytest.mark.parametrize("layout", ["odd", "pitch2"])
def test_views_the_typed_entries_refuse_take_the_cast_path(dev, calls, layout):
    """a bf16 view at a 2-byte-odd offset (address = 2 mod 8), or with a row pitch that is no multiple of 4 elements: still
    answered, through the cast and the fp32 entry, with the fp32 result (d_feat in feat's dtype all the same)"""
    import ctc_amd
    shape = (2, 10, 16, 8)
    tf, tb = _to(_fwd_case(shape, True, True), dev), _to(_bwd_case(shape, True, True), dev)
    feat = _lowp(tf["feat"], torch.bfloat16, layout)
    got = _forward(ctc_amd.head_forward, tf, feat)
    assert got is not None and calls == [("ctc_amd_head_forward", False)]
    _assert_bitwise(FWD_NAMES, got, _forward(ctc_amd.head_forward, tf, feat.float()), "fallback forward")
    feat = _lowp(tb["feat"], torch.bfloat16, layout)
    got = _backward(ctc_amd.head_backward, tb, feat, True)
    assert got is not None and calls[-1] == ("ctc_amd_head_backward", False) and got[0].dtype is torch.bfloat16
    want = _rounded(_backward(ctc_amd.head_backward, tb, feat.float(), True), torch.bfloat16)
    _assert_bitwise(BWD_NAMES, got, want, "fallback backward")
    cell_feat, head, cell = _cell_inputs(dev, 3, 5, 32, 8)
    feat = _lowp(cell_feat, torch.bfloat16, layout)
    got = ctc_amd.lstm_forward(feat, *head.values(), *cell.values(), 8)
    assert got is not None and calls[-1] == ("ctc_amd_lstm_forward", False)
    assert torch.equal(got, ctc_amd.lstm_forward(feat.float(), *head.values(), *cell.values(), 8))
