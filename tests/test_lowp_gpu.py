"""bf16 / fp16 logits in the no-blank loss (include/ctc_amd.h, ctc_amd_noblank_loss_grad_typed).

The contract: x is widened exactly and the arithmetic is the fp32 launch's, so on the same values nll and loss are
BITWISE those of the fp32 path on x.float(), and the gradient is bitwise that path's gradient rounded to x.dtype."""
import numpy as np
import pytest
import torch

from oracle import ctc_numpy
from tests.helpers import np_, synth_noblank

pytestmark = pytest.mark.gpu

NLL_RTOL = 1e-5                                   # test_parity_gpu.NLL_RTOL
DTYPES = [torch.bfloat16, torch.float16]
_IBITS = {torch.bfloat16: torch.int16, torch.float16: torch.int16, torch.float32: torch.int32}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    import ctc_amd  # noqa: F401  (raises if libctc_amd.so is missing)
    return torch.device("cuda:0")


def _bits(t):
    return t.detach().contiguous().view(_IBITS[t.dtype])


def _assert_bitwise(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    eq = _bits(a) == _bits(b)
    assert bool(eq.all()), "%s: %d of %d elements differ" % (what, int((~eq).sum()), eq.numel())


def _loss(x_leaf, view, lab, Tb, L, ls, grad):
    import ctc_amd
    loss, nll = ctc_amd.noblank_ctc_loss(view(x_leaf), lab, Tb, L, label_smoothing=ls)
    if grad:
        loss.backward()
    torch.cuda.synchronize()
    return loss.detach(), nll.detach(), (x_leaf.grad[(slice(None),) + view.cols] if grad else None)


class _Cols:
    """x -> x[:, :B] (a strided view of a wider batch) or x itself"""

    def __init__(self, B=None):
        self.cols = (slice(0, B),) if B is not None else (slice(None),)

    def __call__(self, x):
        return x[(slice(None),) + self.cols]


# (T, B, C, S, extra): config 2, the persistent form, every r16 row chunking, the domain edges
SHAPES = {
    "config2": (150, 256, 158, 20, {}),
    "persistent": (150, 2048, 158, 20, {}),
    "C2": (150, 64, 2, 20, {}),
    "C62": (150, 64, 62, 20, {}),
    "C94": (150, 64, 94, 20, {}),
    "C256": (150, 64, 256, 20, {}),
    "S31": (120, 64, 158, 31, {}),                                  # (at T = 150 the lattice exceeds the LDS: raises)
    "T168": (168, 64, 158, 20, {}),
    "strided": (150, 96, 158, 20, {"wide": 160}),
    "forward_only": (150, 256, 158, 20, {"grad": False}),
    "smoothed": (150, 128, 158, 20, {"ls": 0.9}),
    # 2-byte logits + gradient beyond the memory-side cache: the non-temporal gradient stores of both forms
    "nt_one_sample": (150, 1600, 256, 20, {}),
    "nt_persistent": (150, 2200, 192, 20, {}),
}


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
@pytest.mark.parametrize("case", sorted(SHAPES))
def test_lowp_bitwise_against_fp32_path(dev, dtype, case):
    T, B, C, S, extra = SHAPES[case]
    grad, ls, wide = extra.get("grad", True), extra.get("ls"), extra.get("wide")
    x, lab, Tb, L = synth_noblank(30 + sorted(SHAPES).index(case), T, wide or B, C, S, var_T=True)
    lab, Tb, L = lab[:B].to(dev), Tb[:B].to(dev), L[:B].to(dev)
    view = _Cols(B if wide else None)
    xl = x.to(dev, dtype).requires_grad_(grad)                       # the 2-byte logits
    xf = xl.detach().float().requires_grad_(grad)                    # the same values in fp32
    loss, nll, g = _loss(xl, view, lab, Tb, L, ls, grad)
    loss32, nll32, g32 = _loss(xf, view, lab, Tb, L, ls, grad)
    assert loss.dtype == nll.dtype == torch.float32
    _assert_bitwise(nll, nll32, "nll")
    _assert_bitwise(loss, loss32, "loss")
    if not grad:
        assert xl.grad is None
        return
    assert g.dtype == dtype
    _assert_bitwise(g, g32.to(dtype), "grad")
    dead = torch.arange(T, device=dev)[:, None] >= Tb[None, :]       # rows t >= T_b: exactly 0
    assert bool((_bits(g)[dead] == 0).all())
    if wide:                                                          # columns outside the view: untouched
        assert bool((xl.grad[:, B:] == 0).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
def test_lowp_against_float64(dev, dtype):
    import ctc_amd
    x, lab, Tb, L = synth_noblank(21, 60, 32, 62, 12, var_T=True)
    xl = x.to(dev, dtype).requires_grad_(True)
    loss, nll = ctc_amd.noblank_ctc_loss(xl, lab.to(dev), Tb.to(dev), L.to(dev))
    loss.backward()
    torch.cuda.synchronize()
    ref = ctc_numpy.noblank_ctc(np_(xl.detach().double()), np_(lab), np_(Tb), np_(L), np.float64)
    scale = np.maximum(1.0, np.abs(ref["nll"]))
    assert (np.abs(np_(nll) - ref["nll"]) <= NLL_RTOL * scale).all()
    # half an ulp of the 2-byte type at the value (<= |v| 2^-(mantissa bits + 1)), plus the fp32 path's own error
    half_ulp = 2.0 ** -(8 if dtype is torch.bfloat16 else 11)
    err = np.abs(np_(xl.grad.double()) - ref["grad"])
    assert (err <= half_ulp * np.abs(ref["grad"]) + 2e-6).all(), err.max()


def test_autocast_linear_step(dev):
    """nn.Linear under autocast(bf16) -> NoBlankCTC -> backward: the logits' gradient is bf16, and the Linear's
    parameter gradients are bitwise those of the same step through logits.float()"""
    import ctc_amd
    T, B, H, C, S = 50, 64, 96, 158, 12
    torch.manual_seed(3)
    lin = torch.nn.Linear(H, C).to(dev)
    feat = torch.randn(T, B, H, device=dev)
    _, lab, Tb, L = synth_noblank(4, T, B, C, S, var_T=True)
    lab, Tb, L = lab.to(dev), Tb.to(dev), L.to(dev)

    def step(cast):
        lin.zero_grad(set_to_none=True)
        with torch.autocast("cuda", torch.bfloat16):
            logits = lin(feat)
            logits.retain_grad()
            loss = ctc_amd.NoBlankCTC()(logits.float() if cast else logits, lab, Tb, L)
        loss.backward()
        torch.cuda.synchronize()
        return logits, loss.detach(), lin.weight.grad.clone(), lin.bias.grad.clone()

    logits, loss, gw, gb = step(False)
    assert logits.dtype == torch.bfloat16 and logits.grad.dtype == torch.bfloat16
    assert loss.dtype == torch.float32
    logits_c, loss_c, gw_c, gb_c = step(True)
    _assert_bitwise(loss, loss_c, "loss")
    _assert_bitwise(logits.grad, logits_c.grad, "logits.grad")
    _assert_bitwise(gw, gw_c, "weight.grad")
    _assert_bitwise(gb, gb_c, "bias.grad")


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16"])
def test_lowp_scaled_and_retained_backward(dev, dtype):
    import ctc_amd
    x, lab, Tb, L = synth_noblank(8, 80, 48, 94, 10, var_T=True)
    lab, Tb, L = lab.to(dev), Tb.to(dev), L.to(dev)
    xl = x.to(dev, dtype).requires_grad_(True)
    ctc_amd.NoBlankCTC()(xl, lab, Tb, L).backward()
    g1 = xl.grad.clone()
    xl.grad = None
    (3 * ctc_amd.NoBlankCTC()(xl, lab, Tb, L)).backward()            # the typed scale kernel
    _assert_bitwise(xl.grad, (g1.float() * 3).to(dtype), "3 * loss")
    xl.grad = None
    loss = ctc_amd.NoBlankCTC()(xl, lab, Tb, L)
    loss.backward(retain_graph=True)
    ga = xl.grad.clone()
    xl.grad = None
    loss.backward()                                                   # recomputed by a second launch
    _assert_bitwise(xl.grad, ga, "retain_graph")
    _assert_bitwise(ga, g1, "first backward")


@pytest.mark.parametrize("B", [8, 600])
def test_lowp_graph_capture(dev, B):
    """forward + backward on bf16 logits captured into a hipGraph, replayed twice on new data: bitwise the eager
    result (B = 600: the persistent form)"""
    import ctc_amd
    x, lab, Tb, L = synth_noblank(5, 30, B, 20, 6, var_T=True)
    xs = x.to(dev, torch.bfloat16).requires_grad_(True)
    labd, Tbd, Ld = lab.to(dev), Tb.to(dev), L.to(dev)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                     # warm-up on the capture stream (workspace, grads)
        for _ in range(2):
            xs.grad = None
            loss = ctc_amd.CTCLoss.apply(xs, labd, Tbd, Ld)
            loss.backward()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    xs.grad = None
    with torch.cuda.graph(g):
        loss = ctc_amd.CTCLoss.apply(xs, labd, Tbd, Ld)
        loss.backward()
    for seed in (6, 7):
        x2, _, _, _ = synth_noblank(seed, 30, B, 20, 6)
        with torch.no_grad():
            xs.copy_(x2.to(dev, torch.bfloat16))
        g.replay()
        torch.cuda.synchronize()
        got_loss, got_grad = loss.detach().clone(), xs.grad.clone()
        xe = xs.detach().clone().requires_grad_(True)
        le = ctc_amd.CTCLoss.apply(xe, labd, Tbd, Ld)
        le.backward()
        torch.cuda.synchronize()
        _assert_bitwise(got_loss, le.detach(), "replayed loss")
        _assert_bitwise(got_grad, xe.grad, "replayed grad")


def test_lowp_outside_domain_raises(dev):
    import ctc_amd
    x, lab, Tb, L = synth_noblank(1, 20, 2, 11, 4)            # odd C
    with pytest.raises(ctc_amd.CtcAmdError, match="float"):
        ctc_amd.NoBlankCTC()(x.to(dev, torch.bfloat16), lab.to(dev), Tb.to(dev), L.to(dev))
    x, lab, Tb, L = synth_noblank(1, 60, 2, 12, 40)           # S = 40 > 31
    with pytest.raises(ctc_amd.CtcAmdError):
        ctc_amd.NoBlankCTC()(x.to(dev, torch.bfloat16), lab.to(dev), Tb.to(dev), L.to(dev))
    x, lab, Tb, L = synth_noblank(1, 150, 2, 158, 31)         # S = 31 at T = 150: the r16 lattice exceeds the LDS
    with pytest.raises(ctc_amd.CtcAmdError):
        ctc_amd.NoBlankCTC()(x.to(dev, torch.float16), lab.to(dev), Tb.to(dev), L.to(dev))
    xb = torch.randn(20, 2, 12, device=dev, dtype=torch.bfloat16)
    with pytest.raises(ValueError):
        ctc_amd.binary_ctc_loss(xb, torch.zeros(2, 3, 12, device=dev), torch.tensor([20, 20]), torch.tensor([3, 2]))
    with pytest.raises(ValueError):
        ctc_amd.blank_ctc_loss(xb.float().log_softmax(2).bfloat16(), torch.ones(2, 3, dtype=torch.long, device=dev),
                               torch.tensor([20, 20]), torch.tensor([3, 2]))
