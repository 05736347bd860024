"""A scale_grad call folded into the captured loss launch it scales (include/ctc_amd.h).

Under stream capture, `ctc_amd_scale_grad[_typed]` issued directly behind a `*_loss_grad` launch on the same stream, for
that launch's gradient buffer, adds no node: the loss kernel reads `*grad_out` when it runs.  Every comparison here is
against the EAGER sequence of the same calls on the same inputs (two launches, as before), bit for bit -- the folded
arithmetic is the scale kernel's by construction, so there is no tolerance.  How often a call was folded / refused is
read from `ctc_amd_debug_scale_folds` of the diagnostics build, bound here (not part of include/ctc_amd.h).
"""
import ctypes

import pytest
import torch

from ctc_amd import _lib
from tests.helpers import synth_binary, synth_noblank

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GOS = (1.0, 0.25, 0.3, -2.0, 0.0)
TORCH_DTYPE = {_lib.F32: torch.float32, _lib.BF16: torch.bfloat16, _lib.F16: torch.float16}


@pytest.fixture(scope="module")
def lib():
    from ctc_amd import build
    lb = ctypes.CDLL(build.build_diag())
    for name, (res, args) in _lib.PROTOTYPES.items():
        fn = getattr(lb, name)
        fn.restype, fn.argtypes = res, args
    lb.ctc_amd_debug_scale_folds.restype = ctypes.c_int
    lb.ctc_amd_debug_scale_folds.argtypes = [ctypes.POINTER(ctypes.c_uint)] * 2
    return lb


def folds(lib):
    """(taken, refused) since the library was loaded"""
    t, r = ctypes.c_uint(), ctypes.c_uint()
    assert lib.ctc_amd_debug_scale_folds(ctypes.byref(t), ctypes.byref(r)) == 0
    return t.value, r.value


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def same_bits(got, want):
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b)), "output %d differs" % k


class Case:
    """device-resident inputs and outputs of one loss+gradient call, and the C-ABI calls on them"""

    def __init__(self, lib, variant, T, B, C, S, dtype=_lib.F32, smoothing=-1.0, lab64=False, seed=0, broken=()):
        self.lib, self.variant, self.shape, self.dtype, self.smoothing = lib, variant, (T, B, C, S), dtype, smoothing
        if variant == "noblank":
            x, tg, il, tl = synth_noblank(seed, T, B, C, S, var_T=True, int64=lab64)
            self.vid = _lib.NOBLANK
        else:
            x, tg, il, tl = synth_binary(seed, T, B, C, S, var_T=True)
            self.vid = _lib.BINARY
        for b in broken:                                     # samples without an alignment: more labels than frames
            il[b], tl[b] = 1, min(2, S)
        td = TORCH_DTYPE[dtype]
        self.x, self.tg, self.il, self.tl = x.to(td).to(DEV), tg.to(DEV), il.to(DEV), tl.to(DEV)
        self.nll = torch.empty(B, dtype=torch.float32, device=DEV)
        self.loss = torch.empty(4, dtype=torch.float32, device=DEV)
        self.grad = torch.empty(T, B, C, dtype=td, device=DEV)
        self.other = torch.empty(T, B, C, dtype=td, device=DEV)      # a gradient-sized buffer that is NOT the launch's
        self.go = torch.ones((), dtype=torch.float32, device=DEV)
        self.ws = torch.zeros(lib.ctc_amd_workspace_bytes(self.vid, T, B, C, S), dtype=torch.uint8, device=DEV)
        self.scale = 1.0 / B

    def outputs(self):
        return [self.nll, self.loss, self.grad, self.other]

    def poison(self):
        self.nll.fill_(-7.0)
        self.loss.fill_(-7.0)
        self.grad.fill_(3.0)
        self.other.copy_(self.x)

    def loss_grad(self, stream, slot=0):
        T, B, C, S = self.shape
        x, lib = self.x, self.lib
        common = (self.il.data_ptr(), self.tl.data_ptr(), T, B, C, S)
        tail = (self.scale, self.scale, self.nll.data_ptr(), self.loss.data_ptr() + 4 * slot, self.grad.data_ptr(),
                self.ws.data_ptr(), stream)
        if self.variant == "binary":
            rc = lib.ctc_amd_binary_loss_grad(x.data_ptr(), x.stride(0), x.stride(1), self.tg.data_ptr(), *common, *tail)
        elif self.dtype == _lib.F32 and self.smoothing < 0:  # (the call of bench.py's Workload.step)
            rc = lib.ctc_amd_noblank_loss_grad(x.data_ptr(), x.stride(0), x.stride(1), self.tg.data_ptr(),
                                               int(self.tg.dtype == torch.int64), *common, *tail)
        else:
            rc = lib.ctc_amd_noblank_loss_grad_typed(x.data_ptr(), self.dtype, x.stride(0), x.stride(1), self.tg.data_ptr(),
                                                     int(self.tg.dtype == torch.int64), *common, self.smoothing, *tail)
        assert rc == 0, rc

    def scale_grad(self, stream, buf=None, n=None, dtype=None):
        buf = self.grad if buf is None else buf
        n = buf.numel() if n is None else n
        dtype = self.dtype if dtype is None else dtype
        if dtype == _lib.F32 and self.dtype == _lib.F32:
            rc = self.lib.ctc_amd_scale_grad(buf.data_ptr(), self.go.data_ptr(), n, stream)
        else:
            rc = self.lib.ctc_amd_scale_grad_typed(buf.data_ptr(), dtype, self.go.data_ptr(), n, stream)
        assert rc == 0, rc

    def step(self, stream):
        self.loss_grad(stream)
        self.scale_grad(stream)

    def eager(self, seq=None, go=None):
        """the calls of `seq` issued eagerly -> clones of the outputs"""
        if go is not None:
            self.go.fill_(go)
        self.poison()
        (seq or self.step)(torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return [t.clone() for t in self.outputs()]

    def capture(self, seq=None):
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            (seq or self.step)(torch.cuda.current_stream().cuda_stream)
        return g

    def replay(self, g, go=None):
        if go is not None:
            self.go.fill_(go)                                # (in place: the graph holds the pointer, never the value)
        self.poison()
        g.replay()
        torch.cuda.synchronize()
        return [t.clone() for t in self.outputs()]


def fold_cases():
    """(variant, T, B, C, S, dtype, smoothing, lab64): the kernels that take the pointer -- the no-blank r16 kernel in
    every form, and the streamed binary kernel (fp32 only), which takes all four shapes"""
    out = []
    for shape in ((9, 3, 158, 4), (7, 2, 8, 3), (6, None, 8, 2)):    # flagship instantiation, odd T; small; persistent form
        for dtype in (_lib.F32, _lib.BF16, _lib.F16):
            out.append(("noblank", *shape, dtype, -1.0, False))
        out.append(("noblank", *shape, _lib.F32, 0.9, False))
        out.append(("noblank", *shape, _lib.F32, -1.0, True))
    out.append(("noblank", 9, 3, 158, 4, _lib.BF16, 0.9, True))
    for shape in ((9, 3, 158, 4), (7, 2, 8, 3), (6, None, 8, 2), (7, 2, 7, 3)):
        out.append(("binary", *shape, _lib.F32, -1.0, False))
    return out


def make(lib, variant, T, B, C, S, dtype=_lib.F32, smoothing=-1.0, lab64=False, **kw):
    return Case(lib, variant, T, 2 * cus() + 1 if B is None else B, C, S, dtype, smoothing, lab64, **kw)


@pytest.mark.parametrize("cfg", fold_cases(), ids=lambda c: "-".join(str(v) for v in c))
def test_fold_and_exactness(lib, cfg):
    case = make(lib, *cfg)
    for go in GOS:
        want = case.eager(go=go)
        t0, r0 = folds(lib)
        g = case.capture()
        assert folds(lib) == (t0 + 1, r0), "one fold per captured step"
        same_bits(case.replay(g), want)
    assert folds(lib)[0] >= len(GOS)


@pytest.mark.parametrize("cfg", [("noblank", 9, 3, 158, 4, _lib.F32), ("noblank", 7, 2, 8, 3, _lib.BF16),
                                 ("noblank", 6, None, 8, 2, _lib.F16), ("binary", 9, 3, 158, 4, _lib.F32)], ids=str)
def test_value_is_read_at_run_time(lib, cfg):
    case = make(lib, *cfg)
    want = {go: case.eager(go=go) for go in (1.0, 0.3)}
    case.go.fill_(1.0)
    g = case.capture()
    for go in (1.0, 0.3, 1.0):
        same_bits(case.replay(g, go=go), want[go])


def test_eager_calls_never_fold(lib):
    case = make(lib, "noblank", 9, 3, 158, 4)
    t0, r0 = folds(lib)
    a = case.eager(go=0.3)
    b = case.eager(go=1.0)
    assert folds(lib) == (t0, r0)
    # the scale launch did its work: grad(0.3) = grad(1) * 0.3, rounded once more
    assert torch.equal(bits(a[2]), bits(b[2] * torch.tensor(0.3, dtype=torch.float32, device=DEV)))
    same_bits(a[:2], b[:2])                                  # nll and loss are not scaled


def test_a_node_captured_in_between_keeps_the_scale_kernel(lib):
    case = make(lib, "noblank", 9, 3, 158, 4)
    scratch = torch.zeros(8, device=DEV)

    def seq(stream):
        case.loss_grad(stream)
        scratch.add_(1.0)                                    # a node on the capturing stream between the two calls
        case.scale_grad(stream)

    want = case.eager(seq, go=0.3)
    t0, r0 = folds(lib)
    g = case.capture(seq)
    assert folds(lib) == (t0, r0 + 1)
    same_bits(case.replay(g), want)                          # scaled: the graph holds the scale kernel


@pytest.mark.parametrize("what", ["grad", "n", "dtype"])
def test_mismatches_are_refused(lib, what):
    case = make(lib, "noblank", 9, 3, 158, 4)
    kw = {"grad": dict(buf=case.other), "n": dict(n=case.grad.numel() - 2), "dtype": dict(dtype=_lib.BF16)}[what]

    def seq(stream):
        case.loss_grad(stream)
        case.scale_grad(stream, **kw)

    want = case.eager(seq, go=0.3)
    t0, r0 = folds(lib)
    g = case.capture(seq)
    assert folds(lib) == (t0, r0 + 1)
    same_bits(case.replay(g), want)


def test_a_second_scale_call_scales_once_more(lib):
    case = make(lib, "noblank", 9, 3, 158, 4)

    def seq(stream):
        case.loss_grad(stream)
        case.scale_grad(stream)
        case.scale_grad(stream)

    want = case.eager(seq, go=0.3)
    t0, r0 = folds(lib)
    g = case.capture(seq)
    assert folds(lib) == (t0 + 1, r0 + 1)
    same_bits(case.replay(g), want)


def test_other_kernel_families_stay_right_under_capture(lib):
    case = make(lib, "noblank", 7, 2, 7, 3)                  # C odd: the xr family, which does not take the pointer
    for go in (1.0, 0.3):
        want = case.eager(go=go)
        t0, _ = folds(lib)
        g = case.capture()
        assert folds(lib)[0] == t0
        same_bits(case.replay(g), want)


def test_two_graphs_replayed_alternately(lib):
    """bench.py's pattern: two graphs of several steps each on one shared workspace, replayed in turn"""
    case = make(lib, "noblank", 9, 3, 158, 4)
    m = 3
    want = case.eager(go=0.3)

    def steps(stream):
        for j in range(m):
            case.loss_grad(stream, slot=j)
            case.scale_grad(stream)

    t0, r0 = folds(lib)
    graphs = [case.capture(steps) for _ in range(2)]
    assert folds(lib) == (t0 + 2 * m, r0)
    case.poison()
    for g in (graphs[0], graphs[1], graphs[0], graphs[1]):
        g.replay()
    torch.cuda.synchronize()
    got = [t.clone() for t in case.outputs()]
    same_bits([got[0], got[2]], [want[0], want[2]])
    assert torch.equal(bits(got[1][:m]), bits(want[1][:1].expand(m)))


def test_two_streams_capturing_at_the_same_time(lib):
    a = make(lib, "noblank", 9, 3, 158, 4, seed=1)
    b = make(lib, "noblank", 7, 2, 8, 3, _lib.BF16, seed=2)
    want_a, want_b = a.eager(go=0.3), b.eager(go=-2.0)
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    ga, gb = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    t0, r0 = folds(lib)
    with torch.cuda.stream(sa):
        ga.capture_begin(capture_error_mode="thread_local")
    with torch.cuda.stream(sb):
        gb.capture_begin(capture_error_mode="thread_local")
    a.loss_grad(sa.cuda_stream)
    b.loss_grad(sb.cuda_stream)
    a.scale_grad(sa.cuda_stream)
    b.scale_grad(sb.cuda_stream)
    with torch.cuda.stream(sb):
        gb.capture_end()
    with torch.cuda.stream(sa):
        ga.capture_end()
    assert folds(lib) == (t0 + 2, r0)
    same_bits(a.replay(ga), want_a)
    same_bits(b.replay(gb), want_b)


def test_smoothed_loss_without_alignment_gives_zero_rows(lib):
    case = make(lib, "noblank", 9, 3, 158, 4, _lib.F32, 0.9, broken=(1,))
    case.x[2, 2, 5] = float("-inf")                          # a -inf logit in a live row: no alignment through the row constants
    want = case.eager(go=0.3)
    t0, r0 = folds(lib)
    g = case.capture()
    assert folds(lib) == (t0 + 1, r0)
    got = case.replay(g)
    same_bits(got, want)
    assert bool((got[2][:, 1] == 0).all()) and bool((got[2][:, 2] == 0).all())
    assert bool((got[2][:, 0] != 0).any())
