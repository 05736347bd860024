"""The producer of the logits: drop-in for the reference's ``LSTM_cell`` (LSTM.py:21-51).

``LSTM_cell(args).forward(feat, v_hsn, v_csn)`` runs, per frame, ``v = self.v(feat[time])`` (Linear + BatchNorm1d +
ReLU + Dropout) and one ``nn.LSTMCell`` step whose hidden state is stored as ``v_series[time]`` -- the ``[T, B, C]``
tensor the CTC losses read.  Here the head of ALL frames is one HIP launch (``ctc_amd_head_forward``: the 1024 -> C
product on the matrix cores, BatchNorm with the statistics of each frame's batch in train mode / the running statistics
in eval mode, ReLU, and the dropout mask torch drew), and the LSTMCell steps and stores are one more
(``ctc_amd_lstm_series`` at the reference's class counts, I + H <= 80; ``ctc_amd_lstm_series_wide`` / ``lstm_series_wide`` up to
160 classes, the benchmark's 158 among them: the weights no longer fit a workgroup's registers and are streamed from L2, from a
transposed copy, the x part of every row computed ahead of the recurrence -- bit for bit the frame-by-frame result, taken for
T B <= ``SERIES_WIDE_MAX_ROWS`` rows (measured, profiles/r16_lstm_wide.md: forward + backward 5.4 ms against 57.2 ms at T = 150,
B = 256, C = 158); one launch per frame, ``ctc_amd_lstm_cell_step``, beyond that gate and beyond 160): gate products, cell update, and the hidden state
written straight into the logits tensor, optionally with one pad column (``pad_classes=True``: an odd class count such
as the reference's 33 gets rows of C + 1 floats, the extra logit -1e30 -- softmax gives it exactly 0, so no loss or
gradient value changes, and the rows become the even, 8-byte aligned rows of the fastest loss kernel).

In eval mode with nothing that needs a gradient (the reference validates under ``eval()`` and ``no_grad``) the two launches
are ONE (``ctc_amd_lstm_forward`` / ``lstm_forward``): a workgroup computes the head rows of its own four samples into LDS and
walks the recurrence from there, so ``v_all [T,B,C]`` never goes to memory; the result is bit-identical to the two launches.
``LSTM_cell.forward`` takes it up to ``FUSED_FORWARD_MAX_WG_ROWS`` head rows per workgroup (4 T <= 64: measured,
profiles/r13_lstm_forward.md -- 50 us against 70 us per forward at the reference's sizes; at T = 150 the two launches win).

Same attribute names as the reference (``v``, ``v.layers``, ``v_cell``): its checkpoints load unchanged.  The backward
pass: the recurrence's is HIP whole (``ctc_amd_lstm_backward`` / ``lstm_backward``: the recurrence launch, then d_x, both weight
gradients and the bias gradients as one products launch on the matrix cores, h_{t-1} read in place from v_series -- two launches,
three when the sums split their rows) for T B <= ``SERIES_BACKWARD_MAX_ROWS`` rows (measured, profiles/r15_lstm_backward.md);
beyond that gate it is the recurrence launch (``ctc_amd_lstm_series_backward``) plus torch arithmetic on its result
(``_series_backward_torch``: three rocBLAS GEMMs and a column sum); behind the wide forward it is the wide recurrence launch
(``ctc_amd_lstm_series_backward_wide`` / ``lstm_series_backward_wide``), the bias gradients as a HIP launch of their own
(``ctc_amd_lstm_bias_grad_wide`` / ``lstm_bias_grad_wide``: torch's column sum replayed wrong from a captured graph behind this
launch at T B = 1500, profiles/r16_lstm_wide.md) and the three GEMMs of the same torch arithmetic, and behind the
frame-by-frame forward a BPTT loop of torch kernels;
the head's backward is HIP as well (``ctc_amd_head_backward`` / ``head_backward``: the BatchNorm / ReLU / Dropout row pass,
then both products, the column sums and the sums over the frames on the matrix cores -- two launches, three when the weight
gradient splits its rows) for T B <= ``HEAD_BACKWARD_MAX_ROWS`` rows (measured, profiles/r14_head_backward.md).  Beyond that
gate, and for the shapes the entry does not take (B > 256, K not a multiple of 16, unaligned rows), the head's backward is
torch arithmetic (``_head_backward_torch``: elementwise kernels and two rocBLAS GEMMs).  Batches beyond 256 samples stay on the
HIP path as well (``ctc_amd_head_forward_wide`` / ``head_forward_wide``: a frame's rows no longer fit one workgroup, so BatchNorm's
batch statistics cross workgroups at a kernel boundary -- one launch in eval mode, two in train mode, the Linear output and all of
eval mode bit for bit the narrow launch's; ``ctc_amd_head_backward_wide`` / ``head_backward_wide``: the row pass walks the frame's
blocks of 256 rows, the products are the narrow entry's) for T B <= ``HEAD_WIDE_MAX_ROWS`` and T B <=
``HEAD_WIDE_BACKWARD_MAX_ROWS`` rows (measured, profiles/r18_head_wide.md: 0.70 ms against 6.41 ms for the train-mode head at
T = 150, B = 2048, C = 33); beyond the first gate torch's layers run frame by frame, beyond the second ``_head_backward_torch``.
A bf16 / fp16 ``feat`` (a backbone under ``torch.autocast``) is read natively by all five head entry points (the ``*_typed``
entries, ``_feat_call``): no ``.float()``, no fp32 copy, every output fp32 and bit for bit that of ``feat.float()``, ``d_feat`` in
``feat``'s dtype; no gate of its own (measured, profiles/r19_head_typed.md: below the cast path's minimum at every point).
No CPU path: non-HIP tensors raise.
"""
import torch
import torch.nn as nn

from . import _lib
from . import functional as F

PAD_LOGIT = -1.0e30


class BasicModule(nn.Module):
    """feature head of one frame: Linear -> BatchNorm1d -> ReLU -> Dropout (LSTM.py:7-18), torch's own layers"""

    def __init__(self, inDim, outDim, dp_rate=0.3):
        super().__init__()
        self.layers = nn.Sequential(nn.Linear(inDim, outDim), nn.BatchNorm1d(outDim), nn.ReLU(), nn.Dropout(p=dp_rate))

    def forward(self, x):
        return self.layers(x)


_LOWP_FEAT = {torch.bfloat16: _lib.BF16, torch.float16: _lib.F16}


def _f32c(t):
    """``t`` itself when it is fp32 and contiguous, else cast and copied"""
    return t if (t.dtype is torch.float32 and t.is_contiguous()) else t.float().contiguous()


def _rows(t, pitch=False):
    """``t`` [T,B,n] itself when the entry can address its rows -- fp32, unit stride over the last dimension and, with ``pitch``,
    a row pitch of at least the width -- else cast and copied"""
    ok = t.dtype is torch.float32 and t.stride(2) == 1 and (not pitch or t.stride(1) >= t.shape[2])
    return t if ok else t.float().contiguous()


def _ptr(t):
    return None if t is None else t.data_ptr()


def _answer(rc, name, refusal_is_none=True):
    """what an entry's return code means to the caller: True, False for UNSUPPORTED_SHAPE (the public functions return None
    then), ``CtcAmdError`` for everything else"""
    if rc == _lib.ERR_UNSUPPORTED_SHAPE and refusal_is_none:
        return False
    if rc:
        _lib.check(rc, name)
    return True


def _scratch(query, dev, *shape):
    """the scratch of one call, (buffer, bytes) as ``query`` sizes it, or None when the entry does not take the shape (the
    query answers 0 for positive sizes).  One ``torch.empty`` per call: ``head_backward`` says why."""
    nbytes = getattr(_lib.load(), query)(*shape)
    if nbytes == 0 and min(shape) >= 1:
        return None
    return torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev), nbytes


def _feat_call(name, feat, pre, post):
    """One head entry on ``feat`` [T,B,K] -> (return code, whether the typed entry ran).  ``pre`` / ``post``: the arguments in
    front of and behind (feat, its strides); ``post`` is a function of that flag (the backward entries write d_feat in feat's
    element type).  An fp32 ``feat`` goes to the entry ``name`` as before.  A bf16 / fp16 ``feat`` with unit last stride -- what a
    backbone under ``torch.autocast`` hands over -- goes to ``name + "_typed"`` as it lies: no ``.float()``, no copy (DESIGN
    3.6c).  When that entry answers UNSUPPORTED_SHAPE (a view that is not 8-byte aligned, a stride that is not a multiple of 4
    elements; also what the fp32 entry refuses, which the second answer then repeats), and for every other dtype or layout, the
    cast and the fp32 entry."""
    lib = _lib.load()
    code = _LOWP_FEAT.get(feat.dtype)
    if code is not None and feat.stride(2) == 1:
        rc = getattr(lib, name + "_typed")(*pre, feat.data_ptr(), code, feat.stride(0), feat.stride(1), *post(True))
        if rc != _lib.ERR_UNSUPPORTED_SHAPE:
            return rc, True
    f = _rows(feat)
    return getattr(lib, name)(*pre, f.data_ptr(), f.stride(0), f.stride(1), *post(False)), False


def _dfeat_as(d_feat, feat):
    """d_feat in the element type of a bf16 / fp16 ``feat`` (the typed entry wrote it so; behind the cast path the fp32 result is
    rounded here, once, as autograd would round it at the module level)"""
    if d_feat is None or feat.dtype not in _LOWP_FEAT or d_feat.dtype is feat.dtype:
        return d_feat
    return d_feat.to(feat.dtype)


def _head_forward(name, query, feat, weight, bias, bn_weight, bn_bias, running_mean, running_var, eps, mask, want_backward_state):
    """``head_forward`` (``query`` None) and ``head_forward_wide`` (``query``: the entry's scratch query): the entry ``name``"""
    F._require_hip(feat, "feat")
    T, B, K = feat.shape
    C = weight.shape[0]
    dev = feat.device
    prm = [_f32c(t) for t in (weight, bias, bn_weight, bn_bias)]
    rm = rv = None
    if running_mean is not None:
        rm, rv = _f32c(running_mean), _f32c(running_var)
    mk = None if mask is None else _f32c(mask)
    tail = ()                                                # (scratch, scratch_bytes) of the wide entry
    if query is not None:
        scratch = _scratch(query, dev, T, B, K, C)
        if scratch is None:
            return None
        tail = (scratch[0].data_ptr(), scratch[1])
    f32 = torch.float32
    out = torch.empty((T, B, C), dtype=f32, device=dev)
    train = rm is None
    lin = torch.empty((T, B, C), dtype=f32, device=dev) if want_backward_state else None
    mean = torch.empty((T, C), dtype=f32, device=dev) if train else None
    var = torch.empty((T, C), dtype=f32, device=dev) if train else None
    inv = torch.empty((T, C), dtype=f32, device=dev) if train else None
    with F._on_device(dev):
        rc, _ = _feat_call(name, feat, (), lambda typed: (
            *(t.data_ptr() for t in prm), _ptr(rm), _ptr(rv), float(eps), _ptr(mk), T, B, K, C, out.data_ptr(), out.stride(0),
            out.stride(1), _ptr(lin), _ptr(mean), _ptr(var), _ptr(inv), *tail, F._stream_handle(dev)))
    return (out, lin, mean, var, inv) if _answer(rc, name) else None


def _head_backward(name, d_out, feat, weight, bn_weight, bn_bias, lin, mean, invstd, running_mean, running_var, eps, mask,
                   need_dfeat):
    """``head_backward`` and ``head_backward_wide``: the entry ``name`` behind its scratch query"""
    F._require_hip(d_out, "d_out")
    F._require_hip(feat, "feat")
    T, B, K = feat.shape
    C = weight.shape[0]
    dev = feat.device
    f32 = torch.float32
    do = _rows(d_out)
    w, g, be, ln, mn, iv, rm, rv, mk = (None if t is None else _f32c(t) for t in (weight, bn_weight, bn_bias, lin, mean, invstd,
                                                                                  running_mean, running_var, mask))
    scratch = _scratch(name + "_scratch_bytes", dev, T, B, K, C)
    if scratch is None:
        return None
    d_weight = torch.empty((C, K), dtype=f32, device=dev)
    d_bias, d_gamma, d_beta = (torch.empty(C, dtype=f32, device=dev) for _ in range(3))
    d_feat = [None]

    def behind_feat(typed):                                  # d_feat: feat's element type from the typed entry, fp32 from the other
        if need_dfeat:
            d_feat[0] = torch.empty((T, B, K), dtype=feat.dtype if typed else f32, device=dev)
        return (w.data_ptr(), g.data_ptr(), be.data_ptr(), ln.data_ptr(), _ptr(mn), _ptr(iv), _ptr(rm), _ptr(rv), float(eps),
                _ptr(mk), T, B, K, C, _ptr(d_feat[0]), B * K if need_dfeat else 0, K if need_dfeat else 0, d_weight.data_ptr(),
                d_bias.data_ptr(), d_gamma.data_ptr(), d_beta.data_ptr(), scratch[0].data_ptr(), scratch[1], F._stream_handle(dev))
    with F._on_device(dev):
        rc, _ = _feat_call(name, feat, (do.data_ptr(), do.stride(0), do.stride(1)), behind_feat)
    return (_dfeat_as(d_feat[0], feat), d_weight, d_bias, d_gamma, d_beta) if _answer(rc, name) else None


def head_forward(feat, weight, bias, bn_weight, bn_bias, running_mean=None, running_var=None, eps=1e-5, mask=None,
                 want_backward_state=False):
    """``dropout(relu(batchnorm(feat[t] @ weight.T + bias)))`` for every frame t in ONE launch (``ctc_amd_head_forward``)
    -> (out [T,B,C], lin [T,B,C] | None, mean [T,C] | None, var [T,C] | None, invstd [T,C] | None), or None when the launch
    does not take the shape (B > 256, K not a multiple of 16, unaligned rows).  running_mean / running_var: eval mode;
    both None: the statistics of each frame's batch.  ``mask``: [T,B,C], already scaled by 1 / (1 - p).  A bf16 / fp16 ``feat``
    is read as it lies (``ctc_amd_head_forward_typed``, see ``_feat_call``): every result is fp32 and bit for bit that of
    ``feat.float()``."""
    return _head_forward("ctc_amd_head_forward", None, feat, weight, bias, bn_weight, bn_bias, running_mean, running_var, eps,
                         mask, want_backward_state)


def head_backward(d_out, feat, weight, bn_weight, bn_bias, lin, mean=None, invstd=None, running_mean=None, running_var=None,
                  eps=1e-5, mask=None, need_dfeat=True):
    """The backward of ``head_forward`` on the HIP path (``ctc_amd_head_backward``: two launches, three when T B > 128) ->
    (d_feat [T,B,K] | None, d_weight [C,K], d_bias [C], d_bn_weight [C], d_bn_bias [C]), or None when the entry does not take
    the shape (what ``head_forward`` refuses, or T B > 2^22 rows).  ``lin``: the forward's Linear output [T,B,C];
    train mode: ``mean`` / ``invstd`` [T,C] as the forward saved them; eval mode: ``running_mean`` / ``running_var`` [C] and
    ``eps``; ``mask`` as the forward took it.  Deterministic (no atomics, fixed sum orders).

    A bf16 / fp16 ``feat`` is read as it lies (``ctc_amd_head_backward_typed``, see ``_feat_call``) and ``d_feat`` comes back in
    ``feat``'s dtype: the fp32 value rounded once to nearest even, which is what autograd makes of an fp32 gradient at the module
    level anyway.  The four parameter gradients stay fp32, bit for bit those of ``feat.float()``.

    The scratch (dlin [T B, C padded to 16], the per-frame partial sums, the partial weight gradients) is one ``torch.empty``
    per call, not a cached buffer: torch's caching allocator hands the same block back without a device call once the shape has
    been seen, the stream ordering of the block is torch's own business that way, and under ``torch.cuda.graph`` capture the
    block comes from the graph's private pool, which a buffer cached outside the capture could not promise."""
    return _head_backward("ctc_amd_head_backward", d_out, feat, weight, bn_weight, bn_bias, lin, mean, invstd, running_mean,
                          running_var, eps, mask, need_dfeat)


def head_forward_wide(feat, weight, bias, bn_weight, bn_bias, running_mean=None, running_var=None, eps=1e-5, mask=None,
                      want_backward_state=False):
    """``head_forward`` for batches beyond 256 samples (``ctc_amd_head_forward_wide``: B up to 65536, the B <= 256 of the narrow
    entry too; one launch in eval mode, two in train mode -- a frame's rows no longer fit one workgroup, so BatchNorm's batch
    statistics cross workgroups at a kernel boundary): the same arguments, the same return value, or None when the entry does
    not take the shape (K not a multiple of 16, unaligned rows, T B > 2^22 rows, B > 65536).  The Linear output and all of eval
    mode are bit for bit the narrow entry's.  A bf16 / fp16 ``feat`` is read as it lies (``ctc_amd_head_forward_wide_typed``), as in
    ``head_forward``.  The scratch is one ``torch.empty`` per call, as ``head_backward`` explains."""
    return _head_forward("ctc_amd_head_forward_wide", "ctc_amd_head_forward_wide_scratch_bytes", feat, weight, bias, bn_weight,
                         bn_bias, running_mean, running_var, eps, mask, want_backward_state)


def head_backward_wide(d_out, feat, weight, bn_weight, bn_bias, lin, mean=None, invstd=None, running_mean=None, running_var=None,
                       eps=1e-5, mask=None, need_dfeat=True):
    """``head_backward`` for batches beyond 256 samples (``ctc_amd_head_backward_wide``: B up to 65536; the row pass walks a
    frame's blocks of 256 rows, the products and the reduce launch are the narrow entry's -- two launches, three when
    T B > 128): the same arguments, the same return value, or None when the entry does not take the shape (what
    ``head_forward_wide`` refuses).  Deterministic.  A bf16 / fp16 ``feat`` is read as it lies (``ctc_amd_head_backward_wide_typed``)
    and ``d_feat`` comes back in ``feat``'s dtype, as in ``head_backward``.  The scratch is one ``torch.empty`` per call, as
    ``head_backward`` explains."""
    return _head_backward("ctc_amd_head_backward_wide", d_out, feat, weight, bn_weight, bn_bias, lin, mean, invstd, running_mean,
                          running_var, eps, mask, need_dfeat)


def _head_backward_torch(d_out, feat, weight, gamma, beta, lin, mean, inv, mask, train, need_dfeat):
    """the head's backward as torch arithmetic (BatchNorm's own formulas on the saved Linear output and statistics, two
    GEMMs over all frames at once): what runs outside the gate.  mean / inv: [T,C] (train) or [1,C] (eval)."""
    T, B, C = lin.shape
    xhat = (lin - mean.unsqueeze(1)) * inv.unsqueeze(1)
    dy = d_out.float()
    if mask is not None:
        dy = dy * mask
    dy = dy * ((xhat * gamma + beta) > 0)
    dbeta = dy.sum((0, 1))
    dgamma = (dy * xhat).sum((0, 1))
    dxh = dy * gamma
    if train:                                            # BatchNorm over the B rows of each frame
        dlin = inv.unsqueeze(1) * (dxh - dxh.mean(1, keepdim=True) - xhat * (dxh * xhat).mean(1, keepdim=True))
    else:
        dlin = dxh * inv.unsqueeze(1)
    flat = dlin.reshape(T * B, C)
    dW = flat.t() @ feat.reshape(T * B, -1).float()
    dfeat = (flat @ weight.float()).reshape(feat.shape) if need_dfeat else None
    return dfeat, dW, flat.sum(0), dgamma, dbeta


class _HeadFn(torch.autograd.Function):
    """feat [T,B,K], Linear and BatchNorm parameters, running statistics (eval) or None (train), mask -> the head's output
    [T,B,C] (+ the batch statistics, non-differentiable).  Forward: one HIP launch.  Backward: ``head_backward`` (HIP) for
    T B <= ``HEAD_BACKWARD_MAX_ROWS`` rows; ``_head_backward_torch`` beyond the gate and for shapes the entry does not take.
    B > 256 (``ctx.wide``): ``head_forward_wide`` (one launch in eval mode, two in train mode) and, for T B <=
    ``HEAD_WIDE_BACKWARD_MAX_ROWS`` rows, ``head_backward_wide``; the caller (``LSTM_cell._head``) holds the forward's gate."""

    @staticmethod
    def forward(ctx, feat, weight, bias, bn_weight, bn_bias, running_mean, running_var, eps, mask):
        need = any(ctx.needs_input_grad[:5])
        ctx.wide = feat.shape[1] > 256
        fwd = head_forward_wide if ctx.wide else head_forward
        res = fwd(feat, weight, bias, bn_weight, bn_bias, running_mean, running_var, eps, mask, want_backward_state=need)
        if res is None:
            raise _lib.CtcAmdError("ctc_amd: the fused head does not take this shape (feature dimension a multiple of 16, "
                                   "16-byte aligned rows, T B <= 2^22)" if ctx.wide else
                                   "ctc_amd: the fused head does not take this shape (B <= 256, feature dimension a multiple of 16)")
        out, lin, mean, var, inv = res
        ctx.train = running_mean is None
        ctx.eps = float(eps)
        if need:
            if not ctx.train:
                mean, inv = running_mean.float().unsqueeze(0), torch.rsqrt(running_var.float() + float(eps)).unsqueeze(0)
            ctx.save_for_backward(feat, weight, bn_weight, bn_bias, lin, mean, inv, mask, running_mean, running_var)
        stats = (mean, var) if ctx.train else (None, None)
        if ctx.train:
            ctx.mark_non_differentiable(mean, var)
        return (out,) + stats

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_out, _dm=None, _dv=None):
        feat, weight, gamma, beta, lin, mean, inv, mask, rmean, rvar = ctx.saved_tensors
        T, B, _ = lin.shape
        need_dfeat = ctx.needs_input_grad[0]
        bwd, gate = (head_backward_wide, HEAD_WIDE_BACKWARD_MAX_ROWS) if ctx.wide else (head_backward, HEAD_BACKWARD_MAX_ROWS)
        res = None
        if T * B <= gate:
            stats = (mean, inv, None, None) if ctx.train else (None, None, rmean, rvar)
            res = bwd(d_out, feat, weight, gamma, beta, lin, *stats, ctx.eps, mask, need_dfeat)
        if res is None:
            res = _head_backward_torch(d_out, feat, weight, gamma, beta, lin, mean, inv, mask, ctx.train, need_dfeat)
        return tuple(res) + (None, None, None, None)


def lstm_cell_step(x, h, c, w_ih, w_hh, b_ih, b_hh, series_row=None, pad_value=PAD_LOGIT, want_gates=False):
    """One fused LSTMCell step on the device -> (h', c', gates | None).  ``series_row``: a [B, cols >= H] view with unit
    stride over its last dimension (e.g. ``v_series[time]``) that receives h' in columns [0, H) and ``pad_value`` behind."""
    F._require_hip(x, "x")
    B, I = x.shape
    H = h.shape[1]
    dev = x.device
    args = [_f32c(t) for t in (x, h, c, w_ih, w_hh, b_ih, b_hh)]
    h_out = torch.empty((B, H), dtype=torch.float32, device=dev)
    c_out = torch.empty((B, H), dtype=torch.float32, device=dev)
    gates = torch.empty((B, 4 * H), dtype=torch.float32, device=dev) if want_gates else None
    sp, ss, sc = None, 0, 0
    if series_row is not None:
        if series_row.dim() != 2 or series_row.shape[0] != B or series_row.shape[1] < H or series_row.stride(1) != 1 \
                or series_row.dtype is not torch.float32 or series_row.device != dev:
            raise ValueError("ctc_amd: series_row must be a float32 [B, >= H] view with unit stride over the classes")
        sp, ss, sc = series_row.data_ptr(), series_row.stride(0), series_row.shape[1]
    with F._on_device(dev):
        rc = _lib.load().ctc_amd_lstm_cell_step(*(t.data_ptr() for t in args), B, I, H, h_out.data_ptr(), c_out.data_ptr(),
                                                _ptr(gates), sp, ss, sc, float(pad_value), F._stream_handle(dev))
    _answer(rc, "ctc_amd_lstm_cell_step", refusal_is_none=False)
    return h_out, c_out, gates


def _series_forward(name, query, v_all, h0, c0, w_ih, w_hh, b_ih, b_hh, cols, pad_value, want_backward_state):
    """``lstm_series`` (``query`` None) and ``lstm_series_wide`` (``query``: the entry's scratch query): the entry ``name``"""
    F._require_hip(v_all, "v_all")
    T, B, I = v_all.shape
    H = h0.shape[1]
    cols = H if cols is None else int(cols)
    dev = v_all.device
    args = [_f32c(t) for t in (v_all, h0, c0, w_ih, w_hh, b_ih, b_hh)]
    tail = ()                                                # (scratch, scratch_bytes) of the wide entry
    if query is not None:
        scratch = _scratch(query, dev, T, B, I, H)
        if scratch is None:
            return None
        tail = (scratch[0].data_ptr(), scratch[1])
    f32 = torch.float32
    series = torch.empty((T, B, cols), dtype=f32, device=dev)
    gates = torch.empty((T, B, 4 * H), dtype=f32, device=dev) if want_backward_state else None
    cells = torch.empty((T + 1, B, H), dtype=f32, device=dev) if want_backward_state else None
    with F._on_device(dev):
        rc = getattr(_lib.load(), name)(*(t.data_ptr() for t in args), T, B, I, H, series.data_ptr(), series.stride(0),
                                        series.stride(1), cols, float(pad_value), _ptr(gates), _ptr(cells), None, None, *tail,
                                        F._stream_handle(dev))
    return (series, gates, cells) if _answer(rc, name) else None


def _series_backward(name, refusal_is_none, d_series, gates, cells, w_hh):
    """``lstm_series_backward`` (a shape the entry refuses raises: its forward refused it first) and
    ``lstm_series_backward_wide`` (None): the entry ``name``"""
    F._require_hip(d_series, "d_series")
    T, B, G = gates.shape
    H = G // 4
    dev = gates.device
    f32 = torch.float32
    ds = _rows(d_series)
    g, c, w = (_f32c(t) for t in (gates, cells, w_hh))
    dpre = torch.empty((T, B, G), dtype=f32, device=dev)
    dh0 = torch.empty((B, H), dtype=f32, device=dev)
    dc0 = torch.empty((B, H), dtype=f32, device=dev)
    with F._on_device(dev):
        rc = getattr(_lib.load(), name)(ds.data_ptr(), ds.stride(0), ds.stride(1), g.data_ptr(), c.data_ptr(), w.data_ptr(), T, B, H,
                                        dpre.data_ptr(), dh0.data_ptr(), dc0.data_ptr(), F._stream_handle(dev))
    return (dpre, dh0, dc0) if _answer(rc, name, refusal_is_none) else None


def lstm_series(v_all, h0, c0, w_ih, w_hh, b_ih, b_hh, cols=None, pad_value=PAD_LOGIT, want_backward_state=False):
    """All T LSTMCell steps in ONE launch (``ctc_amd_lstm_series``; the reference's class counts, I + H <= 80) ->
    (v_series [T,B,cols], gates [T,B,4H] | None, cells [T+1,B,H] | None), or None when the size is not one the launch
    takes (step frame by frame with ``lstm_cell_step`` then)."""
    return _series_forward("ctc_amd_lstm_series", None, v_all, h0, c0, w_ih, w_hh, b_ih, b_hh, cols, pad_value, want_backward_state)


def lstm_series_backward(d_series, gates, cells, w_hh):
    """The backward recurrence of ``lstm_series`` in one launch (``ctc_amd_lstm_series_backward``) ->
    (dpre [T,B,4H], dh0 [B,H], dc0 [B,H]); ``d_series`` [T,B,>=H]: the upstream gradient of v_series."""
    return _series_backward("ctc_amd_lstm_series_backward", False, d_series, gates, cells, w_hh)


def lstm_series_wide(v_all, h0, c0, w_ih, w_hh, b_ih, b_hh, cols=None, pad_value=PAD_LOGIT, want_backward_state=False):
    """``lstm_series`` for every 1 <= I, H <= 160 (``ctc_amd_lstm_series_wide``: the benchmark's C = 158, and the narrow shapes
    too) -> (v_series [T,B,cols], gates [T,B,4H] | None, cells [T+1,B,H] | None), bit for bit what T calls of
    ``lstm_cell_step`` give, or None when the entry does not take the shape (I or H > 160, T B > 2^22 rows).  The scratch (the
    transposed weights, the x part of every row's pre-activations [T B, 4H]) is one ``torch.empty`` per call, for
    ``head_backward``'s reasons."""
    return _series_forward("ctc_amd_lstm_series_wide", "ctc_amd_lstm_series_wide_scratch_bytes", v_all, h0, c0, w_ih, w_hh, b_ih,
                           b_hh, cols, pad_value, want_backward_state)


def lstm_series_backward_wide(d_series, gates, cells, w_hh):
    """``lstm_series_backward`` for every 1 <= H <= 160 (``ctc_amd_lstm_series_backward_wide``, one launch, deterministic) ->
    (dpre [T,B,4H], dh0 [B,H], dc0 [B,H]), or None when the entry does not take the shape (H > 160)."""
    return _series_backward("ctc_amd_lstm_series_backward_wide", True, d_series, gates, cells, w_hh)


def lstm_bias_grad_wide(dpre):
    """The bias gradients behind ``lstm_series_backward_wide``: the column sums of ``dpre`` [T,B,4H] as one deterministic HIP launch
    (``ctc_amd_lstm_bias_grad_wide``: a fixed sum order, no scratch and nothing to clear) -> (d_b_ih [4H], d_b_hh [4H]), two
    tensors with the same values."""
    F._require_hip(dpre, "dpre")
    G = dpre.shape[-1]
    d = _f32c(dpre)
    rows = d.numel() // G
    d_b_ih, d_b_hh = (torch.empty(G, dtype=torch.float32, device=d.device) for _ in range(2))
    with F._on_device(d.device):
        rc = _lib.load().ctc_amd_lstm_bias_grad_wide(d.data_ptr(), rows, G // 4, d_b_ih.data_ptr(), d_b_hh.data_ptr(),
                                                     F._stream_handle(d.device))
    _answer(rc, "ctc_amd_lstm_bias_grad_wide", refusal_is_none=False)
    return d_b_ih, d_b_hh


def lstm_backward(d_series, gates, cells, v_all, h0, series, w_ih, w_hh, need_dx=True):
    """The backward of ``lstm_series`` on the HIP path, whole (``ctc_amd_lstm_backward``: the recurrence launch, one products
    launch, a reduce launch when T B > 128) -> (d_x [T,B,I] | None, dh0 [B,H], dc0 [B,H], d_w_ih [4H,I], d_w_hh [4H,H],
    d_b_ih [4H], d_b_hh [4H]), or None when the entry does not take the shape (what ``lstm_series`` refuses, or T B > 2^22
    rows).  ``gates`` / ``cells``: as ``lstm_series`` saved them; ``v_all`` [T,B,I]: the cell inputs; ``series`` [T,B,>=H]: the
    forward's v_series, whose rows are read in place as h_{t-1} (``h0`` for t = 0).  ``d_b_ih`` and ``d_b_hh`` are two tensors
    with the same values.  ``d_series`` / ``v_all`` / ``series`` are passed as they lie when their rows have unit stride and a
    pitch of at least their width; anything else (an expanded gradient with pitch 0) is copied first.  Deterministic (no atomics, fixed sum orders).  The scratch (dpre [T B, 4H], the partial sums) is one
    ``torch.empty`` per call, for ``head_backward``'s reasons."""
    F._require_hip(d_series, "d_series")
    F._require_hip(v_all, "v_all")
    T, B, I = v_all.shape
    H = h0.shape[1]
    dev = v_all.device
    f32 = torch.float32
    # rows the entry can address: unit stride over the columns and a row pitch of at least the width (autograd hands a
    # broadcast upstream gradient over with pitch 0, e.g. behind series.sum(1): that one is copied)
    ds, x, sr = (_rows(t, pitch=True) for t in (d_series, v_all, series))
    g, c, h, wi, wh = (_f32c(t) for t in (gates, cells, h0, w_ih, w_hh))
    scratch = _scratch("ctc_amd_lstm_backward_scratch_bytes", dev, T, B, I, H)
    if scratch is None:
        return None
    d_x = torch.empty((T, B, I), dtype=f32, device=dev) if need_dx else None
    dh0, dc0 = (torch.empty((B, H), dtype=f32, device=dev) for _ in range(2))
    d_w_ih = torch.empty((4 * H, I), dtype=f32, device=dev)
    d_w_hh = torch.empty((4 * H, H), dtype=f32, device=dev)
    d_b_ih, d_b_hh = (torch.empty(4 * H, dtype=f32, device=dev) for _ in range(2))
    with F._on_device(dev):
        rc = _lib.load().ctc_amd_lstm_backward(
            ds.data_ptr(), ds.stride(0), ds.stride(1), g.data_ptr(), c.data_ptr(), x.data_ptr(), x.stride(0), x.stride(1),
            h.data_ptr(), sr.data_ptr(), sr.stride(0), sr.stride(1), wi.data_ptr(), wh.data_ptr(), T, B, I, H,
            _ptr(d_x), B * I if need_dx else 0, I if need_dx else 0, dh0.data_ptr(), dc0.data_ptr(), d_w_ih.data_ptr(),
            d_w_hh.data_ptr(), d_b_ih.data_ptr(), d_b_hh.data_ptr(), scratch[0].data_ptr(), scratch[1], F._stream_handle(dev))
    return (d_x, dh0, dc0, d_w_ih, d_w_hh, d_b_ih, d_b_hh) if _answer(rc, "ctc_amd_lstm_backward") else None


def _series_backward_torch(d_series, v_all, w_ih, w_hh, hs, cs, gs, H, recurrence=lstm_series_backward, bias_grad=None):
    """the backward of the one-launch recurrence with torch arithmetic behind the recurrence launch (three rocBLAS GEMMs over
    all frames at once, a column sum, a clone): what runs outside the gate, and behind the wide recurrence
    (``recurrence=lstm_series_backward_wide``, where the column sum is a HIP launch too: ``bias_grad=lstm_bias_grad_wide``).
    hs [T+1,B,H]: h0 and the hidden states."""
    dpre, dh0, dc0 = recurrence(d_series, gs, cs, w_hh)
    flat = dpre.reshape(-1, 4 * H)
    if bias_grad is None:
        db = flat.sum(0)
        db_ih, db_hh = db, db.clone()
    else:
        db_ih, db_hh = bias_grad(dpre)
    return (dpre @ w_ih.float(), dh0, dc0, flat.t() @ v_all.reshape(-1, v_all.shape[2]).float(),
            flat.t() @ hs[:-1].reshape(-1, H), db_ih, db_hh, None, None)


def lstm_forward(feat, weight, bias, bn_weight, bn_bias, running_mean, running_var, eps, h0, c0, w_ih, w_hh, b_ih, b_hh,
                 cols=None, pad_value=PAD_LOGIT):
    """EVAL mode, no gradient: ``head_forward`` (running statistics, no mask) and ``lstm_series`` as ONE launch
    (``ctc_amd_lstm_forward``; the head's output stays in LDS) -> v_series [T,B,cols], bit-identical to the two launches, or
    None when the launch does not take the shape (2 C > 80, K not a multiple of 16, unaligned rows, T C beyond the LDS).  A bf16 /
    fp16 ``feat`` is read as it lies (``ctc_amd_lstm_forward_typed``, see ``_feat_call``); v_series stays fp32, the same bits."""
    F._require_hip(feat, "feat")
    T, B, K = feat.shape
    C = weight.shape[0]
    cols = C if cols is None else int(cols)
    dev = feat.device
    args = [_f32c(t) for t in (weight, bias, bn_weight, bn_bias, running_mean, running_var)]
    cell = [_f32c(t) for t in (h0, c0, w_ih, w_hh, b_ih, b_hh)]
    series = torch.empty((T, B, cols), dtype=torch.float32, device=dev)
    with F._on_device(dev):
        rc, _ = _feat_call("ctc_amd_lstm_forward", feat, (), lambda typed: (
            *(t.data_ptr() for t in args), float(eps), *(t.data_ptr() for t in cell), T, B, K, C, series.data_ptr(),
            series.stride(0), series.stride(1), cols, float(pad_value), None, None, F._stream_handle(dev)))
    return series if _answer(rc, "ctc_amd_lstm_forward") else None


# LSTM_cell.forward in eval mode takes the one-launch path up to this many head rows per workgroup (4 T: a workgroup does the
# head of its own four samples for all T frames, B / 4-way parallel where the separate head launch is T * ceil(C / 16)-way
# parallel, so beyond some T the two launches win -- whatever B is).  Measured, not guessed (profiles/r13_lstm_forward.md):
# T = 10, 12 and 16 win at B = 10 and at B = 256 (0.72 ... 0.78 and 0.54 ... 0.59 of the two launches' time), T = 20 loses at
# B = 10 (1.07 x), T = 150 at every B (1.2 - 1.5 x); the bound is the largest measured point that wins at every B measured.
FUSED_FORWARD_MAX_WG_ROWS = 64

# _HeadFn.backward takes the HIP path (head_backward) up to this many head rows T B; 0 closes the gate.  The scalar is T B
# because the measurements are ordered by it: the row pass and both products are T B rows of work, the torch arithmetic is
# launch-bound (110 - 150 us) up to a few thousand rows and a pair of rocBLAS GEMMs beyond, and at equal T B the ratio moves
# little with how T B splits into T and B.  Measured, not guessed (profiles/r14_head_backward.md, K = 1024, with and without
# d_feat): at T B = 100 ... 10240 the new call's median is 0.15 ... 0.79 of the torch arithmetic's and below the minimum of
# its rounds at every B in {10, 64, 256} and C in {33, 158}; at T B = 38400 it wins at C = 33 (0.24 - 0.35 x) and loses at
# C = 158 (1.02 - 1.09 x).  The bound is the largest measured point that wins at every B and C measured (r13's rule).
HEAD_BACKWARD_MAX_ROWS = 10240

# LSTM_cell._head takes the wide head (head_forward_wide: one launch in eval mode, two in train mode) for B > 256 up to this many
# head rows T B; 0 closes the gate, and such a batch goes through torch's four layers frame by frame as before.  T B for the
# neighbours' reason: the product, the statistics and the epilogue are T B rows of work, the comparator is 4 T torch kernels.
# Measured, not guessed (profiles/r18_head_wide.md, LSTM_cell._head with the gate open and closed, both captured into graphs,
# K = 1024, B in {512, 1024, 2048}, C in {33, 158}, train mode with p = 0.3 and eval mode): at every measured T B = 5120 ...
# 307200 the wide path's median is 0.07 ... 0.83 of the closed gate's and below the minimum of its rounds -- 0.70 ms against
# 6.41 ms in train mode at T = 150, B = 2048, C = 33, 2.82 ms against 6.88 ms at C = 158, 158 us against 286 us at T = 10, B = 512,
# C = 33; the narrowest win is eval mode at T = 10, B = 2048, C = 158 (228 us against 273 us).  The bound is the largest measured
# point that wins at every B and C measured (r13's rule); no measured point loses, so it is the largest measured point.
HEAD_WIDE_MAX_ROWS = 307200

# _HeadFn.backward behind the wide head takes the HIP path (head_backward_wide) up to this many head rows T B; 0 closes the gate,
# and _head_backward_torch runs on the saved state, as it does beyond the gate.  Measured, not guessed (profiles/r18_head_wide.md,
# the same shapes, train mode, with and without d_feat, both bodies captured into graphs): at T B = 5120, 10240 and 20480 the new
# call's median is 0.27 ... 0.85 of the torch arithmetic's and below the minimum of its rounds at every B and C; at T B = 76800,
# 153600 and 307200 it wins at C = 33 (0.29 ... 0.33 x: 2.03 ms against 6.81 ms at T = 150, B = 2048) and loses at C = 158
# (1.16 ... 1.29 x: the products launch, ctc_amd_head_backward's own, against two rocBLAS GEMMs -- what closes
# HEAD_BACKWARD_MAX_ROWS at 10240 too).  The bound is the largest measured point that wins at every B and C measured (r13's rule).
HEAD_WIDE_BACKWARD_MAX_ROWS = 20480

# _SeriesFn.backward takes the HIP path whole (lstm_backward) up to this many rows T B; 0 closes the gate.  T B for
# HEAD_BACKWARD_MAX_ROWS's reason: the products and the column sums are T B rows of work, the torch arithmetic behind the
# recurrence launch is launch-bound at small T B and three rocBLAS GEMMs beyond.  Measured, not guessed
# (profiles/r15_lstm_backward.md, both bodies captured into graphs, (I, H) in {(33, 33), (38, 38)}, with and without d_x): at
# every measured T B = 100 ... 38400 the new call's median is 0.49 ... 0.97 of the closed gate's and below the minimum of its
# rounds at every B in {10, 64, 256} -- behind the recurrence launch both start with, 17 us against 39 us at T B = 100 and
# 130 us against 249 us at T B = 38400.  The bound is the largest measured point that wins at every B and (I, H) measured
# (r13's rule); no measured point loses, so it is the largest measured point.
SERIES_BACKWARD_MAX_ROWS = 38400

# _SeriesFn takes the wide recurrence (lstm_series_wide forward; lstm_series_backward_wide, lstm_bias_grad_wide and
# _series_backward_torch's three GEMMs backward)
# for the shapes lstm_series refuses, I and H up to 160, up to this many rows T B; 0 closes the gate, and the T step launches
# and the BPTT loop of torch kernels run as before.  T B for the neighbours' reason: the x part, the saved state and the torch
# arithmetic behind the backward launch are T B rows of work, and the comparator is launch-bound (T step launches, then about
# two dozen torch kernels per frame).  Measured, not guessed (profiles/r16_lstm_wide.md, forward + backward captured into one
# graph, I = H in {158, 96}): at every measured T B = 100 ... 38400 the open path's median is 0.09 ... 0.27 of the closed
# gate's and below the minimum of its rounds at every B in {10, 64, 256} -- 5.40 ms against 57.2 ms at T = 150, B = 256,
# C = 158, 0.43 ms against 1.63 ms at T = 10, B = 10; forward alone 0.23 ... 0.46, backward alone 0.07 ... 0.23; every graph
# replay gives the eager bits.  The bound
# is the largest measured point that wins at every B and H measured (r13's rule); no measured point loses, so it is the
# largest measured point.
SERIES_WIDE_MAX_ROWS = 38400
SERIES_WIDE_MAX_CLASSES = 160                        # kWideMax of csrc/lstm_wide.hpp: the bound of the wide entries on I and H


class _SeriesFn(torch.autograd.Function):
    """v_all [T,B,I], (h0, c0), LSTMCell parameters -> v_series [T,B,cols]: one launch for the reference's class counts, the
    wide recurrence (``ctx.wide``) up to 160 classes and T B <= ``SERIES_WIDE_MAX_ROWS`` rows, T fused launches otherwise.  Backward of the one launch: ``lstm_backward`` (HIP, whole) for T B <=
    ``SERIES_BACKWARD_MAX_ROWS`` rows; beyond the gate, and when the entry does not take the shape, the recurrence launch and
    ``_series_backward_torch``.  Backward of the wide recurrence: its own recurrence launch and ``_series_backward_torch``.
    Backward of the T launches: BPTT in torch."""

    @staticmethod
    def forward(ctx, v_all, h0, c0, w_ih, w_hh, b_ih, b_hh, cols, pad_value):
        T, B, _ = v_all.shape
        H = h0.shape[1]
        need = any(ctx.needs_input_grad[:7])
        ctx.H = H
        ctx.wide = False
        whole = lstm_series(v_all, h0, c0, w_ih, w_hh, b_ih, b_hh, cols, pad_value, want_backward_state=need)
        if whole is not None:
            series, gates, cells = whole
            ctx.one_launch = need
            ctx.in_place = need and T * B <= SERIES_BACKWARD_MAX_ROWS
            if ctx.in_place:                                 # h_{t-1} is read from v_series itself: no concatenated copy
                ctx.save_for_backward(v_all, w_ih, w_hh, h0.detach(), cells, gates, series)
            elif need:
                hs = torch.cat([h0.detach().float().unsqueeze(0), series[:, :, :H]])
                ctx.save_for_backward(v_all, w_ih, w_hh, hs, cells, gates)
            return series
        ctx.in_place = False
        ctx.one_launch = False
        if 0 < T * B <= SERIES_WIDE_MAX_ROWS and max(v_all.shape[2], H) <= SERIES_WIDE_MAX_CLASSES:   # beyond the narrow entry's sizes
            whole = lstm_series_wide(v_all, h0, c0, w_ih, w_hh, b_ih, b_hh, cols, pad_value, want_backward_state=need)
            if whole is not None:
                series, gates, cells = whole
                ctx.wide = need
                if need:
                    hs = torch.cat([h0.detach().float().unsqueeze(0), series[:, :, :H]])
                    ctx.save_for_backward(v_all, w_ih, w_hh, hs, cells, gates)
                return series
        series = torch.empty((T, B, cols), dtype=torch.float32, device=v_all.device)
        hs, cs, gs = [h0], [c0], []
        h, c = h0, c0
        for t in range(T):
            h, c, g = lstm_cell_step(v_all[t], h, c, w_ih, w_hh, b_ih, b_hh, series[t], pad_value, want_gates=need)
            if need:
                hs.append(h); cs.append(c); gs.append(g)
        if need:
            ctx.save_for_backward(v_all, w_ih, w_hh, torch.stack(hs), torch.stack(cs), torch.stack(gs))
        return series

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_series):
        H = ctx.H
        if ctx.in_place:                                     # the gate was open in forward: (h0, series) saved, not their concatenation
            v_all, w_ih, w_hh, h0, cs, gs, series = ctx.saved_tensors
            res = None
            if v_all.shape[0] * v_all.shape[1] <= SERIES_BACKWARD_MAX_ROWS:
                res = lstm_backward(d_series, gs, cs, v_all, h0, series, w_ih, w_hh, ctx.needs_input_grad[0])
            if res is not None:
                return tuple(res) + (None, None)
            hs = torch.cat([h0.float().unsqueeze(0), series[:, :, :H]])
            return _series_backward_torch(d_series, v_all, w_ih, w_hh, hs, cs, gs, H)
        v_all, w_ih, w_hh, hs, cs, gs = ctx.saved_tensors
        T = v_all.shape[0]
        if ctx.one_launch:                                   # the recurrence in one launch, the rest as GEMMs over all frames
            return _series_backward_torch(d_series, v_all, w_ih, w_hh, hs, cs, gs, H)
        if getattr(ctx, "wide", False):                     # the same behind the wide recurrence launch
            return _series_backward_torch(d_series, v_all, w_ih, w_hh, hs, cs, gs, H, lstm_series_backward_wide,
                                          lstm_bias_grad_wide)
        dh = torch.zeros_like(hs[0])
        dc = torch.zeros_like(cs[0])
        dv = torch.empty_like(v_all)
        dw_ih, dw_hh = torch.zeros_like(w_ih), torch.zeros_like(w_hh)
        db = torch.zeros(4 * H, dtype=torch.float32, device=v_all.device)
        for t in range(T - 1, -1, -1):
            dh = dh + d_series[t, :, :H]
            i, f, g, o = gs[t].split(H, dim=1)
            tc = torch.tanh(cs[t + 1])
            dc = dc + dh * o * (1.0 - tc * tc)
            dpre = torch.cat([dc * g * i * (1.0 - i), dc * cs[t] * f * (1.0 - f), dc * i * (1.0 - g * g),
                              dh * tc * o * (1.0 - o)], dim=1)
            dv[t] = dpre @ w_ih
            dw_ih += dpre.t() @ v_all[t]
            dw_hh += dpre.t() @ hs[t]
            db += dpre.sum(0)
            dh = dpre @ w_hh
            dc = dc * f
        return dv, dh, dc, dw_ih, dw_hh, db, db.clone(), None, None


class LSTM_cell(nn.Module):
    """``LSTM_cell(args)`` as in the reference (``args.extract_feat_dim``, ``.v_class``, ``.batch_size``, ``.temporal``);
    ``forward(feat[T,B,feat_dim], v_hsn[B,C], v_csn[B,C]) -> v_series[T,B,C]`` (``[T,B,C+1]`` with ``pad_classes`` and odd C)."""

    def __init__(self, args, _BaseModule=BasicModule, pad_classes=False):
        super().__init__()
        self.args = args
        self.input_size = args.extract_feat_dim
        self.v_class = args.v_class
        self.batch_size = args.batch_size
        self.temporal = args.temporal
        self.pad_classes = bool(pad_classes)
        self.v = _BaseModule(self.input_size, self.v_class)
        self.v_cell = nn.LSTMCell(self.v_class, self.v_class)

    def _std_layers(self):
        """self.v's four layers when it is the reference's BasicModule (what the HIP head computes), else None"""
        layers = getattr(self.v, "layers", None)
        std = (isinstance(layers, nn.Sequential) and len(layers) == 4 and isinstance(layers[0], nn.Linear)
               and isinstance(layers[1], nn.BatchNorm1d) and isinstance(layers[2], nn.ReLU) and isinstance(layers[3], nn.Dropout)
               and layers[0].bias is not None and layers[1].affine and layers[1].track_running_stats)
        return layers if std else None

    def _head(self, feat):
        """self.v applied to every frame (LSTM.py:48): one launch when self.v is the reference's BasicModule and the shape
        is one the launch takes, the module itself frame by frame otherwise (a custom _BaseModule, ...).  B > 256: the wide
        launches (``head_forward_wide``) for T B <= ``HEAD_WIDE_MAX_ROWS`` rows, the module frame by frame beyond that gate."""
        T = self.temporal
        layers = self._std_layers()
        std = layers is not None
        B, K = feat.shape[1], feat.shape[2]
        wide_closed = B > 256 and T * B > HEAD_WIDE_MAX_ROWS
        if not std or feat.shape[0] < T or wide_closed or K % 16 or (self.training and (B < 2 or layers[1].momentum is None)):
            return torch.stack([self.v(feat[time]) for time in range(T)])
        lin, bn, drop = layers[0], layers[1], layers[3]
        x = feat[:T]
        mask = None
        if self.training and drop.p > 0:                     # torch draws the mask (its Philox stream), one call for all frames
            mask = torch.nn.functional.dropout(torch.ones((T, B, lin.out_features), dtype=torch.float32, device=feat.device),
                                               drop.p, True)
        if not self.training:
            return _HeadFn.apply(x, lin.weight, lin.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps, mask)[0]
        out, mean, var = _HeadFn.apply(x, lin.weight, lin.bias, bn.weight, bn.bias, None, None, bn.eps, mask)
        with torch.no_grad():                                # the running statistics, as T per-frame calls would leave them
            m = float(bn.momentum)
            coef = m * (1.0 - m) ** torch.arange(T - 1, -1, -1, dtype=torch.float32, device=feat.device)
            keep = (1.0 - m) ** T
            bn.running_mean.mul_(keep).add_(coef @ mean)
            bn.running_var.mul_(keep).add_(coef @ (var * (B / (B - 1.0))))
            bn.num_batches_tracked += T
        return out

    def _forward_one_launch(self, feat, v_hsn, v_csn, cols):
        """eval mode, the standard head, nothing that needs a gradient, a shape inside the measured gate: feat -> v_series as
        ONE launch (``lstm_forward``, bit-identical to the two launches).  None: the caller takes the two launches."""
        T = self.temporal
        layers = None if self.training else self._std_layers()
        if layers is None or feat.dim() != 3 or feat.shape[0] < T or 4 * T > FUSED_FORWARD_MAX_WG_ROWS:
            return None
        # B > 256 stays closed here: the head of such a batch is head_forward_wide's launch, followed by the recurrence's; whether
        # one launch from feat to v_series pays at these batches has not been measured (a measurement of its own).
        if feat.shape[1] > 256:
            return None
        if torch.is_grad_enabled() and any(t.requires_grad for t in (feat, v_hsn, v_csn, *self.parameters())):
            return None
        lin, bn, cell = layers[0], layers[1], self.v_cell
        return lstm_forward(feat[:T], lin.weight, lin.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps,
                            v_hsn, v_csn, cell.weight_ih, cell.weight_hh, cell.bias_ih, cell.bias_hh, cols, PAD_LOGIT)

    def forward(self, feat, v_hsn, v_csn):
        F._require_hip(feat, "feat")
        H = self.v_class
        cols = H + 1 if (self.pad_classes and H % 2) else H
        cell = self.v_cell
        series = self._forward_one_launch(feat, v_hsn, v_csn, cols)
        if series is not None:
            return series
        v_all = self._head(feat)                             # (BatchNorm statistics per frame, as the reference)
        return _SeriesFn.apply(v_all, v_hsn, v_csn, cell.weight_ih, cell.weight_hh, cell.bias_ih, cell.bias_hh, cols, PAD_LOGIT)
