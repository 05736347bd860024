"""autograd.Function front-end of the HIP CTC engine.

Surface (BASELINE north_star): ``CTCLoss.apply(log_probs, targets, input_lengths,
target_lengths)`` -> 0-dim fp32 loss, differentiable w.r.t. ``log_probs``.

Mirrors the call convention of the reference's loss modules
(``ctc_loss(v_output, v_target, input_length, v_target_length)``, train.py:427,576):

* ``log_probs`` are RAW LOGITS [T,B,C] -- the module applies LogSoftmax(dim=2)
  (NoBlankCTC.py:136) / Sigmoid (NoBlankBinaryCTC.py:146) itself; the returned
  gradient is w.r.t. those logits.
* ``targets`` [B,S] integer class indices (int32 or int64, -1 padded) selects the
  no-blank loss; [B,S,C] float multi-hot rows selects the binary variant.
* loss = mean over the batch only, no division by target length (NoBlankCTC.py:139-140).

Forward runs ONE fused HIP launch that produces the loss and (when the input needs
a gradient) the whole input gradient; backward multiplies that buffer by the upstream
gradient on the device (a no-op launch when it is 1.0, i.e. ``loss.backward()``).
There is no CPU path: non-HIP tensors raise.

The read-outs of the no-blank and the binary lattice (``*_best_path``, ``*_posteriors``, ``*_token_spans``) take float32,
bfloat16 or float16 logits: 2-byte logits are read as they lie by the ``_typed`` entries of include/ctc_amd.h, and every
output is bit for bit that of the same call on ``logits.float()``.
"""
import math
import os
from typing import NamedTuple

import torch

from . import _lib

_workspaces = {}           # (device index, raw stream, variant) -> [tensor, ...]; the LAST one is current
_ws_need = {}              # (variant, T, B, C, S) -> bytes
_VALIDATE = os.environ.get("CTC_AMD_VALIDATE", "0") == "1"
# 2-byte logits the no-blank loss reads natively (include/ctc_amd.h, ctc_amd_noblank_loss_grad_typed)
_LOWP_CODE = {torch.bfloat16: _lib.BF16, torch.float16: _lib.F16}
_LOWP_DOMAIN = ("C even <= 256, S <= 31, T <= 168, even strides and 4-byte aligned rows")
# 2-byte logits the no-blank / binary read-outs hand to their `_typed` entries as they lie.  A dtype that is
# accepted (`_LOWP_CODE`) but missing here is cast with `.float()` in front of the untyped entry -- the same bits, one more
# launch: tools/readout_typed_bench.py empties this dict to time that path in the same process.
_LOWP_READOUT = {torch.bfloat16: _lib.BF16, torch.float16: _lib.F16}
_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream_handle(device):
    """hipStream_t of torch's current stream on `device` as an integer (no Stream object built)."""
    if _raw_stream is not None:
        return _raw_stream(device.index)
    return torch.cuda.current_stream(device).cuda_stream


def _workspace(variant, T, B, C, S, device, stream=None):
    """Zero-initialised once, one per (device, stream, variant): see include/ctc_amd.h.

    A workspace that has become too small is SUPERSEDED, not freed: a hipGraph captured earlier still holds its raw
    pointer (the calls are capture-safe, tests capture after an eager warm-up), and replaying it must not write
    counters and lattices into memory the allocator has handed to someone else.  So that a loop whose shapes keep
    growing (length-bucketed batches with rising T) does not pile up one buffer per new maximum, a superseding
    buffer is at least 1.5x its predecessor: O(log) buffers, at most ~3x the largest need held in total.
    `release_workspaces()` frees them all when the caller knows no captured graph is alive."""
    shape = (variant, T, B, C, S)
    need = _ws_need.get(shape)
    if need is None:
        need = _ws_need[shape] = _lib.load().ctc_amd_workspace_bytes(variant, T, B, C, S)
    key = (device.index, _stream_handle(device) if stream is None else stream, variant)
    held = _workspaces.get(key)
    if held is None:
        held = _workspaces[key] = []
    if not held or held[-1].numel() < need:
        size = need if not held else max(need, held[-1].numel() + held[-1].numel() // 2)
        held.append(torch.zeros((size + 4095) & ~4095, dtype=torch.uint8, device=device))
    return held[-1]


def release_workspaces(device=None):
    """Frees the hidden workspaces of `device` (all devices if None), superseded ones included, and returns the bytes
    released.  ONLY when no hipGraph that captured a call of this module is still going to be replayed (it holds the raw
    pointers) -- eager loops may call it at any time: it synchronises the device(s) first, and the next call allocates
    afresh.  Also drops the entries of streams that no longer exist (the key carries the raw stream handle)."""
    want = None if device is None else torch.device(device).index
    freed = 0
    for key in list(_workspaces):
        if want is not None and key[0] != want:
            continue
        torch.cuda.synchronize(key[0])
        freed += sum(w.numel() for w in _workspaces[key])
        del _workspaces[key]
    return freed


STATUS_BITS = {1: "no-blank launch", 2: "binary launch", 4: "blank-CTC launch", 8: "blank-CTC best path",
               16: "blank-CTC posteriors"}


def workspace_status(device=None, clear=True):
    """OR of the status words of this process's hidden workspaces on `device` (all devices if None).

    0 = every in-launch hand-off completed.  A non-zero value means a bounded wait ran out in some
    launch since the last clear (the affected outputs were filled with NaN, include/ctc_amd.h);
    synchronises the workspaces' streams."""
    import ctypes
    lib = _lib.load()
    total = 0
    for (dev_index, stream, _variant), held in list(_workspaces.items()):
        if device is not None and torch.device(device).index not in (None, dev_index):
            continue
        with torch.cuda.device(dev_index):
            for ws in held:
                word = ctypes.c_uint(0)
                rc = lib.ctc_amd_workspace_status(ws.data_ptr(), int(bool(clear)), stream, ctypes.byref(word))
                if rc:
                    _lib.check(rc, "ctc_amd_workspace_status")
                total |= word.value
    return total


def check_status(device=None):
    """Raise CtcAmdError if any launch since the last check reported a starved hand-off."""
    st = workspace_status(device, clear=True)
    if st:
        what = ", ".join(v for k, v in STATUS_BITS.items() if st & k)
        raise _lib.CtcAmdError("ctc_amd: an in-launch wait ran out (%s, status %d): the outputs of that call "
                               "carry NaN -- see include/ctc_amd.h, ctc_amd_workspace_status" % (what, st))


def collective_gate(variant, batch, device=None, launch_stream=None, timeout_us=30):
    """Enqueue, on the CURRENT stream, a one-wave kernel that returns once the next no-blank / binary loss launch
    issued on `launch_stream` (default: the stream that is current now ... call this under
    ``torch.cuda.stream(side)`` with ``launch_stream=main.cuda_stream``) has filled the chip, or after `timeout_us`.
    Put it between the previous loss launch and an asynchronous collective so that the collective's kernel is
    not dispatched in front of the next launch (include/ctc_amd.h: ctc_amd_collective_gate).  No-op (returns
    False) when that stream has not run a loss of this variant yet."""
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    key = (dev.index, _stream_handle(dev) if launch_stream is None else launch_stream,
           {"noblank": _lib.NOBLANK, "binary": _lib.BINARY}.get(variant, variant))
    held = _workspaces.get(key)
    if not held:
        return False
    with _on_device(dev):
        rc = _lib.load().ctc_amd_collective_gate(held[-1].data_ptr(), int(batch), int(timeout_us), _stream_handle(dev))
    if rc:
        _lib.check(rc, "ctc_amd_collective_gate")
    return True


BLANK_MAX_LABELS = 1023            # ctc_amd_blank_loss_grad, the best path and the posteriors: S <= 1023
BLANK_NARROW_LABELS = 255          # beyond: the wide entries (ctc_amd_blank_best_path_wide, ctc_amd_blank_posteriors_wide)


def set_blank_schedule(mode):
    """-1: the library chooses (default); 1 / 0: force / forbid the persistent blank-CTC launch; 2: force it with the
    worker pool gathering the emission rows.  Targets of more than 255 label columns always take the wide
    three-launch path, whatever is set here."""
    _lib.check(_lib.load().ctc_amd_blank_set_schedule(int(mode)), "ctc_amd_blank_set_schedule")


class _NullCtx:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


_NULL = _NullCtx()


def _on_device(dev):
    """device guard only when the tensor's device is not already current (saves a few us per call)"""
    return _NULL if torch.cuda.current_device() == dev.index else torch.cuda.device(dev)


def _require_hip(x, name):
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise _lib.CtcAmdError(
            "ctc_amd: %s must be a tensor on a HIP (cuda) device -- the engine has no CPU path" % name)


def _lengths(v, B, lo_name, device, hi, lo=1):
    """-> int64 device tensor [B]; values are validated on the host only when that
    costs no device synchronisation (CPU input) or CTC_AMD_VALIDATE=1."""
    if (v.__class__ is torch.Tensor and v.is_cuda and v.dtype is torch.int64 and v.device == device and v.dim() == 1
            and v.shape[0] == B and v.is_contiguous() and not _VALIDATE):
        return v                                    # the usual case (train.py:397-399): nothing to convert or check
    if not isinstance(v, torch.Tensor):
        v = torch.as_tensor(v, dtype=torch.int64)
    if v.dim() != 1 or v.numel() != B:
        raise ValueError("ctc_amd: %s must have shape [%d], got %s" % (lo_name, B, tuple(v.shape)))
    if v.dtype not in (torch.int64, torch.int32, torch.int16, torch.uint8, torch.int8):
        raise ValueError("ctc_amd: %s must be an integer tensor, got %s" % (lo_name, v.dtype))
    if not v.is_cuda or _VALIDATE:
        h = v.detach().cpu()
        if h.numel() and (int(h.min()) < lo or int(h.max()) > hi):
            raise ValueError("ctc_amd: %s must lie in [%d, %d]" % (lo_name, lo, hi))
    if v.dtype == torch.int64 and v.device == device and v.is_contiguous():
        return v
    return v.to(device=device, dtype=torch.int64, non_blocking=True).contiguous()


def _placed(t, dev, dtype=None):
    """`t` as a contiguous tensor on `dev` (of `dtype` if given): itself when it already is one"""
    if (dtype is None or t.dtype is dtype) and t.device == dev and t.is_contiguous():
        return t
    return t.to(device=dev, dtype=dtype, non_blocking=True).contiguous()


def _variant_of(targets):
    if targets.dim() == 2 and not targets.dtype.is_floating_point:
        return _lib.NOBLANK
    if targets.dim() == 3 and targets.dtype.is_floating_point:
        return _lib.BINARY
    raise ValueError("ctc_amd: targets must be [B,S] integer (no-blank) or [B,S,C] float (binary), got "
                     "%s %s" % (tuple(targets.shape), targets.dtype))


def _launch(variant, x, targets, in_len, tgt_len, want_grad, batch_total, blank=0, label_smoothing=None):
    """Validate, allocate outputs and enqueue the fused kernel.  -> (loss, nll, grad|None)"""
    if x.__class__ is not torch.Tensor and not isinstance(x, torch.Tensor) or not x.is_cuda:
        _require_hip(x, "log_probs")
    if x.dim() != 3:
        raise ValueError("ctc_amd: log_probs must be [T,B,C], got %s" % (tuple(x.shape),))
    lowp = _LOWP_CODE.get(x.dtype) if variant == _lib.NOBLANK else None
    if x.dtype is not torch.float32 and lowp is None:
        raise ValueError("ctc_amd: log_probs must be float32 (the engine computes in fp32; the no-blank loss also reads "
                         "bfloat16 / float16), got %s" % x.dtype)
    T, B, C = x.shape
    if T < 1 or B < 1 or C < 1:
        raise ValueError("ctc_amd: empty log_probs %s" % (tuple(x.shape),))
    dev = x.device
    xs = x.detach() if x.requires_grad else x
    st, sb, sc = xs.stride()
    if sc != 1:
        xs = xs.contiguous()
        st, sb, sc = xs.stride()
    if not isinstance(targets, torch.Tensor):
        raise ValueError("ctc_amd: targets must be a tensor")
    tshape = targets.shape
    if tshape[0] != B:
        raise ValueError("ctc_amd: targets batch %d != log_probs batch %d" % (tshape[0], B))
    S = tshape[1]
    if S < 1:
        raise ValueError("ctc_amd: targets need at least one label column")
    tdt = targets.dtype
    if variant == _lib.BINARY:
        if tshape[2] != C:
            raise ValueError("ctc_amd: binary targets last dim %d != C %d" % (tshape[2], C))
        tg = _placed(targets, dev, torch.float32)
    else:
        if tdt is not torch.int32 and tdt is not torch.int64:
            targets = targets.long()
        tg = _placed(targets, dev)
    il = _lengths(in_len, B, "input_lengths", dev, T)
    tl = _lengths(tgt_len, B, "target_lengths", dev, S, lo=0 if variant == _lib.BLANK else 1)
    scale = 1.0 / (B if batch_total is None else int(batch_total))
    # nll and the loss are tensors of their own, not views of one buffer: autograd refuses in-place arithmetic
    # on a view returned by a custom Function (`loss /= accum_steps`, `loss += aux` in a training loop)
    nll = torch.empty(B, dtype=torch.float32, device=dev)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    grad = torch.empty((T, B, C), dtype=x.dtype, device=dev) if want_grad else None
    lib = _lib.load()
    with _on_device(dev):
        stream = _stream_handle(dev)
        ws = _workspace(variant, T, B, C, S, dev, stream)
        gp = grad.data_ptr() if want_grad else None
        op, lp_ = nll.data_ptr(), loss.data_ptr()
        if lowp is not None:
            ls = -1.0 if label_smoothing is None else float(label_smoothing)
            if label_smoothing is not None and not 0.0 <= ls <= 1.0:   # (< 0 means "plain" to the typed entry)
                _lib.check(_lib.ERR_BAD_ARGUMENT, "ctc_amd_noblank_loss_grad_typed")
            rc = lib.ctc_amd_noblank_loss_grad_typed(
                xs.data_ptr(), lowp, st, sb, tg.data_ptr(), int(tg.dtype is torch.int64),
                il.data_ptr(), tl.data_ptr(), T, B, C, S, ls, scale, scale, op, lp_, gp, ws.data_ptr(), stream)
            if rc == _lib.ERR_UNSUPPORTED_SHAPE:
                raise _lib.CtcAmdError(
                    "ctc_amd: %s logits [T=%d, B=%d, C=%d] with S=%d are outside the no-blank loss's reduced-precision "
                    "domain (%s); pass log_probs.float() for other shapes" % (x.dtype, T, B, C, S, _LOWP_DOMAIN))
            if rc:
                _lib.check(rc, "ctc_amd_noblank_loss_grad_typed")
        elif variant == _lib.NOBLANK and label_smoothing is not None:
            rc = lib.ctc_amd_noblank_smoothed_loss_grad(
                xs.data_ptr(), st, sb, tg.data_ptr(), int(tg.dtype is torch.int64),
                il.data_ptr(), tl.data_ptr(), T, B, C, S, float(label_smoothing), scale, scale,
                op, lp_, gp, ws.data_ptr(), stream)
            if rc:
                _lib.check(rc, "ctc_amd_noblank_smoothed_loss_grad")
        elif variant == _lib.NOBLANK:
            rc = lib.ctc_amd_noblank_loss_grad(
                xs.data_ptr(), st, sb, tg.data_ptr(), int(tg.dtype is torch.int64),
                il.data_ptr(), tl.data_ptr(), T, B, C, S, scale, scale,
                op, lp_, gp, ws.data_ptr(), stream)
            if rc:
                _lib.check(rc, "ctc_amd_noblank_loss_grad")
        elif variant == _lib.BINARY:
            rc = lib.ctc_amd_binary_loss_grad(
                xs.data_ptr(), st, sb, tg.data_ptr(),
                il.data_ptr(), tl.data_ptr(), T, B, C, S, scale, scale,
                op, lp_, gp, ws.data_ptr(), stream)
            if rc:
                _lib.check(rc, "ctc_amd_binary_loss_grad")
        else:
            rc = lib.ctc_amd_blank_loss_grad(
                xs.data_ptr(), st, sb, tg.data_ptr(), int(tg.dtype is torch.int64),
                il.data_ptr(), tl.data_ptr(), T, B, C, S, int(blank), scale, scale,
                op, lp_, gp, ws.data_ptr(), stream)
            if rc == _lib.ERR_UNSUPPORTED_SHAPE and S > BLANK_MAX_LABELS:
                raise _lib.CtcAmdError(
                    "ctc_amd: the blank CTC loss takes targets of at most %d label columns (2S+1 <= %d lattice states), "
                    "got S=%d" % (BLANK_MAX_LABELS, 2 * BLANK_MAX_LABELS + 1, S))
            if rc:
                _lib.check(rc, "ctc_amd_blank_loss_grad")
    if _VALIDATE:
        check_status(dev)
    return loss, nll, grad


def _scaled_grad(ctx, gout):
    """upstream gradient x the buffer the forward launch filled (in place, on device)."""
    grad = ctx.grad
    ctx.grad = None                         # the buffer is handed to autograd exactly once
    if grad is None:                        # backward again (retain_graph): recompute
        x, targets = ctx.saved_tensors
        variant, batch_total, blank, smoothing = ctx.meta
        _, _, grad = _launch(variant, x, targets, ctx.lens[0], ctx.lens[1], True, batch_total, blank, smoothing)
    g = gout
    if g.dtype is not torch.float32 or g.device != grad.device or not g.is_contiguous() or g.requires_grad:
        g = g.detach().to(device=grad.device, dtype=torch.float32).contiguous()
    dev = grad.device
    with _on_device(dev):
        if grad.dtype is torch.float32:
            rc = _lib.load().ctc_amd_scale_grad(grad.data_ptr(), g.data_ptr(), grad.numel(), _stream_handle(dev))
        else:                               # the no-blank loss's bf16 / fp16 gradient
            rc = _lib.load().ctc_amd_scale_grad_typed(grad.data_ptr(), _LOWP_CODE[grad.dtype], g.data_ptr(),
                                                      grad.numel(), _stream_handle(dev))
    if rc:
        _lib.check(rc, "ctc_amd_scale_grad")
    return grad


class _LossFn(torch.autograd.Function):
    """(loss, nll) with the input gradient produced by the forward launch."""

    @staticmethod
    def forward(ctx, x, targets, in_len, tgt_len, variant, batch_total, blank, label_smoothing=None):
        want = ctx.needs_input_grad[0]
        loss, nll, grad = _launch(variant, x, targets, in_len, tgt_len, want, batch_total, blank, label_smoothing)
        ctx.grad = grad
        ctx.meta = (variant, batch_total, blank, label_smoothing)
        if want:
            ctx.save_for_backward(x, targets)
            ctx.lens = (in_len, tgt_len)
        ctx.mark_non_differentiable(nll)
        return loss, nll

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gout, _gnll):
        return _scaled_grad(ctx, gout), None, None, None, None, None, None, None


_host_ext = False          # the C++ autograd Function (csrc/autograd_ext.cpp): False = not looked for yet, None = absent


def _load_host_ext():
    """ctc_amd/lib/ext/ctc_amd_autograd_ext.so, built by ctc_amd.build.build_host_ext().  It only shortens the HOST side
    of an eager step (the same C-ABI calls from a C++ autograd node): absent or CTC_AMD_HOST_EXT=0 -> the Python
    Functions below do the same launches."""
    global _host_ext
    _host_ext = None
    if os.environ.get("CTC_AMD_HOST_EXT", "1") == "0":
        return None
    import ctypes
    import importlib.util
    from .build import HOST_EXT_SO
    if not os.path.exists(HOST_EXT_SO):
        return None
    try:                                                       # optional: anything wrong with it (built against another torch:
        from .build import host_ext_is_current                 # undefined symbols, a missing entry point) -> the Python Functions
        if not host_ext_is_current():
            raise ImportError("built for another torch version")
        spec = importlib.util.spec_from_file_location("ctc_amd_autograd_ext", HOST_EXT_SO)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        lib = _lib.load()
        addr = lambda f: ctypes.cast(f, ctypes.c_void_p).value
        mod.set_abi(addr(lib.ctc_amd_noblank_loss_grad), addr(lib.ctc_amd_binary_loss_grad), addr(lib.ctc_amd_scale_grad))
    except (ImportError, OSError, AttributeError, RuntimeError) as e:
        import warnings
        warnings.warn("ctc_amd: the C++ autograd node (%s) is unusable (%s: %s); the Python Function issues the same "
                      "launches" % (os.path.basename(HOST_EXT_SO), type(e).__name__, e))
        return None
    _host_ext = mod
    return mod


def _fast_apply(x, targets, in_len, tgt_len, batch_total, variant=None):
    """-> [loss, nll] through the C++ autograd node when every argument is already in the form the launch takes
    (float32 logits on the current HIP device with unit stride over the classes, targets and int64 lengths contiguous
    on that device), else None: the Python Function converts, validates and raises."""
    ext = _host_ext
    if ext is False:
        ext = _load_host_ext()
    if ext is None or _VALIDATE:
        return None
    T = torch.Tensor
    if not (x.__class__ is T and targets.__class__ is T and in_len.__class__ is T and tgt_len.__class__ is T):
        return None
    if not x.is_cuda or x.dtype is not torch.float32 or x.dim() != 3 or x.stride(2) != 1:
        return None
    dev = x.device
    Tn, B, C = x.shape
    tdim, tdt = targets.dim(), targets.dtype
    if tdim == 2 and (tdt is torch.int32 or tdt is torch.int64):
        v = _lib.NOBLANK
    elif tdim == 3 and tdt is torch.float32 and targets.shape[2] == C:
        v = _lib.BINARY
    else:
        return None
    if variant is not None and v != variant:
        return None
    S = targets.shape[1]
    if (Tn < 1 or B < 1 or C < 1 or S < 1 or targets.shape[0] != B or targets.device != dev or not targets.is_contiguous()
            or in_len.dtype is not torch.int64 or tgt_len.dtype is not torch.int64 or in_len.device != dev
            or tgt_len.device != dev or in_len.dim() != 1 or tgt_len.dim() != 1 or in_len.shape[0] != B
            or tgt_len.shape[0] != B or not in_len.is_contiguous() or not tgt_len.is_contiguous()
            or torch.cuda.current_device() != dev.index or targets.requires_grad):
        return None
    stream = _stream_handle(dev)
    ws = _workspace(v, Tn, B, C, S, dev, stream)
    try:
        return ext.ctc_loss(x, targets, in_len, tgt_len, v, 0 if batch_total is None else int(batch_total), stream, ws.data_ptr())
    except RuntimeError as e:
        if "ctc_amd: fused launch failed" in str(e):
            return None                      # the Python Function repeats the call and raises the library's own error
        raise


class CTCLoss(torch.autograd.Function):
    """Drop-in ``CTCLoss.apply(log_probs, targets, input_lengths, target_lengths)``.

    The variant follows the targets: [B,S] integer -> NoBlankCTC arithmetic
    (NoBlankCTC.py:129-141), [B,S,C] float -> NoBlankBinaryCTC (NoBlankBinaryCTC.py:139-151).
    Optional 5th argument ``batch_total``: global batch size when this call sees only a
    shard (loss and gradient are scaled by 1/batch_total; see ctc_amd.distributed).

    ``apply`` hands canonical arguments to the C++ autograd node of csrc/autograd_ext.cpp (same launches, less host
    time per eager step); anything else -- and every error -- takes the Python Function below.
    """

    @classmethod
    def apply(cls, log_probs, targets, input_lengths, target_lengths, batch_total=None):
        out = _fast_apply(log_probs, targets, input_lengths, target_lengths, batch_total)
        if out is not None:
            return out[0]
        return super().apply(log_probs, targets, input_lengths, target_lengths, batch_total)

    @staticmethod
    def forward(ctx, log_probs, targets, input_lengths, target_lengths, batch_total=None):
        variant = _variant_of(targets)
        want = ctx.needs_input_grad[0]
        loss, nll, grad = _launch(variant, log_probs, targets, input_lengths, target_lengths, want,
                                  batch_total)
        ctx.grad = grad
        ctx.meta = (variant, batch_total, 0, None)
        if want:
            ctx.save_for_backward(log_probs, targets)
            ctx.lens = (input_lengths, target_lengths)
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gout):
        return _scaled_grad(ctx, gout), None, None, None, None


def noblank_ctc_loss(logits, targets, input_lengths, target_lengths, batch_total=None, label_smoothing=None):
    """-> (loss, nll[B]); NoBlankCTC arithmetic.

    ``label_smoothing=lam`` selects the emission variant sketched in comments at NoBlankCTC.py:100-107 (the
    true class weighted lam, every other class (1 - lam) / C); None = the module as shipped.  lam in [0, 1]; shapes of
    the four-rows-per-wave kernel only (C even <= 256, S <= 31, T <= 168), fp32 / bf16 / fp16 logits.  lam = 1 is the
    plain call bit for bit.  Every logit of a frame enters every emission of that frame, e = a lp[c_l] + b sum_n lp[n]
    with b = (1 - lam) / C, a = lam - b: a sample with a -inf logit anywhere in a live frame, or with pad logits (-1e30)
    whose sum alone carries nll to 1e12, has no alignment -- nll >= 1e12 (possibly +inf, never NaN), all of its gradient
    rows exactly 0, and the batch loss is the mean of the nll as reported.  lam <= 1 / (C + 1) (a <= 0) is defined on
    finite logits only."""
    if label_smoothing is None:
        out = _fast_apply(logits, targets, input_lengths, target_lengths, batch_total, _lib.NOBLANK)
        if out is not None:
            return out[0], out[1]
    return _LossFn.apply(logits, targets, input_lengths, target_lengths, _lib.NOBLANK, batch_total, 0,
                         label_smoothing)


def binary_ctc_loss(logits, targets, input_lengths, target_lengths, batch_total=None):
    """-> (loss, nll[B]); NoBlankBinaryCTC arithmetic."""
    out = _fast_apply(logits, targets, input_lengths, target_lengths, batch_total, _lib.BINARY)
    if out is not None:
        return out[0], out[1]
    return _LossFn.apply(logits, targets, input_lengths, target_lengths, _lib.BINARY, batch_total, 0)


def blank_ctc_loss(log_probs, targets, input_lengths, target_lengths, blank=0, batch_total=None):
    """-> (loss, nll[B]); torch.nn.CTCLoss(blank, reduction='mean', zero_infinity=False)
    semantics (models/layers/AsyncTFCriterion.py:198): log_probs are normalised
    log-probabilities, loss = mean_b(nll_b / max(L_b,1)).  ``targets`` [B,S] with S <= 1023 label columns
    (CtcAmdError beyond); more than 255 columns take the wide lattice path of the library (several waves per chain).
    ``blank_best_path`` / ``blank_forced_align`` and ``blank_posteriors`` take the same widths.

    ``-inf`` log-probs are allowed (a masked vocabulary); the gradient at a ``-inf`` entry is exactly 0.  A sample with
    no alignment -- through its lengths (``T_b < L_b + adjacent repeats``) or through its emissions (every path crosses
    a ``-inf`` entry) -- has ``nll = +inf`` like torch and an all-zero gradient where torch gives NaN; ``loss`` is then
    ``+inf`` and the gradients of the other samples are what they would be without it."""
    return _LossFn.apply(log_probs, targets, input_lengths, target_lengths, _lib.BLANK, batch_total, blank)


def _readout_inputs(x, name, targets, in_len, tgt_len, variant):
    """What the read-outs (best path, posteriors, token spans) do before their launch -> (xs, tg, il, tl, T, B, C, S, dev):
    logits [T,B,C] on a HIP device, detached and with unit class stride -- float32, or for the no-blank and binary variants
    also bfloat16 / float16, kept in their own dtype (a copy for the class stride included); targets of `variant` and int64
    lengths on that device.  The blank read-outs refuse empty shapes here (target lengths may be 0); the no-blank and binary
    ones leave that to the library, which answers with its own error."""
    blank = variant == _lib.BLANK
    _require_hip(x, name)
    if x.dim() != 3 or (x.dtype != torch.float32 and (blank or x.dtype not in _LOWP_CODE)):
        raise ValueError("ctc_amd: %s must be float32 [T,B,C]" % name if blank else
                         "ctc_amd: %s must be float32, bfloat16 or float16 [T,B,C]" % name)
    T, B, C = x.shape
    if blank and (T < 1 or B < 1 or C < 1):
        raise ValueError("ctc_amd: empty %s %s" % (name, tuple(x.shape)))
    dev = x.device
    xs = x.detach()
    if xs.stride(2) != 1:
        xs = xs.contiguous()
    if variant == _lib.BINARY:
        if _variant_of(targets) != _lib.BINARY or targets.shape[0] != B or targets.shape[2] != C:
            raise ValueError("ctc_amd: targets must be [B,S,C] float")
        tg = _placed(targets, dev, torch.float32)
    else:
        if (blank and not isinstance(targets, torch.Tensor)) or _variant_of(targets) != _lib.NOBLANK \
                or targets.shape[0] != B:
            raise ValueError("ctc_amd: targets must be [B,S] integer")
        if targets.dtype not in (torch.int32, torch.int64):
            targets = targets.long()
        tg = _placed(targets, dev)
    S = tg.shape[1]
    if blank and S < 1:
        raise ValueError("ctc_amd: targets need at least one label column")
    il = _lengths(in_len, B, "input_lengths", dev, T)
    tl = _lengths(tgt_len, B, "target_lengths", dev, S, lo=0 if blank else 1)
    return xs, tg, il, tl, T, B, C, S, dev


def _logits_call(entry, xs, rest, fallback=False):
    """The C-ABI call `entry`(x, stride_t, stride_b, *rest) on the logits `xs` -> its return code.  float32 logits go to
    `entry`.  bfloat16 / float16 logits go to `entry + "_typed"` as they lie (no fp32 image, no cast launch); `fallback`:
    when that entry answers UNSUPPORTED_SHAPE -- only ctc_amd_noblank_posteriors_typed has a narrower domain than its
    sibling -- and for a 2-byte dtype that `_LOWP_READOUT` does not hold, the cast and the untyped entry, which then
    answers as it does for float32 input, its own error included."""
    lib = _lib.load()
    code = _LOWP_READOUT.get(xs.dtype)
    if code is not None:
        rc = getattr(lib, entry + "_typed")(xs.data_ptr(), code, xs.stride(0), xs.stride(1), *rest)
        if rc != _lib.ERR_UNSUPPORTED_SHAPE or not fallback:
            return rc
    if xs.dtype is not torch.float32:
        xs = xs.float()                                      # (keeps the unit class stride)
    return getattr(lib, entry)(xs.data_ptr(), xs.stride(0), xs.stride(1), *rest)


def _readout(entry, variant, x, name, targets, in_len, tgt_len, width, out_dtype, extra=(), workspace=True, fallback=False):
    """One read-out launch -> (out[B,T,width] or out[B,T] of out_dtype, per_sample[B] fp32).  `entry`: the C-ABI call
    (x, strides, targets[, labels_i64], lengths, T, B, C, S, *extra, per-sample or main output as the header orders
    them, workspace, stream), its `_typed` sibling for 2-byte logits (`_logits_call`); `width(S)`: last dimension of the
    main output, None for [B,T]."""
    xs, tg, il, tl, T, B, C, S, dev = _readout_inputs(x, name, targets, in_len, tgt_len, variant)
    w = width(S) if width else None
    out = torch.empty((B, T) if w is None else (B, T, w), dtype=out_dtype, device=dev)
    per = torch.empty(B, dtype=torch.float32, device=dev)
    lab = () if variant == _lib.BINARY else (int(tg.dtype is torch.int64),)
    # best paths: (path, score); posteriors: (nll, gamma)
    outs = (out.data_ptr(), per.data_ptr()) if w is None else (per.data_ptr(), out.data_ptr())
    with _on_device(dev):
        stream = _stream_handle(dev)
        ws = _workspace(variant, T, B, C, S, dev, stream).data_ptr() if workspace else None
        rc = _logits_call(entry, xs, (tg.data_ptr(), *lab, il.data_ptr(), tl.data_ptr(), T, B, C, S, *extra, *outs, ws,
                                      stream), fallback)
    _lib.check(rc, entry)
    if variant == _lib.BLANK and _VALIDATE:
        check_status(dev)
    return out, per


def noblank_best_path(logits, targets, input_lengths, target_lengths):
    """Best (Viterbi) alignment on the no-blank lattice -> (path[B,T] int32, score[B]).

    ``path[b,t]`` is the label POSITION l_t (index into targets[b]) occupied at step t, -1 for
    ``t >= T_b`` or when no alignment exists; ``score[b]`` its log-probability.  Max-semiring
    twin of the loss recursion (NoBlankCTC.py:71-87); SURVEY 8(f) rank 1.

    ``logits``: float32, bfloat16 or float16 logits [T,B,C].  2-byte logits are read as they lie
    (``ctc_amd_noblank_best_path_typed``: no fp32 copy, any shape the float32 call takes); path and score are bit for bit
    those of the call on ``logits.float()``.
    """
    return _readout("ctc_amd_noblank_best_path", _lib.NOBLANK, logits, "logits", targets, input_lengths, target_lengths,
                    None, torch.int32, workspace=False)


def binary_best_path(logits, targets, input_lengths, target_lengths):
    """Best (Viterbi) alignment on the lattice of the binary variant -> (path[B,T] int32, score[B]); ``targets`` [B,S,C]
    float label rows, ``path[b,t]`` the label ROW occupied at step t (-1 for ``t >= T_b`` or when no alignment exists).
    Max-semiring twin of NoBlankBinaryCTC's recursion (NoBlankBinaryCTC.py:72-95); SURVEY 8(f) rank 1.  float32, bfloat16
    or float16 logits: 2-byte logits are read as they lie (``ctc_amd_binary_best_path_typed``), with the bits of the call on
    ``logits.float()``."""
    return _readout("ctc_amd_binary_best_path", _lib.BINARY, logits, "logits", targets, input_lengths, target_lengths,
                    None, torch.int32, workspace=False)


def blank_best_path(log_probs, targets, input_lengths, target_lengths, blank=0):
    """Best (Viterbi) alignment on the blank-CTC lattice -> (path[B,T] int32, score[B] fp32).

    Same inputs as ``blank_ctc_loss``: ``log_probs`` [T,B,C] normalised log-probabilities (used as given),
    ``targets`` [B,S] int32/int64.  ``path[b,t]`` is the extended-label STATE s_t (even = blank, odd s = label
    (s-1)//2 of targets[b]) for ``t < T_b``, -1 beyond ``T_b`` and for samples with no alignment; ``score[b]`` the
    log-probability of that alignment (-inf when none exists).  S <= 1023 label columns, as the loss and
    ``blank_posteriors`` (CtcAmdError beyond): up to 255 columns ctc_amd_blank_best_path runs, 256..1023 take ctc_amd_blank_best_path_wide (several
    waves per sample; the same arithmetic, the same bits for a sample whichever entry serves it).  include/ctc_amd.h.
    """
    S = targets.shape[1] if isinstance(targets, torch.Tensor) and targets.dim() == 2 else 0   # (_readout validates)
    if S > BLANK_MAX_LABELS:
        raise _lib.CtcAmdError(
            "ctc_amd: the blank CTC best path takes targets of at most %d label columns (2S+1 <= %d lattice states), "
            "got S=%d" % (BLANK_MAX_LABELS, 2 * BLANK_MAX_LABELS + 1, S))
    entry = "ctc_amd_blank_best_path_wide" if S > BLANK_NARROW_LABELS else "ctc_amd_blank_best_path"
    return _readout(entry, _lib.BLANK, log_probs, "log_probs", targets, input_lengths,
                    target_lengths, None, torch.int32, extra=(int(blank),))


def blank_forced_align(log_probs, targets, input_lengths, target_lengths, blank=0):
    """Forced alignment of known targets (the batched form of torchaudio-style ``forced_align``) ->
    (tokens[B,T] int64, frame_scores[B,T] fp32).

    ``tokens[b,t]`` is the class of the best path's state at frame t (``blank`` or the target label), -1 beyond
    ``T_b`` / without an alignment; ``frame_scores[b,t] = log_probs[t,b,tokens[b,t]]`` (0 where tokens is -1), so
    that their sum over t in order is ``blank_best_path``'s score.  Derived on the device from the path, so S <= 1023
    label columns as there and as the loss."""
    path, _ = blank_best_path(log_probs, targets, input_lengths, target_lengths, blank)
    dev = path.device
    tg = targets.to(device=dev, dtype=torch.int64)
    valid = path >= 0
    st = path.long().clamp(min=0)
    lab = torch.gather(tg, 1, ((st - 1) >> 1).clamp(0, tg.shape[1] - 1))
    tokens = torch.where((st & 1) == 1, lab, torch.full_like(lab, int(blank)))
    tokens = torch.where(valid, tokens, torch.full_like(tokens, -1))
    lp = log_probs.detach().transpose(0, 1)                                   # [B,T,C] view
    fs = torch.gather(lp, 2, tokens.clamp(min=0).unsqueeze(2)).squeeze(2)
    frame_scores = torch.where(valid, fs, torch.zeros_like(fs))
    return tokens, frame_scores


def blank_posteriors(log_probs, targets, input_lengths, target_lengths, blank=0):
    """Per-frame state posteriors of the blank-CTC lattice -> (gamma[B,T,2S+1] fp32, nll[B] fp32).

    Same inputs as ``blank_best_path``.  ``gamma[b,t,s]`` = P(extended-label state s at frame t | log_probs, targets)
    (even s = blank, odd s = label (s-1)//2 of targets[b]); rows sum to 1 for ``t < T_b``, and are 0 for ``t >= T_b``,
    for ``s > 2 L_b`` and for samples with no alignment (``nll`` +inf, as ``blank_ctc_loss`` reports it).  Not
    differentiable.  ``gamma[b, t, path[b, t]]`` with ``blank_best_path``'s path is the confidence of each aligned
    frame.  S <= 1023 label columns, as the loss and ``blank_best_path`` (CtcAmdError beyond): up to 255 columns
    ctc_amd_blank_posteriors runs, 256..1023 take ctc_amd_blank_posteriors_wide (several waves per chain, one
    rescaling for all of them).  include/ctc_amd.h.
    """
    S = targets.shape[1] if isinstance(targets, torch.Tensor) and targets.dim() == 2 else 0   # (_readout validates)
    if S > BLANK_MAX_LABELS:
        raise _lib.CtcAmdError(
            "ctc_amd: the blank CTC posteriors take targets of at most %d label columns (2S+1 <= %d lattice states), "
            "got S=%d" % (BLANK_MAX_LABELS, 2 * BLANK_MAX_LABELS + 1, S))
    entry = "ctc_amd_blank_posteriors_wide" if S > BLANK_NARROW_LABELS else "ctc_amd_blank_posteriors"
    return _readout(entry, _lib.BLANK, log_probs, "log_probs", targets, input_lengths,
                    target_lengths, lambda S: 2 * S + 1, torch.float32, extra=(int(blank),))


class BlankTokenSpans(NamedTuple):
    """What ``blank_token_spans`` returns (shapes and meanings: its docstring)."""
    start: torch.Tensor
    end: torch.Tensor
    conf: torch.Tensor
    frame_conf: torch.Tensor
    path: torch.Tensor
    score: torch.Tensor
    nll: torch.Tensor


def blank_token_spans(log_probs, targets, input_lengths, target_lengths, blank=0):
    """One record per target label from the best alignment and the posteriors of the blank-CTC lattice, in one call ->
    ``BlankTokenSpans(start, end, conf, frame_conf, path, score, nll)``.

    Same inputs as ``blank_best_path``.  For label j < L_b of a sample that has an alignment, ``start[b,j]`` [B,S] int32 is
    the first frame the best path gives to that label and ``end[b,j]`` one past the last (the frames between are all
    its own); ``conf[b,j]`` [B,S] fp32 is the mean over those frames of ``frame_conf``.  The class of span j is
    ``targets[b,j]``.  Padding columns j >= L_b and samples without an alignment have start = end = -1 and conf = 0.
    ``frame_conf[b,t]`` [B,T] fp32 is the posterior of the best path's state at frame t, ``gamma[b,t,path[b,t]]`` of
    ``blank_posteriors`` bit for bit (0 where path is -1) -- but gamma [B,T,2S+1] itself is never allocated or written.
    ``path`` [B,T] int32 and ``score`` [B] are ``blank_best_path``'s, ``nll`` [B] is ``blank_posteriors``', bit for bit.
    conf is a float32 sum over the span in ascending t followed by one division, so a float32 loop reproduces it.
    Not differentiable.  S <= 1023 label columns, as the other blank read-outs (CtcAmdError beyond).
    ``blank_forced_align`` stays the frame-level form (a token and its log-probability per frame).  include/ctc_amd.h.
    """
    S = targets.shape[1] if isinstance(targets, torch.Tensor) and targets.dim() == 2 else 0   # (_readout_inputs validates)
    if S > BLANK_MAX_LABELS:
        raise _lib.CtcAmdError(
            "ctc_amd: the blank CTC token spans take targets of at most %d label columns (2S+1 <= %d lattice states), "
            "got S=%d" % (BLANK_MAX_LABELS, 2 * BLANK_MAX_LABELS + 1, S))
    xs, tg, il, tl, T, B, C, S, dev = _readout_inputs(log_probs, "log_probs", targets, input_lengths, target_lengths,
                                                      _lib.BLANK)
    path = torch.empty((B, T), dtype=torch.int32, device=dev)
    frame_conf = torch.empty((B, T), dtype=torch.float32, device=dev)
    start = torch.empty((B, S), dtype=torch.int32, device=dev)
    end = torch.empty((B, S), dtype=torch.int32, device=dev)
    conf = torch.empty((B, S), dtype=torch.float32, device=dev)
    score = torch.empty(B, dtype=torch.float32, device=dev)
    nll = torch.empty(B, dtype=torch.float32, device=dev)
    with _on_device(dev):
        stream = _stream_handle(dev)
        ws = _workspace(_lib.BLANK, T, B, C, S, dev, stream)
        rc = _lib.load().ctc_amd_blank_token_spans(
            xs.data_ptr(), xs.stride(0), xs.stride(1), tg.data_ptr(), int(tg.dtype is torch.int64), il.data_ptr(),
            tl.data_ptr(), T, B, C, S, int(blank), path.data_ptr(), score.data_ptr(), nll.data_ptr(),
            frame_conf.data_ptr(), start.data_ptr(), end.data_ptr(), conf.data_ptr(), ws.data_ptr(), stream)
    _lib.check(rc, "ctc_amd_blank_token_spans")
    if _VALIDATE:
        check_status(dev)
    return BlankTokenSpans(start, end, conf, frame_conf, path, score, nll)


class TokenSpans(NamedTuple):
    """What ``noblank_token_spans`` / ``binary_token_spans`` return (shapes and meanings: their docstrings)."""
    start: torch.Tensor
    end: torch.Tensor
    conf: torch.Tensor
    frame_conf: torch.Tensor
    path: torch.Tensor
    score: torch.Tensor
    nll: torch.Tensor


TOKEN_SPANS_MAX_LABELS = 256       # ctc_amd_noblank_token_spans / ctc_amd_binary_token_spans: S <= 256
TOKEN_SPANS_LDS_BYTES = 160 * 1024


def _token_spans(entry, variant, logits, targets, in_len, tgt_len):
    xs, tg, il, tl, T, B, C, S, dev = _readout_inputs(logits, "logits", targets, in_len, tgt_len, variant)
    path = torch.empty((B, T), dtype=torch.int32, device=dev)
    frame_conf = torch.empty((B, T), dtype=torch.float32, device=dev)
    start = torch.empty((B, S), dtype=torch.int32, device=dev)
    end = torch.empty((B, S), dtype=torch.int32, device=dev)
    conf = torch.empty((B, S), dtype=torch.float32, device=dev)
    score = torch.empty(B, dtype=torch.float32, device=dev)
    nll = torch.empty(B, dtype=torch.float32, device=dev)
    lab = () if variant == _lib.BINARY else (int(tg.dtype is torch.int64),)
    with _on_device(dev):
        rc = _logits_call(entry, xs, (
            tg.data_ptr(), *lab, il.data_ptr(), tl.data_ptr(), T, B, C, S,
            path.data_ptr(), score.data_ptr(), nll.data_ptr(), frame_conf.data_ptr(), start.data_ptr(), end.data_ptr(),
            conf.data_ptr(), None, _stream_handle(dev)))
    if rc == _lib.ERR_UNSUPPORTED_SHAPE:
        raise _lib.CtcAmdError(
            "ctc_amd: %s holds a sample's lattice in LDS: S <= %d label columns and about 13 bytes per cell of T x S "
            "(emissions, alpha, beta' and a back-pointer byte%s) within %d bytes -- T = 150 at S <= 64; got T=%d, S=%d, "
            "C=%d" % (entry, TOKEN_SPANS_MAX_LABELS, ", plus 64 C bytes of row buffers" if variant == _lib.BINARY else "",
                      TOKEN_SPANS_LDS_BYTES, T, S, C))
    _lib.check(rc, entry)
    return TokenSpans(start, end, conf, frame_conf, path, score, nll)


def noblank_token_spans(logits, targets, input_lengths, target_lengths):
    """The segmentation of a clip by its transcript on the no-blank lattice, in one launch ->
    ``TokenSpans(start, end, conf, frame_conf, path, score, nll)``.

    Same inputs as ``noblank_best_path``: float32, bfloat16 or float16 logits [T,B,C] on a HIP device (any batch / time
    strides; 2-byte logits are read as they lie by ``ctc_amd_noblank_token_spans_typed`` -- the same shapes, and every output
    bit for bit that of the call on ``logits.float()``), ``targets``
    [B,S] int32 / int64 (negative labels inside L_b wrap as there), lengths on the host or on the device.  For sample b
    with T_b frames and L_b labels:

    * ``path`` [B,T] int32 and ``score`` [B] are ``noblank_best_path``'s, bit for bit: the label position per frame, -1
      for ``t >= T_b``; -1 / -inf for a sample without an alignment.
    * ``nll`` [B] is ``-alpha[T_b-1, L_b-1]`` of the lattice; ``+inf`` for a sample without an alignment (``L_b > T_b``
      or lengths outside the tensor) -- the loss itself reports the reference's sentinel magnitude (1e13) there.
    * ``frame_conf`` [B,T] fp32 is the posterior of the state the best path occupies, ``gamma_t(path_t)`` with gamma
      normalised per row as in ``noblank_posteriors``; 0 where ``path`` is -1.  gamma [B,T,S] itself is never written.
    * ``start``, ``end`` [B,S] int32: label j owns the frames ``start[b,j] .. end[b,j]-1``.  Every label j < L_b of an
      aligned sample owns at least one frame and the spans partition ``[0, T_b)``: ``start[b,0] == 0``, ``end[b,j] ==
      start[b,j+1]``, ``end[b,L_b-1] == T_b``.  Columns j >= L_b and samples without an alignment get -1 / -1.
    * ``conf`` [B,S] fp32: the float32 sum of ``frame_conf`` over the span, from 0 in ascending t, then one float32
      division by ``float(end - start)``; 0 where start is -1.  A float32 loop over ``path`` and ``frame_conf`` reproduces
      it bit for bit (the rule of ``blank_token_spans``).

    The class of span j is ``targets[b,j]``.  Not differentiable; no CPU path.  One workgroup per sample keeps the
    lattice in LDS: S <= 256, and ``((3T + 8) SP + 2T + 3 SP + 8) * 4 + T * SP + 16`` bytes (SP = S rounded up to a
    multiple of 1, 2, 4 for S <= 64, 128, 256: 13 bytes per lattice cell) within 160 KB -- T = 150 at every S <= 64;
    ``CtcAmdError`` beyond.  include/ctc_amd.h, DESIGN.md 3.10.
    """
    return _token_spans("ctc_amd_noblank_token_spans", _lib.NOBLANK, logits, targets, input_lengths, target_lengths)


def binary_token_spans(logits, targets, input_lengths, target_lengths):
    """``noblank_token_spans`` on the lattice of the binary variant -> ``TokenSpans``: ``targets`` [B,S,C] float label
    rows as in ``binary_best_path``, whose ``path`` / ``score`` these are bit for bit; the class of span j is row j of
    the targets.  float32, bfloat16 or float16 logits, 2-byte ones read as they lie (``ctc_amd_binary_token_spans_typed``)
    with the bits of the call on ``logits.float()``.  ``nll`` is ``+inf`` for a sample without an alignment (the loss itself reports the reference's sentinel
    magnitude there).  LDS bound: ``((3T + 8) SP + 2T + 2 SP + 16 C + 8) * 4 + T * SP + 16`` bytes within 160 KB (S <=
    256; T = 150 at every S <= 64 and C <= 256 -- not ``binary_posteriors``' T <= 168, S <= 64, C <= 256);
    ``CtcAmdError`` beyond."""
    return _token_spans("ctc_amd_binary_token_spans", _lib.BINARY, logits, targets, input_lengths, target_lengths)


def noblank_posteriors(logits, targets, input_lengths, target_lengths):
    """Per-step state posteriors of the no-blank lattice -> (gamma[B,T,S], nll[B]).

    ``gamma[b,t,l]`` = P(label position l at step t | logits, targets): the soft alignment whose
    class-scatter is the loss gradient; rows sum to 1 for ``t < T_b``.  SURVEY 8(f) rank 1.

    ``logits``: float32, bfloat16 or float16 logits [T,B,C].  2-byte logits are read as they lie
    (``ctc_amd_noblank_posteriors_typed``) inside the reduced-precision domain of the no-blank loss -- C even <= 256,
    S <= 31, T <= 168, even strides, 4-byte aligned rows; outside it they are cast with ``.float()`` and take the float32
    entry.  Either way gamma and nll are bit for bit those of the call on ``logits.float()``.
    """
    return _readout("ctc_amd_noblank_posteriors", _lib.NOBLANK, logits, "logits", targets, input_lengths,
                    target_lengths, lambda S: S, torch.float32, fallback=True)


def binary_posteriors(logits, targets, input_lengths, target_lengths):
    """Per-step posteriors of the binary (multi-hot) lattice -> (gamma[B,T,S], nll[B]): ``gamma[b,t,l]`` =
    P(target row l at step t | logits, targets), rows sum to 1 for ``t < T_b``.  SURVEY 8(f) rank 1, the sibling of
    ``noblank_posteriors``; shapes of the pipelined binary kernel (S <= 64, T <= 168, C <= 256).  float32, bfloat16 or
    float16 logits: 2-byte logits are read as they lie (``ctc_amd_binary_posteriors_typed``, the same shapes), with the bits
    of the call on ``logits.float()``."""
    return _readout("ctc_amd_binary_posteriors", _lib.BINARY, logits, "logits", targets, input_lengths,
                    target_lengths, lambda S: S, torch.float32)


def dedup_multihot_targets(rows, exact_rows=False):
    """Target construction on the device (datasets/charades_ctc_next_pred.py:646-651,663-678).

    ``rows`` [B,S,C] integer multi-hot label rows (one row per annotated time step of a clip) ->
    ``(targets [B,S,C] int32, lengths [B] int64)``: the rows whose code is new, in order of first
    appearance, padded with rows of -1 (the block the reference stores as ``o_only_target`` /
    ``o_target_length``).  ``targets.clamp(min=0).float()`` is the [B,S,C] float input of NoBlankBinaryCTC.

    Default (``exact_rows=False``): the reference's own comparison -- the int32 code ``sum_o row[o] * 2**o``
    as torch accumulates it into an IntTensor (class 31 is the sign bit, classes 32..63 drop out, code 0
    never enters); bit-exact with the reference at its default 38 / 33 classes (opts.py:60-61).  With more
    than 64 classes the reference raises OverflowError (``2**64``), and so does this.  ``exact_rows=True``
    compares whole rows instead (any C)."""
    _require_hip(rows, "rows")
    if rows.dim() != 3 or rows.dtype.is_floating_point:
        raise ValueError("ctc_amd: rows must be an integer tensor [B,S,C], got %s %s" % (tuple(rows.shape), rows.dtype))
    B, S, C = rows.shape
    if B < 1 or S < 1 or C < 1:
        raise ValueError("ctc_amd: empty rows %s" % (tuple(rows.shape),))
    if not exact_rows and C > 64:
        raise OverflowError("ctc_amd: int too big to convert -- the reference's row code 2**o does not exist for "
                            "class o >= 64 (C = %d); pass exact_rows=True" % C)
    r = rows if rows.dtype is torch.int32 and rows.is_contiguous() else rows.to(torch.int32).contiguous()
    out = torch.empty_like(r)
    length = torch.empty(B, dtype=torch.int64, device=r.device)
    with _on_device(r.device):
        rc = _lib.load().ctc_amd_dedup_multihot_targets(r.data_ptr(), B, S, C, int(bool(exact_rows)), out.data_ptr(),
                                                        length.data_ptr(), _stream_handle(r.device))
    if rc:
        _lib.check(rc, "ctc_amd_dedup_multihot_targets")
    return out, length


class CollapsedTokens(NamedTuple):
    """What ``collapse_frames`` returns (shapes and meanings: its docstring)."""
    tokens: torch.Tensor
    lengths: torch.Tensor
    start: torch.Tensor
    end: torch.Tensor
    conf: torch.Tensor


EDIT_DISTANCE_MAX_REF = 1023       # ctc_amd_edit_distance: M <= 1023, the one limit on target widths (BLANK_MAX_LABELS)


def _eval_labels(t, name, batch=None):
    """a [B,*] int32 / int64 tensor on a HIP device, or ValueError (rank, dtype, device, batch size)"""
    if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.dtype not in (torch.int32, torch.int64):
        raise ValueError("ctc_amd: %s must be an int32 or int64 tensor of rank 2" % name)
    if not t.is_cuda:
        raise ValueError("ctc_amd: %s must be on a HIP (cuda) device -- the engine has no CPU path" % name)
    if batch is not None and t.shape[0] != batch:
        raise ValueError("ctc_amd: %s has %d rows, the batch has %d" % (name, t.shape[0], batch))
    return t.detach()


def collapse_frames(frames, input_lengths, blank=None, frame_conf=None, max_tokens=None):
    """Per-frame decisions to tokens with frame spans, on the device -> ``CollapsedTokens(tokens, lengths, start, end,
    conf)``: maximal runs of equal labels are merged and the runs of ``blank`` dropped.

    ``frames`` [B,T] int32 / int64 on a HIP device, any strides (the ``.t()`` view of a [T,B] tensor takes no copy): the
    greedy decision ``logits.argmax(-1).t()``, the classes along ``blank_best_path``'s path, or the per-frame label
    positions of ``noblank_best_path`` / ``binary_best_path``.  ``input_lengths`` [B], 0 <= T_b <= T; frames at ``t >=
    T_b`` are never read.  ``blank``: the class that separates tokens (``a, blank, a`` gives two tokens, ``a, a`` one);
    ``None``: no blank -- every run is a token, a run of -1 included (the decode of the no-blank and binary lattices).

    * ``tokens`` [B,W] int32, W = ``max_tokens`` (default T): the label of each run; ``lengths`` [B] int64 their number --
      the true count even where it exceeds W, so a truncation shows.
    * ``start``, ``end`` [B,W] int32: first and last frame of the run, both inclusive.
    * ``conf`` [B,W] fp32 when ``frame_conf`` [B,T] fp32 is given (else ``None``): the float32 sum of ``frame_conf`` over
      the run in ascending t, then one float32 division by the frame count -- a float32 loop reproduces the bits.

    Columns at and beyond ``lengths[b]`` hold -1 / -1 / -1 / 0.  int64 labels are read through their low 32 bits.  One
    launch, no host synchronisation, capture-safe.  include/ctc_amd.h, DESIGN.md 3.12."""
    fr = _eval_labels(frames, "frames")
    B, T = fr.shape
    dev = fr.device
    W = T if max_tokens is None else int(max_tokens)
    if T < 1 or B < 1 or W < 1:
        raise ValueError("ctc_amd: collapse_frames needs B, T and max_tokens >= 1, got B=%d, T=%d, max_tokens=%d" % (B, T, W))
    fc = None
    if frame_conf is not None:
        if not isinstance(frame_conf, torch.Tensor) or frame_conf.dtype != torch.float32 \
                or tuple(frame_conf.shape) != (B, T):
            raise ValueError("ctc_amd: frame_conf must be float32 [B,T] = [%d,%d]" % (B, T))
        if frame_conf.device != dev:
            raise ValueError("ctc_amd: frame_conf must be on the device of frames")
        fc = frame_conf.detach()
    il = _lengths(input_lengths, B, "input_lengths", dev, T, lo=0)
    tokens = torch.empty((B, W), dtype=torch.int32, device=dev)
    start = torch.empty((B, W), dtype=torch.int32, device=dev)
    end = torch.empty((B, W), dtype=torch.int32, device=dev)
    conf = torch.empty((B, W), dtype=torch.float32, device=dev) if fc is not None else None
    lengths = torch.empty(B, dtype=torch.int64, device=dev)
    with _on_device(dev):
        rc = _lib.load().ctc_amd_collapse_frames(
            fr.data_ptr(), int(fr.dtype is torch.int64), fr.stride(0), fr.stride(1), il.data_ptr(),
            None if fc is None else fc.data_ptr(), 0 if fc is None else fc.stride(0), 0 if fc is None else fc.stride(1),
            T, B, -1 if blank is None else int(blank), W, tokens.data_ptr(), lengths.data_ptr(), start.data_ptr(),
            end.data_ptr(), None if conf is None else conf.data_ptr(), _stream_handle(dev))
    _lib.check(rc, "ctc_amd_collapse_frames")
    return CollapsedTokens(tokens, lengths, start, end, conf)


def edit_distance(hyp, hyp_lengths, ref, ref_lengths):
    """Levenshtein distance (unit costs) between ``hyp[b,:hyp_lengths[b]]`` and ``ref[b,:ref_lengths[b]]`` -> ``dist``
    [B] int32, on the device.  ``hyp`` [B,N], ``ref`` [B,M] int32 / int64 on a HIP device (the two dtypes may differ; any
    batch stride, so a row slice of a wider tensor takes no copy); lengths may be 0 and elements beyond a length are never
    read.  M <= 1023, the limit on target widths everywhere here (``CtcAmdError`` beyond); any N.  Exact; one launch, no
    host synchronisation, capture-safe.  include/ctc_amd.h, DESIGN.md 3.12."""
    h = _eval_labels(hyp, "hyp")
    B, N = h.shape
    r = _eval_labels(ref, "ref", B)
    M = r.shape[1]
    dev = h.device
    if r.device != dev:
        raise ValueError("ctc_amd: hyp and ref must be on the same device")
    if B < 1:
        raise ValueError("ctc_amd: edit_distance needs B >= 1")
    if N > 1 and h.stride(1) != 1:
        h = h.contiguous()
    if M > 1 and r.stride(1) != 1:
        r = r.contiguous()
    hl = _lengths(hyp_lengths, B, "hyp_lengths", dev, N, lo=0)
    rl = _lengths(ref_lengths, B, "ref_lengths", dev, M, lo=0)
    dist = torch.empty(B, dtype=torch.int32, device=dev)
    with _on_device(dev):
        rc = _lib.load().ctc_amd_edit_distance(
            h.data_ptr() if N else None, int(h.dtype is torch.int64), h.stride(0), hl.data_ptr(),
            r.data_ptr() if M else None, int(r.dtype is torch.int64), r.stride(0), rl.data_ptr(),
            B, N, M, dist.data_ptr(), _stream_handle(dev))
    _lib.check(rc, "ctc_amd_edit_distance")
    return dist


def label_error_rate(hyp, hyp_lengths, ref, ref_lengths):
    """The standard CTC metric -> ``(ler, dist)``: ``dist`` [B] int32 is ``edit_distance``'s, ``ler = sum(dist) /
    max(sum(ref_lengths), 1)`` a 0-dim float32 tensor on the device (the sums are integer; no host synchronisation)."""
    dist = edit_distance(hyp, hyp_lengths, ref, ref_lengths)
    rl = _lengths(ref_lengths, dist.shape[0], "ref_lengths", dist.device, ref.shape[1], lo=0)
    ler = dist.sum(dtype=torch.int64).to(torch.float32) / rl.sum().clamp(min=1).to(torch.float32)
    return ler, dist


class BeamHypotheses(NamedTuple):
    """What ``blank_beam_search`` / ``noblank_beam_search`` return (shapes and meanings: their docstrings)."""
    tokens: torch.Tensor
    lengths: torch.Tensor
    scores: torch.Tensor
    count: torch.Tensor


class FusedBeamHypotheses(NamedTuple):
    """What ``blank_beam_search`` / ``noblank_beam_search`` return when a table ``lm`` is given: ``scores`` is the fused
    score the hypotheses are ordered by, ``ctc_scores`` the acoustic log-probability alone."""
    tokens: torch.Tensor
    lengths: torch.Tensor
    scores: torch.Tensor
    count: torch.Tensor
    ctc_scores: torch.Tensor


BEAM_MAX_WIDTH = 64                # ctc_amd_beam_search: 1 <= nbest <= beam_width <= 64
BEAM_MAX_CLASSES = 32              # ... and 1 <= top_classes <= 32


def _beam_lm_table(lm, C, dev):
    """the bigram table as the library is given it: float32 [C+1, C] on `dev`, unit column stride, row stride >= C (such a
    view is passed as it lies, any other is made contiguous)"""
    if not isinstance(lm, torch.Tensor) or lm.dtype != torch.float32 or tuple(lm.shape) != (C + 1, C):
        raise ValueError("ctc_amd: lm must be a float32 tensor [C+1, C] = [%d, %d], got %s" % (
            C + 1, C, "%s %s" % (lm.dtype, tuple(lm.shape)) if isinstance(lm, torch.Tensor) else type(lm).__name__))
    if lm.device != dev:
        raise ValueError("ctc_amd: lm must be on the logits' device %s, got %s" % (dev, lm.device))
    lm = lm.detach()
    if lm.stride(1) != 1 or lm.stride(0) < C:
        lm = lm.contiguous()
    return lm


def _beam_search(x, name, input_lengths, beam_width, nbest, top_classes, blank, max_tokens, lm=None, lm_weight=1.0,
                 token_bonus=0.0):
    if not isinstance(x, torch.Tensor) or x.dim() != 3 or x.dtype != torch.float32:
        raise ValueError("ctc_amd: %s must be a float32 tensor [T,B,C]" % name)
    T, B, C = x.shape
    W, N, K = int(beam_width), int(nbest), int(top_classes)
    L = T if max_tokens is None else int(max_tokens)
    if T < 1 or B < 1 or C < 2:
        raise ValueError("ctc_amd: %s needs T >= 1, B >= 1 and C >= 2, got %s" % (name, tuple(x.shape)))
    if not 1 <= N <= W <= BEAM_MAX_WIDTH:
        raise ValueError("ctc_amd: beam search needs 1 <= nbest <= beam_width <= %d, got nbest=%d, beam_width=%d"
                         % (BEAM_MAX_WIDTH, N, W))
    if not 1 <= K <= BEAM_MAX_CLASSES:
        raise ValueError("ctc_amd: beam search needs 1 <= top_classes <= %d, got %d" % (BEAM_MAX_CLASSES, K))
    if L < 1:
        raise ValueError("ctc_amd: beam search needs max_tokens >= 1, got %d" % L)
    if blank is not None and not 0 <= int(blank) < C:
        raise ValueError("ctc_amd: blank must lie in [0, %d), got %d" % (C, int(blank)))
    if not x.is_cuda:
        raise ValueError("ctc_amd: %s must be on a HIP (cuda) device -- the engine has no CPU path" % name)
    K = min(K, C if blank is None else C - 1)
    dev = x.device
    xs = x.detach()
    if xs.stride(2) != 1:
        xs = xs.contiguous()
    il = _lengths(input_lengths, B, "input_lengths", dev, T, lo=0)
    alpha, beta = float(lm_weight), float(token_bonus)
    if lm is None:
        if alpha != 1.0 or beta != 0.0:
            raise ValueError("ctc_amd: lm_weight and token_bonus need a table lm (a pure length bonus: a table of zeros)")
    else:
        lm = _beam_lm_table(lm, C, dev)
        if not (math.isfinite(alpha) and alpha >= 0.0 and math.isfinite(beta)):
            raise ValueError("ctc_amd: beam search needs a finite lm_weight >= 0 and a finite token_bonus, got %r, %r"
                             % (lm_weight, token_bonus))
    tokens = torch.empty((B, N, L), dtype=torch.int32, device=dev)
    lengths = torch.empty((B, N), dtype=torch.int64, device=dev)
    scores = torch.empty((B, N), dtype=torch.float32, device=dev)
    count = torch.empty(B, dtype=torch.int32, device=dev)
    lib = _lib.load()
    need = lib.ctc_amd_beam_search_scratch_bytes(T, B, W)
    scratch = torch.empty(need, dtype=torch.uint8, device=dev)
    if lm is not None:
        ctc_scores = torch.empty((B, N), dtype=torch.float32, device=dev)
        with _on_device(dev):
            rc = lib.ctc_amd_beam_search_lm(xs.data_ptr(), xs.stride(0), xs.stride(1), il.data_ptr(), T, B, C,
                                            -1 if blank is None else int(blank), W, K, N, L, lm.data_ptr(), lm.stride(0),
                                            alpha, beta, tokens.data_ptr(), lengths.data_ptr(), scores.data_ptr(),
                                            ctc_scores.data_ptr(), count.data_ptr(), scratch.data_ptr(), need,
                                            _stream_handle(dev))
        _lib.check(rc, "ctc_amd_beam_search_lm")
        return FusedBeamHypotheses(tokens, lengths, scores, count, ctc_scores)
    with _on_device(dev):
        rc = lib.ctc_amd_beam_search(xs.data_ptr(), xs.stride(0), xs.stride(1), il.data_ptr(), T, B, C,
                                     -1 if blank is None else int(blank), W, K, N, L, tokens.data_ptr(),
                                     lengths.data_ptr(), scores.data_ptr(), count.data_ptr(), scratch.data_ptr(), need,
                                     _stream_handle(dev))
    _lib.check(rc, "ctc_amd_beam_search")
    return BeamHypotheses(tokens, lengths, scores, count)


def blank_beam_search(log_probs, input_lengths, beam_width=16, nbest=1, top_classes=16, blank=0, max_tokens=None,
                      lm=None, lm_weight=1.0, token_bonus=0.0):
    """CTC prefix beam search on the blank lattice, on the device -> ``BeamHypotheses(tokens, lengths, scores, count)``:
    the ``nbest`` most probable LABEL SEQUENCES of each sample, best first.  A sequence's probability is the sum over all
    of its alignments, so this is not ``argmax`` + ``collapse_frames`` (the best single alignment).

    ``log_probs`` [T,B,C] float32 normalised log-probabilities on a HIP device (the contract of ``blank_ctc_loss``), any
    frame / batch strides (a view with another class stride is made contiguous); ``input_lengths`` [B], 0 <= T_b <= T.
    Per frame every prefix of the beam is extended by the ``top_classes`` (<= 32, clamped to C - 1) non-blank classes of
    the largest inputs and the ``beam_width`` (<= 64) most probable prefixes are kept; ties go to a prefix that stays over
    one that is extended, then to the lower beam slot, then to the more probable class (include/ctc_amd.h states the
    rules in full).

    * ``tokens`` [B,nbest,L] int32, L = ``max_tokens`` (default T), -1 behind a sequence's end; ``lengths`` [B,nbest] int64,
      the true token count even where it exceeds L, so a truncation shows.
    * ``scores`` [B,nbest] float32: natural-log probability of the sequence as the search summed it -- at most the exact
      ``-nll`` of that sequence, equal to it when nothing of it was pruned.
    * ``count`` [B] int32: the hypotheses that exist; rows at and beyond it hold -1 / 0 / -inf.  T_b = 0 gives the one
      empty hypothesis with score 0.

    One launch, no host synchronisation, capture-safe (the scratch tensor, 8 B (T beam_width + 1) bytes, is allocated
    here), deterministic.  NaN inputs give an unspecified result.  DESIGN.md 3.13.

    ``lm``: a float32 table [C+1, C] on the same device, shared by the batch -- ``lm[p, c]`` the log-score
    of token c behind token p, row C that of a first token; a finite entry is a score, ``-inf`` forbids the transition
    whatever ``lm_weight`` is.  Every token of a prefix adds ``lm_weight * lm[previous or C, c] + token_bonus`` to the
    score the prefixes are ranked by, frame by frame (shallow fusion with a bigram language model; a 0 / -inf table is a
    transition grammar; a pure length bonus is a table of zeros).  ``lm_weight`` is finite and >= 0, ``token_bonus``
    finite; without ``lm`` both must keep their defaults.  The class candidates of a frame are still chosen on
    ``log_probs`` alone, and the blank's column of ``lm`` is never read.  A view of ``lm`` with unit column stride and a
    row stride >= C is read as it lies, any other is made contiguous.  With ``lm`` the result is
    ``FusedBeamHypotheses(tokens, lengths, scores, count, ctc_scores)``: ``scores`` the fused score, which orders the
    hypotheses, ``ctc_scores`` [B,nbest] float32 the acoustic log-probability alone (what ``scores`` is without ``lm``)."""
    return _beam_search(log_probs, "log_probs", input_lengths, beam_width, nbest, top_classes, int(blank), max_tokens,
                        lm, lm_weight, token_bonus)


def noblank_beam_search(logits, input_lengths, beam_width=16, nbest=1, top_classes=16, max_tokens=None,
                        lm=None, lm_weight=1.0, token_bonus=0.0):
    """``blank_beam_search`` on the no-blank lattice: ``logits`` [T,B,C] float32 RAW logits, as for every other
    ``noblank_*`` function -- the kernel subtracts each row's log-sum-exp itself, in fp32.  There is no blank: a label
    sequence has no equal neighbours, the empty sequence exists only for T_b = 0, and ``top_classes`` is clamped to C.
    ``lm``, ``lm_weight``, ``token_bonus``: as there -- here typically a transition grammar over the classes; the diagonal
    of ``lm`` is never read.  If row C forbids every class, no hypothesis exists for T_b >= 1 (``count`` 0)."""
    return _beam_search(logits, "logits", input_lengths, beam_width, nbest, top_classes, None, max_tokens,
                        lm, lm_weight, token_bonus)


SEQUENCE_SCORES_MAX_LABELS = 255   # ctc_amd_sequence_scores: 511 blank-lattice states, at most 8 per lane of one wave


def _sequence_scores_call(x, name, input_lengths, sequences, sequence_lengths, counts, blank):
    """the checks and the placement of a call -> (x detached, unit class stride; everything else of the call)"""
    if not isinstance(x, torch.Tensor) or x.dim() != 3 or x.dtype != torch.float32:
        raise ValueError("ctc_amd: %s must be a float32 tensor [T,B,C]" % name)
    T, B, C = x.shape
    if T < 1 or B < 1 or C < 1:
        raise ValueError("ctc_amd: %s needs T >= 1, B >= 1 and C >= 1, got %s" % (name, tuple(x.shape)))
    if blank is not None and not 0 <= int(blank) < C:
        raise ValueError("ctc_amd: blank must lie in [0, %d), got %d" % (C, int(blank)))
    seq = sequences
    if not isinstance(seq, torch.Tensor) or seq.dtype not in (torch.int32, torch.int64) or seq.dim() not in (2, 3):
        raise ValueError("ctc_amd: sequences must be an int32 or int64 tensor [B,N,L] (per sample) or [N,L] (shared by "
                         "the batch)")
    shared = seq.dim() == 2
    N, L = seq.shape[-2:]
    if not shared and seq.shape[0] != B:
        raise ValueError("ctc_amd: sequences must have shape [%d,N,L], got %s" % (B, tuple(seq.shape)))
    if N < 1 or L < 1:
        raise ValueError("ctc_amd: sequences needs N >= 1 and L >= 1, got %s" % (tuple(seq.shape),))
    sl = sequence_lengths
    if not isinstance(sl, torch.Tensor):
        sl = torch.as_tensor(sl)
    if sl.dtype not in (torch.int64, torch.int32, torch.int16, torch.uint8, torch.int8) or \
            tuple(sl.shape) != tuple(seq.shape[:-1]):
        raise ValueError("ctc_amd: sequence_lengths must be an integer tensor %s, got %s %s"
                         % (list(seq.shape[:-1]), sl.dtype, tuple(sl.shape)))
    if counts is not None and (not isinstance(counts, torch.Tensor) or counts.dim() != 1 or counts.shape[0] != B or
                               counts.dtype != torch.int32):
        raise ValueError("ctc_amd: counts must be an int32 tensor [%d] (the `count` of a BeamHypotheses)" % B)
    if L > SEQUENCE_SCORES_MAX_LABELS:
        raise _lib.CtcAmdError("ctc_amd: sequence scores take sequences of at most %d labels, got L = %d"
                               % (SEQUENCE_SCORES_MAX_LABELS, L))
    if not x.is_cuda:
        raise ValueError("ctc_amd: %s must be on a HIP (cuda) device -- the engine has no CPU path" % name)
    dev = x.device
    xs = x.detach()
    if xs.stride(2) != 1:
        xs = xs.contiguous()
    il = _lengths(input_lengths, B, "input_lengths", dev, T, lo=0)
    if seq.device != dev:
        seq = seq.to(dev, non_blocking=True)
    if seq.stride(-1) != 1:
        seq = seq.contiguous()
    if sl.device != dev or sl.dtype != torch.int64:
        sl = sl.to(device=dev, dtype=torch.int64, non_blocking=True)
    if sl.stride(-1) != 1:
        sl = sl.contiguous()
    if counts is not None:
        counts = _placed(counts.detach(), dev)
    # everything of a call but x, as both entries take it
    cands = (seq.data_ptr(), int(seq.dtype == torch.int64), 0 if shared else seq.stride(0), seq.stride(-2), L,
             sl.data_ptr(), 0 if shared else sl.stride(0), None if counts is None else counts.data_ptr(), N)
    return xs, _SequenceScoresCall(il, -1 if blank is None else int(blank), cands, (seq, sl, counts))


def _sequence_scores(x, name, input_lengths, sequences, sequence_lengths, counts, blank):
    xs, call = _sequence_scores_call(x, name, input_lengths, sequences, sequence_lengths, counts, blank)
    C = x.shape[2]
    if x.requires_grad and torch.is_grad_enabled():
        if C > SEQUENCE_SCORES_GRAD_MAX_CLASSES:
            raise _lib.CtcAmdError("ctc_amd: the gradient of the sequence scores takes at most %d classes, got C = %d "
                                   "(detach %s, or call under torch.no_grad(), for the scores alone)"
                                   % (SEQUENCE_SCORES_GRAD_MAX_CLASSES, C, name))
        return _SequenceScoresFn.apply(x, call)
    return _sequence_scores_forward(xs, call)


SEQUENCE_SCORES_GRAD_MAX_CLASSES = 4096   # ctc_amd_sequence_scores_grad: the staged path of the forward kernel only


class _SequenceScoresCall(NamedTuple):
    input_lengths: torch.Tensor    # [B] int64 on the device
    blank: int                     # -1: the no-blank lattice
    cands: tuple                   # the arguments from `seq` to `N` of both C entries
    keep: tuple                    # the tensors those pointers belong to


def _sequence_scores_forward(xs, call):
    T, B, C = xs.shape
    dev = xs.device
    scores = torch.empty((B, call.cands[-1]), dtype=torch.float32, device=dev)
    with _on_device(dev):
        rc = _lib.load().ctc_amd_sequence_scores(xs.data_ptr(), xs.stride(0), xs.stride(1), call.input_lengths.data_ptr(),
                                                 T, B, C, call.blank, *call.cands, scores.data_ptr(), _stream_handle(dev))
    _lib.check(rc, "ctc_amd_sequence_scores")
    return scores


def _scratch(kind, need, device):
    """`need` bytes of device memory for a launch that wants scratch (contents mean nothing before and after), from the
    cache of `_workspace`: one growing buffer per (device, stream, kind), superseded by one at least 1.5x as large when
    it is too small, never freed while a captured graph may hold its pointer -- `release_workspaces()` frees it."""
    key = (device.index, _stream_handle(device), kind)
    held = _workspaces.get(key)
    if held is None:
        held = _workspaces[key] = []
    if not held or held[-1].numel() < need:
        size = need if not held else max(need, held[-1].numel() + held[-1].numel() // 2)
        held.append(torch.empty((size + 4095) & ~4095, dtype=torch.uint8, device=device))
    return held[-1]


def _sequence_scores_grad(xs, call, w, out=None, want_scores=False):
    """One call of ctc_amd_sequence_scores_grad: xs [T,B,C] float32 (unit class stride), w [B,N] float32 -> the weighted
    gradient [T,B,C] (written into `out`, any frame / batch strides, when given), with the scores when asked."""
    T, B, C = xs.shape
    dev = xs.device
    N, L = call.cands[-1], call.cands[4]
    if w.dtype != torch.float32 or tuple(w.shape) != (B, N):
        raise ValueError("ctc_amd: the weights of the sequence scores must be float32 [%d,%d]" % (B, N))
    if w.stride(1) != 1:
        w = w.contiguous()
    grad = torch.empty((T, B, C), dtype=torch.float32, device=dev) if out is None else out
    scores = torch.empty((B, N), dtype=torch.float32, device=dev) if want_scores else None
    lib = _lib.load()
    need = lib.ctc_amd_sequence_scores_grad_scratch_bytes(T, B, C, N, L, call.blank)
    if need == 0:
        raise _lib.CtcAmdError("ctc_amd: the gradient of the sequence scores takes at most %d classes and %d labels, got "
                               "C = %d, L = %d" % (SEQUENCE_SCORES_GRAD_MAX_CLASSES, SEQUENCE_SCORES_MAX_LABELS, C, L))
    scratch = _scratch("sequence_scores_grad", need, dev)
    with _on_device(dev):
        rc = lib.ctc_amd_sequence_scores_grad(xs.data_ptr(), xs.stride(0), xs.stride(1), call.input_lengths.data_ptr(),
                                              T, B, C, call.blank, *call.cands, w.data_ptr(), w.stride(0),
                                              grad.data_ptr(), grad.stride(0), grad.stride(1),
                                              None if scores is None else scores.data_ptr(),
                                              scratch.data_ptr(), scratch.numel(), _stream_handle(dev))
    _lib.check(rc, "ctc_amd_sequence_scores_grad")
    return (grad, scores) if want_scores else grad


class _SequenceScoresFn(torch.autograd.Function):
    """scores = the forward launch, unchanged; backward = one call of ctc_amd_sequence_scores_grad with w = grad_output"""

    @staticmethod
    def forward(ctx, x, call):
        xs = x.detach()
        if xs.stride(2) != 1:
            xs = xs.contiguous()
        ctx.save_for_backward(x)
        ctx.call = call
        return _sequence_scores_forward(xs, call)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_scores):
        (x,) = ctx.saved_tensors
        xs = x.detach()
        if xs.stride(2) != 1:
            xs = xs.contiguous()
        w = grad_scores
        if w.dtype != torch.float32:
            w = w.float()
        return _sequence_scores_grad(xs, ctx.call, w), None


def blank_sequence_scores(log_probs, input_lengths, sequences, sequence_lengths, counts=None, blank=0):
    """Exact scores of given label sequences on the blank lattice -> ``scores`` [B,N] float32: ``scores[b, n]`` is the
    natural-log probability of candidate n for sample b, summed over ALL of its alignments of the first T_b frames --
    ``-nll`` of ``blank_ctc_loss`` on that sequence as the target, where that is finite.  All N candidates of all samples
    in one launch: N-best rescoring (``BeamHypotheses.scores`` is only a lower bound of this value), transcript retrieval,
    scoring hypotheses made elsewhere.  Differentiable in ``log_probs`` (below): N-best discriminative training.

    ``log_probs`` [T,B,C] float32 normalised log-probabilities on a HIP device (the contract of ``blank_ctc_loss``), any
    frame / batch strides (a view with another class stride is made contiguous); ``input_lengths`` [B], 0 <= T_b <= T.
    ``sequences``: int32 or int64, either ``[B,N,L]`` with ``sequence_lengths [B,N]`` (candidates per sample; a
    ``BeamHypotheses`` goes in as it is: ``blank_sequence_scores(lp, il, hyp.tokens, hyp.lengths, counts=hyp.count)``) or
    ``[N,L]`` with ``sequence_lengths [N]`` (one set shared by the batch: read through a batch stride of 0, never
    materialised B times, and the same bits as the expanded tensor gives).  Values at and behind a sequence's length are
    never read (-1 padding is fine).  ``counts``: optional int32 [B], the candidates of each sample that exist.
    N >= 1 is otherwise unbounded; L <= 255 labels (``CtcAmdError`` beyond); any T, any C.

    Decided inside the launch, in this order: n >= counts[b]: -inf.  A length < 0 or > L (a hypothesis the beam search
    truncated): NaN, "not scored".  A label among the first ``len`` outside [0, C) or equal to ``blank``: NaN.  T_b = 0:
    0 for the empty sequence, else -inf.  No alignment -- fewer frames than labels + repeats, or every alignment crosses a
    ``-inf`` input (a masked vocabulary; allowed) --: -inf, never NaN and never the loss's 1e13.  The empty sequence scores
    the all-blank path.  NaN inputs give an unspecified value.

    One launch, no scratch, no host synchronisation, capture-safe, deterministic (two calls, or a graph replay, give the
    same bits).  Within 1e-5 max(1, |score|) of float64 also at T = 2000.  DESIGN.md 3.15.

    The gradient.  When ``log_probs`` requires grad and grad mode is on, the result requires grad; the
    values are the same bits and the forward is the same launch (nothing is saved but the inputs).  ``backward`` is one
    call of ``ctc_amd_sequence_scores_grad`` with the incoming gradient as weights: ``log_probs.grad[t, b, c] = sum over
    n of grad_scores[b, n] * d scores[b, n] / d log_probs[t, b, c]``, a contiguous float32 [T,B,C] tensor, for all N
    candidates at once, deterministic.  ``d scores[b, n] / d log_probs[t, b, c]`` is the occupancy of class c at frame t
    in candidate n's own lattice (the sum of the state posteriors of the states that carry c), 0 for t >= T_b: the true
    partial derivative with ``log_probs`` taken as free inputs -- NOT the ``exp(log_probs) - occupancy`` convention of
    ``torch.nn.functional.ctc_loss`` and ``blank_ctc_loss``, which fold the ``log_softmax`` in front of the loss into the
    gradient.  Behind a ``log_softmax`` the gradient that reaches the logits is the same.  A score that is ``-inf`` or
    NaN takes no gradient, whatever arrives for it (NaN and inf included), and rows beyond ``counts`` take none either: the
    candidate is skipped, not multiplied by 0, so ``torch.where(torch.isfinite(s), s, s.new_tensor(-1e30))`` followed by
    a softmax over n is safe.  Where ``log_probs`` is ``-inf`` the gradient is 0.  C <= 4096 (``CtcAmdError`` beyond,
    when a gradient is asked for).  The scratch of the backward (``ctc_amd_sequence_scores_grad_scratch_bytes``: about
    16 (2L + 1) bytes per candidate and frame) comes from the module's growing workspace cache; ``release_workspaces()``
    frees it.  Without a gradient -- the input does not require grad, or under ``torch.no_grad()`` -- nothing changes."""
    return _sequence_scores(log_probs, "log_probs", input_lengths, sequences, sequence_lengths, counts, int(blank))


def noblank_sequence_scores(logits, input_lengths, sequences, sequence_lengths, counts=None):
    """``blank_sequence_scores`` on the no-blank lattice: ``logits`` [T,B,C] float32 RAW logits, as for every other
    ``noblank_*`` function -- the kernel subtracts each row's log-sum-exp itself, in fp32, once for all candidates.  The
    lattice is the loss's: stay / advance, from the first label at frame 0 to the last at frame T_b - 1, so the score is
    ``-nll`` of ``noblank_ctc_loss`` on that target where that is finite.  For a sequence without equal neighbours that is
    the probability that the frames collapse to it; with equal neighbours it is what the loss's lattice gives for that
    target (the two labels are two states), not a collapse probability.  The empty sequence has an alignment only for
    T_b = 0 (score 0; -inf for T_b >= 1); fewer frames than labels: -inf.  A row that is ``-inf`` throughout gives an
    unspecified value.  Everything else as there, the gradient included: here ``d scores[b, n] / d logits[t, b, c]`` is the
    class occupancy minus ``softmax(logits[t, b])[c]`` (the log-sum-exp is taken inside, so this IS the gradient with
    respect to the raw logits, the convention of ``noblank_ctc_loss``), and the softmax is taken once per row for all
    candidates; a ``-inf`` or NaN score takes no gradient."""
    return _sequence_scores(logits, "logits", input_lengths, sequences, sequence_lengths, counts, None)
