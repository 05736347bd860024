"""Lengths and labels outside their range on the MI355X: every loss and every lattice read-out, on every path of the
existing tables, with device-resident lengths that nothing has validated -- the cases, the buffers and the float64
expectations of tests/bad_inputs_ref.py (tests/test_bad_inputs_ref.py checks them without a GPU, and that no address an
unguarded kernel would touch leaves this file's own allocations: memory safety here never rests on a guard).

Every launch goes through the C ABI on padded buffers (x in the middle of a larger tensor of canary logits, every other
array in front of a canary tail), twice: the case, and its TWIN in which every bad-length sample is the in-range pair
without an alignment (1, 2).  Then once more through the public Python API with default settings.  Per launch:
  * the good samples -- those with labels outside [0, C) among them -- have the twin's BITS in nll, gradient rows, gamma,
    path, score, frame_conf, spans and conf (every kernel here works per sample and is deterministic);
  * against float64 they stay within the bounds the existing tests hold these paths to on `randn` inputs: nll 1e-5
    relative, the gradient within plain_bound (test_noblank_vs_oracle_shapes / test_binary_vs_oracle_shapes /
    test_blank_vs_torch_cpu at that B), gamma 2e-4 (blank: 2e-5 up to T = 256, 5e-4 beyond, test_blank_posteriors_gpu),
    the best path's score 1e-5 / 2e-5 relative (blank: path and score those of the float32 restatement, bit for bit);
  * a bad-length sample reports what include/ctc_amd.h says: nll >= 1e12 and never NaN (blank: +inf), all T gradient
    rows 0, path -1 on all T frames, score -inf, gamma 0, spans -1 / -1, conf 0, frame_conf 0, +inf from the token spans;
  * `loss` is what the header defines for the nll the launch returned (tests/batch_sum_ref.py);
  * every canary -- the flanks of x, every tail, and the inputs themselves -- keeps its bits, and the status word is 0.
The Python layer: the ABI run's bits from device lengths, ValueError before any launch from CPU lengths out of range, and
from device lengths with CTC_AMD_VALIDATE (functional._VALIDATE) switched on.

Measured on an MI355X (gfx950), the library as this file's commit leaves it: all 140 cases pass in 3.1 s (5 s of wall time
with the start of the interpreter; the slowest case 0.31 s).  Largest errors of the good samples against float64 --
    no-blank  nll 3.0e-7 relative, gradient 6.6e-6 (bound 1e-4 at B = 5), gamma 1.3e-5, score 3.3e-5 (bound 1e-5 |score|)
    binary    nll 4.3e-7, gradient 3.6e-7 (bound 2.6e-5 at B = 2), gamma 8.5e-6, score 1.7e-5
    blank     nll 1.4e-6, gradient 7.8e-6 (bound 2.1e-5 .. 9.4e-5), gamma 7.3e-5 at T = 660 (bound 5e-4)
-- and every bitwise assertion held.  Before the fixes of this commit these failed: the twelve blank-loss cases whose good
sample carries a negative label (clamped onto the blank's class: nll off by up to 1.5e-2 relative, then the gradient by
up to 3.5e-2).  The blank posteriors and token spans wrote NaN, not +inf, for a bad-length sample: seen in
the source and changed before the first run."""
import ctypes

import numpy as np
import pytest
import torch

from tests import bad_inputs_ref as ref
from tests import batch_sum_ref
from tests import blank_grad_ref as bg
from tests import lattice_inputs_ref as li
from tests.helpers import np_
from tests.smoothing_ref import smoothed_ref
from tests.test_blank_token_spans_abi import padded as blank_padded, spans_of_path as blank_spans_of_path
from tests.test_token_spans_abi import padded, spans_of_path

pytestmark = pytest.mark.gpu

FLOAT_CANARY, INT_CANARY = 24576.0, 0x5A5A5A5A            # (24576: exact in bf16 and fp16 too)
NO_ALIGNMENT = li.NO_ALIGNMENT
SCORE_RTOL = {"noblank": 1e-5, "binary": 2e-5}              # test_noblank_best_path / test_binary_best_path
TORCH_DTYPE = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
DTYPE_CODE = {"f32": 0, "bf16": 1, "f16": 2}
VARIANT = {"noblank": 0, "binary": 1, "blank": 2}

LOSS_RUNS = ([("noblank", p, c, "f32", None) for p in li.NOBLANK_LOSS for c in range(len(ref.compositions(li.NOBLANK_SHAPES[p][1])))]
             + [("noblank", "r16", c, form, lam) for c in (0, 1) for form, lam in (("bf16", None), ("f16", None), ("f32", 0.5))]
             + [("binary", p, c, "f32", None) for p in li.BINARY_SHAPES for c in (0, 1)])
BLANK_RUNS = [(p, c, s) for p in bg.SHAPES for c in (0, 1) for s in bg.SCHEDULES[p]]
READOUT_RUNS = ([(f, kind, p, c, "f32") for f in ("noblank", "binary") for kind, table in
                 (("best_path", li.PATH_SHAPES), ("posteriors", li.POSTERIOR_SHAPES), ("token_spans", li.PATH_SHAPES))
                 for p in table[f] for c in (0, 1)]
                + [(f, kind, {"noblank": "r16", "binary": "flow"}[f], 0, {"noblank": "bf16", "binary": "f16"}[f])
                   for f in ("noblank", "binary") for kind in ("best_path", "posteriors", "token_spans")])
BLANK_READOUT_RUNS = [(kind, p, c) for kind in ("best_path", "posteriors", "token_spans") for p in ("k2", "k8", "w2", "w3")
                      for c in (0, 1)]


def _id(run):
    return "-".join("auto" if v is None else str(v) for v in run)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    import ctc_amd  # noqa: F401  (raises if libctc_amd.so is missing)
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _restore_schedule():
    yield
    import ctc_amd
    ctc_amd.set_blank_schedule(-1)
    try:                                                         # a device fault ends the run: nothing more is launched on it
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit("the device reported %s: no further launches" % str(e).splitlines()[0], returncode=3)


def _lib():
    from ctc_amd import _lib as binding
    return binding.load()


# ---- buffers ---------------------------------------------------------------------------------------------------------
class Buffers:
    """a case on the device, laid out as tests/bad_inputs_ref.layout says; every array is remembered with the bits it was
    given, so that check_untouched() can tell a stray store anywhere: flanks, tails, and the inputs themselves"""

    def __init__(self, dev, case, form="f32"):
        self.dev, self.c, self.form = dev, case, form
        f, T, B, C, S = (case[k] for k in ("family", "T", "B", "C", "S"))
        self.f, self.T, self.B, self.C, self.S = f, T, B, C, S
        self.lay = ref.layout(f, T, B, C, S)
        self.kept = []                                           # (name, tensor, its bits on the host)
        dt = TORCH_DTYPE[form]
        X = torch.full((T + ref.T_MARGIN, B + 1, 3 * C), ref.LOGPROB_CANARY if f == "blank" else ref.LOGIT_CANARY, dtype=dt)
        X[:T, :B, C:2 * C] = case["x"].to(dt)
        assert X.numel() == self.lay["X"][0]
        self.X = self._keep("X", X)
        self.x = self.X[:T, :B, C:2 * C]
        assert (self.x.storage_offset(), self.x.stride(0), self.x.stride(1)) == ref.x_strides(B, C) and self.x.stride(2) == 1
        if f == "binary":
            n, tail = self.lay["y"]
            y = torch.zeros(n + tail)
            y[:n] = case["tg"].reshape(-1)
            self.tg_full = self._keep("y", y)
            self.tg = self.tg_full[:n].view(B, S, C)
        else:
            n, tail = self.lay["labels"]
            lab = torch.empty(n + tail, dtype=case["tg"].dtype)
            lab[:n] = case["tg"].reshape(-1)
            lab[n:] = torch.tensor(ref.label_tail(C), dtype=lab.dtype)
            self.tg_full = self._keep("labels", lab)
            self.tg = self.tg_full[:n].view(B, S)
        self.lens = {}
        for which in ("", "_twin"):
            pair = []
            for name, key in (("in_len", "Tb"), ("tgt_len", "L")):
                n, tail = self.lay[name]
                v = torch.ones(n + tail, dtype=torch.int64)      # (the tail: a valid length)
                v[:n] = torch.from_numpy(np.array(case[key + which]))
                pair.append(self._keep(name + which, v)[:n])
            self.lens[which] = pair
        self.outs = []

    def _keep(self, name, host):
        d = host.to(self.dev)
        self.kept.append((name, d, host.clone()))
        return d

    def out(self, name, shape, dtype=torch.float32):
        """an output of the ABI's shape in front of its canary tail, canaries all over"""
        n, tail = self.lay[name]
        assert int(np.prod(shape)) == n, (name, shape, n)
        if dtype == torch.int32:
            full = torch.full((n + tail,), INT_CANARY, dtype=dtype, device=self.dev)
        else:
            full = torch.full((n + tail,), FLOAT_CANARY, dtype=dtype, device=self.dev)
        self.outs.append((name, full, n))
        return full[:n].view(*shape)

    def check_untouched(self, what):
        torch.cuda.synchronize()
        for name, d, host in self.kept:
            same = torch.equal(d.cpu().view(torch.uint8), host.view(torch.uint8))
            assert same, "%s: %s (an input, its flanks or its tail) was written to" % (what, name)
        for name, full, n in self.outs:
            tail = full[n:].cpu()
            want = torch.full_like(tail, INT_CANARY if tail.dtype == torch.int32 else FLOAT_CANARY)
            assert torch.equal(tail.view(torch.uint8), want.view(torch.uint8)), "%s: the tail of %s was written to" % (what, name)
        self.outs = []


def _workspace(dev, f, T, B, C, S):
    n = _lib().ctc_amd_workspace_bytes(VARIANT[f], T, B, C, S)
    return torch.zeros((n + 4095) & ~4095, dtype=torch.uint8, device=dev)


def _status(ws):
    word = ctypes.c_uint(0)
    rc = _lib().ctc_amd_workspace_status(ws.data_ptr(), 1, torch.cuda.current_stream().cuda_stream, ctypes.byref(word))
    assert rc == 0
    return word.value


def _call(entry, buf, which, ws, extra, outs):
    """entry(x[, x_dtype], stride_t, stride_b, targets[, labels_i64], in_len, tgt_len, T, B, C, S, *extra, *outs, ws, stream)"""
    il, tl = buf.lens[which]
    args = [buf.x.data_ptr()]
    assert entry.endswith("_typed") == (buf.form != "f32")
    if buf.form != "f32":
        args.append(DTYPE_CODE[buf.form])
    args += [buf.x.stride(0), buf.x.stride(1), buf.tg.data_ptr()]
    if buf.f != "binary":
        args.append(int(buf.tg.dtype == torch.int64))
    args += [il.data_ptr(), tl.data_ptr(), buf.T, buf.B, buf.C, buf.S, *extra]
    args += [None if o is None else o.data_ptr() for o in outs]
    args += [None if ws is None else ws.data_ptr(), torch.cuda.current_stream().cuda_stream]
    rc = getattr(_lib(), entry)(*args)
    assert rc == 0, (entry, rc)


def run_loss(buf, which, lam=None, blank=0):
    """one loss launch through the C ABI -> dict of numpy arrays (nll, loss, grad as float32), the scale it was given"""
    f, T, B, C, S = buf.f, buf.T, buf.B, buf.C, buf.S
    ws = _workspace(buf.dev, f, T, B, C, S)
    nll, loss = buf.out("nll", (B,)), buf.out("loss", (1,))
    grad = buf.out("grad", (T, B, C), TORCH_DTYPE[buf.form])
    scale = 1.0 / B
    if f == "blank":
        _call("ctc_amd_blank_loss_grad", buf, which, ws, (blank, scale, scale), (nll, loss, grad))
    elif f == "binary":
        _call("ctc_amd_binary_loss_grad", buf, which, ws, (scale, scale), (nll, loss, grad))
    elif buf.form != "f32":
        _call("ctc_amd_noblank_loss_grad_typed", buf, which, ws, (-1.0 if lam is None else lam, scale, scale), (nll, loss, grad))
    elif lam is not None:
        _call("ctc_amd_noblank_smoothed_loss_grad", buf, which, ws, (lam, scale, scale), (nll, loss, grad))
    else:
        _call("ctc_amd_noblank_loss_grad", buf, which, ws, (scale, scale), (nll, loss, grad))
    r = {"nll": np_(nll), "loss": np.float32(np_(loss)[0]), "grad": np_(grad.float()), "grad_raw": grad.clone(),
         "scale": np.float32(scale)}
    buf.check_untouched("loss" + which)
    assert _status(ws) == 0
    return r


READOUT_OUTPUTS = {
    "best_path": ("path", "score"),
    "posteriors": ("nll", "gamma"),
    "token_spans": ("path", "score", "nll", "frame_conf", "start", "end", "conf"),
}


def run_readout(buf, kind, which, blank=0):
    f, T, B, C, S = buf.f, buf.T, buf.B, buf.C, buf.S
    shapes = {"path": ((B, T), torch.int32), "score": ((B,), torch.float32), "nll": ((B,), torch.float32),
              "gamma": ((B, T, ref.states(f, S)), torch.float32), "frame_conf": ((B, T), torch.float32),
              "start": ((B, S), torch.int32), "end": ((B, S), torch.int32), "conf": ((B, S), torch.float32)}
    outs = {name: buf.out(name, *shapes[name]) for name in READOUT_OUTPUTS[kind]}
    ws = _workspace(buf.dev, f, T, B, C, S)
    entry = "ctc_amd_%s_%s" % (f, kind)
    if f == "blank":
        if S > 255 and kind != "token_spans":
            entry += "_wide"
        _call(entry, buf, which, ws, (blank,), list(outs.values()))
    else:
        _call(entry + ("" if buf.form == "f32" else "_typed"), buf, which, ws, (), list(outs.values()))
    r = {name: np_(t) for name, t in outs.items()}
    buf.check_untouched("%s%s" % (kind, which))
    assert _status(ws) == 0
    return r


# ---- assertions --------------------------------------------------------------------------------------------------------
def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def per_sample(name, a, b):
    """sample b of an output (the gradient is [T,B,C])"""
    return a[:, b] if name == "grad" else a[b]


def check_twin(case, main, twin, what):
    """good samples: the twin's bits, in every per-sample output"""
    for name in main:
        if name in ("loss", "scale", "grad_raw"):
            continue
        for b in np.nonzero(~case["bad"])[0]:
            assert np.array_equal(bits(per_sample(name, main[name], b)), bits(per_sample(name, twin[name], b))), \
                "%s: %s of good sample %d differs from the twin run" % (what, name, b)


def check_bad_lengths(case, r, what, which=""):
    """the contract values of a sample with lengths outside the tensor (and of the twin's (1, 2))"""
    f = case["family"]
    for b in np.nonzero(case["bad"])[0]:
        tag = "%s%s: sample %d (%s: T_b = %d, L_b = %d)" % (what, which, b, case["kind"][b], case["Tb" + which][b],
                                                          case["L" + which][b])
        if "nll" in r:
            v = r["nll"][b]
            assert not np.isnan(v) and v >= NO_ALIGNMENT, "%s: nll %r" % (tag, v)
            if f == "blank" or "frame_conf" in r:
                assert np.isposinf(v), "%s: nll %r where +inf is due" % (tag, v)
        if "grad" in r:
            assert (r["grad"][:, b] == 0).all(), "%s: a gradient row is not 0" % tag
        if "path" in r:
            assert (r["path"][b] == -1).all(), "%s: path" % tag
            assert np.isneginf(r["score"][b]), "%s: score %r" % (tag, r["score"][b])
        if "gamma" in r:
            assert (r["gamma"][b] == 0).all(), "%s: gamma" % tag
        if "frame_conf" in r:
            assert (r["frame_conf"][b] == 0).all() and (r["conf"][b] == 0).all(), "%s: confidences" % tag
            assert (r["start"][b] == -1).all() and (r["end"][b] == -1).all(), "%s: spans" % tag


def check_loss_scalar(case, r, what, which=""):
    f, B = case["family"], case["B"]
    e = batch_sum_ref.expected_loss(f, r["nll"], B, r["scale"], L=np.array(case["L" + which]) if f == "blank" else None)
    wrong = batch_sum_ref.check_loss(r["loss"], e)
    assert not wrong, (what, wrong)


def gradient_bound(case):
    f, T, B = case["family"], case["T"], case["B"]
    return bg.plain_bound(T, B) if f == "blank" else li.plain_bound(f, B)


def check_good_against_float64(case, r, e, what, grad_ref=None):
    """the twin run's good samples (bad labels included) against float64, within the existing bounds"""
    f, T = case["family"], case["T"]
    good = ~case["bad"]
    assert e["fin"][good].all()
    out = {}
    if "nll" in r:
        nll = r["nll"].astype(np.float64)
        want = e["nll"] if grad_ref is None else grad_ref["nll"]
        out["nll_rel"] = float((np.abs(nll[good] - want[good]) / np.maximum(1.0, np.abs(want[good]))).max())
        assert out["nll_rel"] <= li.NLL_RTOL, "%s: nll off by %.3e relative" % (what, out["nll_rel"])
    if "grad" in r:
        want = e["grad"] if grad_ref is None else grad_ref["grad"]
        out["grad"] = float(np.abs(r["grad"].astype(np.float64)[:, good] - want[:, good]).max())
        assert np.isfinite(r["grad"]).all()
        assert out["grad"] <= gradient_bound(case), "%s: gradient off by %.3e (bound %.3e)" % (what, out["grad"], gradient_bound(case))
        for b in np.nonzero(good)[0]:
            assert (r["grad"][int(case["Tb_twin"][b]):, b] == 0).all(), "%s: sample %d beyond T_b" % (what, b)
    if "gamma" in r:
        out["gamma"] = float(np.abs(r["gamma"].astype(np.float64)[good] - e["gamma"][good]).max())
        bound = li.GAMMA_ATOL if f != "blank" else (2e-5 if T <= 256 else 5e-4)
        assert out["gamma"] <= bound, "%s: gamma off by %.3e (bound %.1e)" % (what, out["gamma"], bound)
    if "path" in r:
        if f == "blank":                                         # the float32 restatement: the kernel's bits
            assert np.array_equal(r["path"][good], e["path"][good]), "%s: path" % what
            assert np.array_equal(bits(r["score"][good]), bits(e["score"][good])), "%s: score" % what
        else:
            score = r["score"].astype(np.float64)
            out["score"] = float(np.abs(score[good] - e["score"][good]).max())
            assert out["score"] <= SCORE_RTOL[f] * max(1.0, np.abs(e["score"][good]).max()), (what, out["score"])
            out["path"] = float((r["path"][good] == e["path"][good]).mean())
            for b in np.nonzero(good)[0]:
                tb, l = int(case["Tb_twin"][b]), int(case["L_twin"][b])
                p = r["path"][b]
                assert (p[tb:] == -1).all() and p[0] == 0 and p[tb - 1] == l - 1 and set(np.diff(p[:tb])) <= {0, 1}, (what, b)
    if "frame_conf" in r:
        path, fc = r["path"], r["frame_conf"]
        want = np.take_along_axis(e["gamma"], np.maximum(path, 0)[:, :, None].astype(np.int64), 2)[:, :, 0]
        want[path < 0] = 0.0
        out["frame_conf"] = float(np.abs(fc[good] - want[good]).max())
        bound = li.GAMMA_ATOL if f != "blank" else (2e-5 if T <= 256 else 5e-4)
        assert out["frame_conf"] <= bound, (what, out["frame_conf"])
        sp, pd = (blank_spans_of_path, blank_padded) if f == "blank" else (spans_of_path, padded)
        s, en, cf = sp(path, fc, case["Tb_twin"], case["L_twin"])
        S = case["S"]
        assert np.array_equal(r["start"], pd(s, S, -1)) and np.array_equal(r["end"], pd(en, S, -1)), "%s: spans" % what
        assert np.array_equal(bits(r["conf"]), bits(pd(cf, S, 0))), "%s: conf" % what
    print("bad inputs %s: %s" % (what, " ".join("%s %.3e" % kv for kv in out.items())))
    return out


# ---- the public Python layer ---------------------------------------------------------------------------------------------
def api_loss(buf, lam=None):
    import ctc_amd
    il, tl = buf.lens[""]
    x = buf.x.detach().requires_grad_(True)
    if buf.f == "blank":
        loss, nll = ctc_amd.blank_ctc_loss(x, buf.tg, il, tl)
    elif buf.f == "binary":
        loss, nll = ctc_amd.binary_ctc_loss(x, buf.tg, il, tl)
    else:
        loss, nll = ctc_amd.noblank_ctc_loss(x, buf.tg, il, tl, label_smoothing=lam)
    loss.backward()
    torch.cuda.synchronize()
    return {"nll": np_(nll), "loss": np.float32(np_(loss.detach())), "grad_raw": x.grad}


def check_api_loss(buf, main, lam, what):
    import ctc_amd
    a = api_loss(buf, lam)
    assert np.array_equal(bits(a["nll"]), bits(main["nll"])), "%s: nll through the Python layer" % what
    assert bits(np.array([a["loss"]]))[0] == bits(np.array([main["loss"]]))[0], "%s: loss through the Python layer" % what
    assert a["grad_raw"].dtype == main["grad_raw"].dtype
    assert torch.equal(a["grad_raw"].contiguous().view(torch.uint8), main["grad_raw"].contiguous().view(torch.uint8)), \
        "%s: gradient through the Python layer" % what
    buf.check_untouched(what + " (Python layer)")
    assert ctc_amd.workspace_status() == 0


def check_api_readout(buf, kind, main, what):
    import ctc_amd
    il, tl = buf.lens[""]
    out = getattr(ctc_amd, "%s_%s" % (buf.f, kind))(buf.x, buf.tg, il, tl)
    torch.cuda.synchronize()
    if kind == "best_path":
        got = {"path": out[0], "score": out[1]}
    elif kind == "posteriors":
        got = {"gamma": out[0], "nll": out[1]}
    else:
        got = {k: getattr(out, k) for k in READOUT_OUTPUTS[kind]}
    for name, t in got.items():
        assert np.array_equal(bits(np_(t)), bits(main[name])), "%s: %s through the Python layer" % (what, name)
    buf.check_untouched(what + " (Python layer)")
    assert ctc_amd.workspace_status() == 0


# ---- 1. the losses -------------------------------------------------------------------------------------------------------
def _loss_case(dev, family, path, comp, form, lam, blank_schedule=None):
    case = ref.make_case(family, path, comp)
    what = "%s-%s-%s%s%s" % (family, path, "ab"[comp], "" if form == "f32" else "-" + form, "" if lam is None else "-lam%g" % lam)
    buf = Buffers(dev, case, form)
    main, twin = run_loss(buf, "", lam), run_loss(buf, "_twin", lam)
    check_twin(case, main, twin, what)
    check_bad_lengths(case, main, what)
    check_bad_lengths(case, twin, what, "_twin")
    check_loss_scalar(case, main, what)
    check_loss_scalar(case, twin, what, "_twin")
    e = ref.expected(family, path, comp)
    if form == "f32":
        grad_ref = None
        if lam is not None:                                      # the smoothed emission: its own float64 restatement
            sm = smoothed_ref(case["x"], ref.effective_classes(family, np_(case["tg"]), case["C"]), case["Tb_twin"],
                              case["L_twin"], lam)
            assert np.array_equal(sm["fin"], e["fin"])
            grad_ref = {"nll": sm["nll"], "grad": sm["grad"]}
        check_good_against_float64(case, twin, e, what, grad_ref)
    else:
        # tests/test_lowp_gpu.py's contract: the bits of the fp32 launch on the widened values, the gradient rounded once
        wide = Buffers(dev, dict(case, x=case["x"].to(TORCH_DTYPE[form]).float()), "f32")
        for which, r in (("", main), ("_twin", twin)):
            w = run_loss(wide, which, lam)
            assert np.array_equal(bits(r["nll"]), bits(w["nll"])), "%s: nll is not the fp32 launch's" % what
            assert torch.equal(r["grad_raw"].view(torch.int16), w["grad_raw"].to(TORCH_DTYPE[form]).view(torch.int16)), what
    check_api_loss(buf, main, lam, what)
    return main


@pytest.mark.parametrize("run", LOSS_RUNS, ids=_id)
def test_loss(dev, run):
    _loss_case(dev, *run)


@pytest.mark.parametrize("run", BLANK_RUNS, ids=_id)
def test_blank_loss(dev, run):
    import ctc_amd
    path, comp, schedule = run
    ctc_amd.set_blank_schedule(-1 if schedule is None else schedule)     # (process-wide: the ABI calls below see it too)
    _loss_case(dev, "blank", path, comp, "f32", None)


# ---- 2. the read-outs ----------------------------------------------------------------------------------------------------
def _readout_case(dev, family, kind, path, comp, form):
    case = ref.make_case(family, path, comp)
    what = "%s-%s-%s-%s%s" % (family, kind, path, "ab"[comp], "" if form == "f32" else "-" + form)
    buf = Buffers(dev, case, form)
    main, twin = run_readout(buf, kind, ""), run_readout(buf, kind, "_twin")
    check_twin(case, main, twin, what)
    check_bad_lengths(case, main, what)
    check_bad_lengths(case, twin, what, "_twin")
    if form == "f32":
        check_good_against_float64(case, twin, ref.expected(family, path, comp), what)
    else:                                                        # tests/test_readout_typed_gpu.py: the fp32 call's bits
        wide = Buffers(dev, dict(case, x=case["x"].to(TORCH_DTYPE[form]).float()), "f32")
        w = run_readout(wide, kind, "")
        for name in main:
            assert np.array_equal(bits(main[name]), bits(w[name])), "%s: %s is not the fp32 launch's" % (what, name)
    check_api_readout(buf, kind, main, what)


@pytest.mark.parametrize("run", READOUT_RUNS, ids=_id)
def test_readout(dev, run):
    _readout_case(dev, *run)


@pytest.mark.parametrize("run", BLANK_READOUT_RUNS, ids=_id)
def test_blank_readout(dev, run):
    kind, path, comp = run
    _readout_case(dev, "blank", kind, path, comp, "f32")


# ---- 3. the Python layer's own checks --------------------------------------------------------------------------------------
LAUNCHING = ("loss_grad", "best_path", "posteriors", "token_spans", "scale_grad")


def _counting(monkeypatch):
    """count the calls of every launching entry on the library handle (tests/test_head_backward_gpu.py)"""
    from ctc_amd import _lib as binding
    lib = binding.load()
    calls = []
    for name in binding.PROTOTYPES:
        if any(k in name for k in LAUNCHING):
            real = getattr(lib, name)
            monkeypatch.setattr(lib, name, lambda *a, _real=real, _name=name: (calls.append(_name), _real(*a))[1])
    return calls


def _api_calls(family):
    import ctc_amd
    names = ["ctc_loss", "best_path", "posteriors", "token_spans"]
    return [getattr(ctc_amd, "%s_%s" % (family, n)) for n in names]


@pytest.mark.parametrize("family,path", [("noblank", "r16"), ("binary", "flow"), ("blank", "k2")])
def test_python_layer_validates_what_it_can_see(dev, monkeypatch, family, path):
    """CPU lengths out of range raise ValueError before any launch; device lengths only with CTC_AMD_VALIDATE
    (functional._VALIDATE), and then before any launch as well; by default they pass unchecked (the runs above)"""
    from ctc_amd import functional
    case = ref.make_case(family, path, 0)
    assert any(k != "infeasible" for k in case["kind"] if k)
    x, tg = case["x"].to(dev), case["tg"].to(dev)
    Tb, L = torch.from_numpy(np.array(case["Tb"])), torch.from_numpy(np.array(case["L"]))
    good_Tb, good_L = (torch.from_numpy(np.array(v)) for v in case["valid"])
    calls = _counting(monkeypatch)
    for fn in _api_calls(family):
        with pytest.raises(ValueError):
            fn(x, tg, Tb, L)                                      # lengths on the host
    assert calls == []
    monkeypatch.setattr(functional, "_VALIDATE", True)
    for fn in _api_calls(family):
        with pytest.raises(ValueError):
            fn(x, tg, Tb.to(dev), L.to(dev))                      # lengths on the device, validation switched on
    assert calls == []
    for fn in _api_calls(family):                                 # valid ones still pass with it
        fn(x, tg, good_Tb.to(dev), good_L.to(dev))
    torch.cuda.synchronize()
    assert len(calls) == 4
