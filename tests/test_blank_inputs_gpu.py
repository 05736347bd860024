"""Blank-CTC loss + gradient on the MI355X on the inputs a real caller produces and `randn.log_softmax` never does:
peaked log-probs (a trained model: `aligned4` / `aligned8`; a peak on the wrong class, nll in the thousands: `rand30`)
and -inf entries (a masked vocabulary: `masked`, `masked_rand30`), on every path of ctc_amd_blank_loss_grad -- 2, 4 and 8
states per lane on the three launches (schedule 0), the persistent launch with row pairs (1) and with the pool gather
(2), and the wide path on two and three waves.  The cases and the float64 reference that is defined at -inf are those of
tests/blank_grad_ref.py; tests/test_blank_inputs_ref.py checks them without a GPU.

Per case and schedule: nll is +inf exactly on the samples without an alignment (the masked cases hold samples that have
none through their EMISSIONS alone: a first label no frame emits, and an empty target whose only path crosses a hole in
the blank) and within 1e-5 relative otherwise; the gradient is finite, exactly 0 beyond T_b, at every -inf entry and on
every row of a sample with nll = +inf; its error against float64 over the feasible samples stays within
min(1e-4, max(plain, 2 err32)), plain = the bound of test_blank_vs_torch_cpu, err32 = the error of torch's own float32
CPU kernel on the same inputs (it exceeds plain on rand30); every live row sums to sum_c exp(lp) - 1 within 1e-5 after
undoing the 1/(L_b B) scale; a forward-only call gives the same nll to 2e-6 relative.  Every case prints err, err32,
err/err32, the bound and max |grad_ref| before it asserts.

Measured on an MI355X (err: the worst of the case's schedules; nll within 1.2e-6 relative everywhere; the persistent
launch against the three launches at most 1.5e-5, on k8-rand30).  The kernels stay at or below 0.13 x err32 on every
case but the two smallest (k2_scalar-aligned8 0.31, k2_scalar-masked 0.99, both below 3e-7 absolute): peaked inputs cost
torch's float32 kernel up to 1.6e-3, the per-row softmax of the lattice here 1.1e-5 at most.

    path       regime         err       err32     bound     max|grad_ref|
    k2_scalar  rand30         2.6e-07   4.5e-05   9.0e-05   2.5e-01
    k2_scalar  aligned4       2.0e-08   5.4e-07   3.2e-05   2.1e-01
    k2_scalar  aligned8       1.3e-08   4.0e-08   3.2e-05   2.5e-02
    k2_scalar  masked         2.5e-07   2.6e-07   3.2e-05   4.6e-02
    k2         rand30         3.6e-06   4.5e-04   1.0e-04   1.7e-01
    k2         aligned4       5.2e-08   4.0e-06   2.1e-05   1.6e-01
    k2         aligned8       1.2e-08   1.6e-07   2.1e-05   6.5e-02
    k2         masked         8.3e-07   7.8e-06   2.1e-05   1.7e-01
    k4         rand30         1.9e-06   8.6e-04   1.0e-04   2.5e-01
    k4         aligned4       1.0e-07   8.0e-06   3.2e-05   2.4e-01
    k4         aligned8       1.1e-08   5.0e-07   3.2e-05   8.2e-02
    k4         masked         1.4e-06   1.1e-05   3.2e-05   5.0e-02
    k8         rand30         1.1e-05   4.5e-04   1.0e-04   6.7e-02
    k8         aligned4       9.3e-08   8.5e-06   4.3e-05   6.3e-02
    k8         aligned8       5.8e-09   2.9e-07   4.3e-05   1.5e-02
    k8         masked         2.1e-06   2.7e-05   5.4e-05   6.7e-02
    w2         rand30         7.6e-07   4.5e-04   1.0e-04   6.7e-02
    w2         aligned4       1.9e-07   1.7e-05   4.3e-05   6.3e-02
    w2         aligned8       5.3e-09   4.5e-07   4.3e-05   1.7e-02
    w2         masked         3.0e-06   4.2e-05   8.5e-05   6.6e-02
    w3         rand30         1.0e-05   1.6e-03   1.0e-04   6.7e-02
    w3         aligned4       6.5e-07   2.3e-05   9.4e-05   6.3e-02
    w3         aligned8       6.7e-09   5.8e-07   9.4e-05   1.6e-02
    w3         masked         4.0e-06   1.1e-04   1.0e-04   6.7e-02
    k2         masked_rand30  4.3e-07   1.8e-04   1.0e-04   1.7e-01
    w2         masked_rand30  6.4e-07   6.1e-04   1.0e-04   6.7e-02

Before the rule "a row whose maximum is below the nll's -1e29 threshold is a zero row" (blank_row_emit, blank_wide.hpp)
every masked case failed here on every schedule and on the wide path, on the samples without an alignment through
their emissions alone: non-zero rows of the size of real gradients (1.4e-3 on k8-masked), NaN on others.
"""
import hashlib
import os

import numpy as np
import pytest
import torch

from tests.blank_grad_ref import CASES, NLL_RTOL, SCHEDULES, SHAPES, exact_case, reference
from tests.helpers import np_

pytestmark = pytest.mark.gpu

RUNS = [(p, r, s) for p, r in CASES for s in SCHEDULES[p]]
FORCED = [c for c in CASES if len(SCHEDULES[c[0]]) == 3]
RECORDED = [(p, s) for p in SHAPES for s in SCHEDULES[p] if s != 2]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "blank_loss_bits.npz")


def _id(v):
    return "-".join("auto" if x is None else str(x) for x in v)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    import ctc_amd  # noqa: F401  (raises if libctc_amd.so is missing)
    return torch.device("cuda:0")


request_undo = []


@pytest.fixture(autouse=True)
def _restore_schedule():
    yield
    while request_undo:
        request_undo.pop()()


def _schedule(mode):
    """blank-CTC schedule for this test only: 1 / 0 force / forbid the persistent launch, 2 forces it with the pool
    gather, None the library's choice (the wide path has one schedule)"""
    import ctc_amd
    ctc_amd.set_blank_schedule(-1 if mode is None else mode)
    request_undo.append(lambda: ctc_amd.set_blank_schedule(-1))


def run_loss(dev, lp, tgt, Tb, L, blank=0, grad=True, fn=None):
    import ctc_amd
    x = lp.to(dev).requires_grad_(grad)
    loss, nll = (fn or ctc_amd.blank_ctc_loss)(x, tgt.to(dev), Tb.to(dev), L.to(dev), blank=blank)
    if grad:
        loss.backward()
    torch.cuda.synchronize()
    return {"loss": float(loss.detach()), "nll": np_(nll).astype(np.float64),
            "grad": np_(x.grad) if grad else None}


def check(r, ref, label):
    """every assertion on one result of the loss (nll, loss, float32 grad) against reference(path, regime)"""
    lp, tgt, Tb, L = ref["inputs"]
    T, B, C = lp.shape
    fin, lpn = ref["fin"], np_(lp).astype(np.float64)
    nll, g32 = r["nll"], r["grad"]
    g = g32.astype(np.float64)
    err = float(np.abs(g[:, fin] - ref["grad"][:, fin]).max())
    nerr = float((np.abs(nll[fin] - ref["nll"][fin]) / np.maximum(1.0, np.abs(ref["nll"][fin]))).max())
    print("blank inputs %s: err %.3e err32 %.3e err/err32 %.3f bound %.3e max|grad_ref| %.3e nll_rel %.2e"
          % (label, err, ref["err32"], err / ref["err32"], ref["bound"], ref["gmax"], nerr))
    # nll and loss
    assert not np.isnan(nll).any() and np.array_equal(np.isinf(nll), ~fin) and (nll[~fin] > 0).all()
    assert nerr <= NLL_RTOL
    if fin.all():
        assert abs(r["loss"] - ref["loss"]) <= NLL_RTOL * max(1.0, abs(ref["loss"]))
    else:
        assert np.isinf(r["loss"]) and r["loss"] > 0
    # the exact parts of the gradient
    assert np.isfinite(g32).all()
    for b in range(B):
        assert np.abs(g32[int(Tb[b]):, b]).max(initial=0.0) == 0.0, "sample %d beyond T_b" % b
        if not fin[b]:
            assert np.abs(g32[:, b]).max() == 0.0, "sample %d has no alignment" % b
    assert (g32[np.isinf(lpn)] == 0.0).all()
    # accuracy
    assert err <= ref["bound"]
    # rows: the occupancy of a live row sums to 1
    for b in np.nonzero(fin)[0]:
        tb = int(Tb[b])
        got = g[:tb, b].sum(1) * (max(int(L[b]), 1) * B)
        assert np.abs(got - (np.exp(lpn[:tb, b]).sum(1) - 1.0)).max() <= 1e-5, "sample %d" % b
    return err


_results = {}


def result(dev, path, regime, schedule):
    """the loss on a case under a schedule, run once per module"""
    key = (path, regime, schedule)
    if key not in _results:
        _schedule(schedule)
        _results[key] = run_loss(dev, *reference(path, regime)["inputs"])
    return _results[key]


@pytest.mark.parametrize("run", RUNS, ids=_id)
def test_against_float64(dev, run):
    path, regime, schedule = run
    ref = reference(path, regime)
    r = result(dev, path, regime, schedule)
    check(r, ref, _id(run))
    f = run_loss(dev, *ref["inputs"], grad=False)               # forward only
    assert np.array_equal(np.isinf(f["nll"]), ~ref["fin"]) and not np.isnan(f["nll"]).any()
    fin = ref["fin"]
    assert (np.abs(f["nll"][fin] - r["nll"][fin]) <= 2e-6 * np.maximum(1.0, np.abs(r["nll"][fin]))).all()


@pytest.mark.parametrize("case", FORCED, ids=_id)
def test_schedules_agree(dev, case):
    """the pool gather (2) feeds the same chains the same rows as the loaders (1): bit for bit; the persistent launch
    against the three launches (beta' stored without its emission, row 2P+1 rebuilt from row 2P): within the bound"""
    ref = reference(*case)
    r0, r1, r2 = (result(dev, *case, s) for s in (0, 1, 2))
    assert np.array_equal(r2["grad"].view(np.int32), r1["grad"].view(np.int32))
    assert np.array_equal(r2["nll"], r1["nll"]) and r2["loss"] == r1["loss"]     # (+inf == +inf on the masked cases)
    d = float(np.abs(r1["grad"].astype(np.float64) - r0["grad"]).max())
    print("blank inputs %s: persistent against three launches %.3e, bound %.3e" % (_id(case), d, ref["bound"]))
    assert d <= ref["bound"]


# ---- the remaining call forms, on the masked case with float4 rows ---------------------------------------------
FORMS = ("k2", "masked")


@pytest.mark.parametrize("schedule", SCHEDULES["k2"])
def test_int32_targets(dev, schedule):
    ref = reference(*FORMS)
    lp, tgt, Tb, L = ref["inputs"]
    _schedule(schedule)
    check(run_loss(dev, lp, tgt.int(), Tb, L), ref, "k2-masked-%d int32 targets" % schedule)


@pytest.mark.parametrize("schedule", SCHEDULES["k2"])
def test_blank_is_last_class(dev, schedule):
    """blank = C-1: the same lattice with the classes rotated by one, so the same reference serves"""
    ref = reference(*FORMS)
    lp, tgt, Tb, L = ref["inputs"]
    _schedule(schedule)
    r = run_loss(dev, torch.roll(lp, -1, 2).contiguous(), tgt - 1, Tb, L, blank=lp.shape[2] - 1)
    r["grad"] = np.roll(r["grad"], 1, 2)
    check(r, ref, "k2-masked-%d blank=C-1" % schedule)


@pytest.mark.parametrize("schedule", SCHEDULES["k2"])
def test_strided_log_probs(dev, schedule):
    import ctc_amd
    ref = reference(*FORMS)
    lp, tgt, Tb, L = ref["inputs"]
    T, B, C = lp.shape
    wide = torch.randn(T, B, C + 12)
    wide[:, :, 4:4 + C] = lp
    xv = wide.to(dev)[:, :, 4:4 + C].requires_grad_(True)
    _schedule(schedule)
    loss, nll = ctc_amd.blank_ctc_loss(xv, tgt.to(dev), Tb.to(dev), L.to(dev))
    loss.backward()
    torch.cuda.synchronize()
    r = {"loss": float(loss.detach()), "nll": np_(nll).astype(np.float64), "grad": np_(xv.grad)}
    check(r, ref, "k2-masked-%d strided view" % schedule)


@pytest.mark.parametrize("schedule", SCHEDULES["k2"])
def test_module(dev, schedule):
    import ctc_amd
    ref = reference(*FORMS)
    m = ctc_amd.BlankCTC()
    base = result(dev, *FORMS, schedule)
    _schedule(schedule)
    r = run_loss(dev, *ref["inputs"],
                 fn=lambda x, t, il, tl, blank=0: (m(x, t, il, tl), torch.zeros(x.shape[1], device=x.device)))
    assert np.isinf(r["loss"]) and r["loss"] > 0
    assert np.array_equal(r["grad"].view(np.int32), base["grad"].view(np.int32))
    ctc_amd.check_status(dev)


# ---- outputs on feasible samples, against a recording ----------------------------------------------------------
def grad_digest(g):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(g, dtype=np.float32).tobytes()).digest(), dtype=np.uint8)


@pytest.mark.parametrize("run", RECORDED, ids=_id)
def test_feasible_samples_keep_their_bits(dev, run):
    """nll, loss and gradient bits on one diffuse all-feasible case per path (exact_case: inputs that every machine
    draws alike), against tests/golden/blank_loss_bits.npz -- recorded on an MI355X from the library as it was before
    the gradient rows of samples without an alignment were zeroed by their likelihood: that rule must not move a bit
    of a sample that has an alignment.  (The gradient is kept as its SHA-256: the rows themselves would be ~1 MB.)"""
    path, schedule = run
    rec = np.load(GOLDEN)
    key = "%s_%s" % (path, "auto" if schedule is None else schedule)
    _schedule(schedule)
    r = run_loss(dev, *exact_case(path))
    assert np.isfinite(r["nll"]).all()
    assert np.array_equal(r["nll"].astype(np.float32).view(np.int32), rec[key + "_nll"])
    assert np.array_equal(np.array([r["loss"]], dtype=np.float32).view(np.int32), rec[key + "_loss"])
    assert np.array_equal(grad_digest(r["grad"]), rec[key + "_grad_sha256"])
