"""The scalar `loss` of every loss launch against tests/batch_sum_ref.py, on the MI355X: the packed fixed-point sum
(`publish_and_reduce_sum`, no-blank and binary, B <= 4095) and the arrival-ticket sum (`ticket_and_reduce`: B > 4095 and
the blank loss) at every call site, in every value regime, and with the state one launch leaves for the next.

The reference takes the per-sample nll THE SAME LAUNCH returned and says what the loss must be (include/ctc_amd.h), so a
failure here is the reduction's, not the lattice's; the lattice at the new batch sizes is pinned separately
(test_nll_and_gradient_at_large_batches).  Inputs: one label per sample, so the nll is a closed form of one number per
sample that the test chooses (tests/batch_sum_ref.py; checked against the float64 oracle in tests/test_batch_sum_ref.py).

Call sites (ctc_amd/csrc) by shape (T, C, S); tests/test_batch_sum_ref.py asserts the no-blank rows against the plan
function, the binary rows follow binary_plan() (K = 1: streamed for T <= 160 and C <= 192, else pipelined for T <= 168
and C <= 256; K > 1: MFMA; C > 256: fused) and tests/test_binary_plan.py asserts them against it at every batch size
below: they depend on kFlowMaxT = 160 (binary_flow.hpp) and its three column chunks of 64, on kPipeMaxT = 168 and
kBinRows * kBinWaves = 160 (binary.hip), on lane_states() (K = 2 from S = 65), on the C <= 256 test of the fast path and
on each kernel's LDS need staying within kMaxLds at these shapes -- a change of one of them can move a row to another
kernel, that test then fails, and this table has to follow:

    no-blank  (8, 8, 2)      noblank_r16.hpp, one sample per workgroup (B <= 512, and every forward-only call)
                             noblank_r16.hpp persistent (B > 512 with a gradient): one workgroup publishes many samples
              (8, 9, 2)      noblank_xr.hpp (two per CU for B > 256)
              (168, 9, 40)   noblank_pipe.hpp          (100, 9, 40), B > 256: noblank_pipe.hpp, two per CU
              (169, 8, 2)    noblank.hip fused, K = 1  (20, 8, 70): K = 2   (20, 8, 130): K = 4
              (212, 9, 64)   noblank.hip fused, lattice in the workspace (behind the list of non-fitting samples)
              (8, 258, 2)    noblank.hip fused, C > 256: the generic (strided) emission rows
    binary    (100, 8, 2)    binary_flow.hpp (streamed)
              (161, 8, 2), (100, 200, 2)   binary.hip pipelined (T > 160; four column chunks)
              (100, 8, 70)   binary.hip MFMA, K = 2    (100, 257, 2): binary.hip fused
    blank     (8, 8, 2)      blank.hip, three launches (gather / chain / gradient; the gradient grid is capped at 2048
                             workgroups from T B > 8192)
              (130, 8, 2)    blank.hip persistent launch, forced      (8, 8, 300): blank_wide.hpp

Every tolerance is the header's own bound (batch_sum_ref.Expected) or an existing constant of tests/test_parity_gpu.py.

Measured on an MI355X (gfx950): every loss of every case is the predicted one -- bit for bit wherever all values fit,
ties included -- and every permuted batch returned the same nll bits and the same loss.  Examples at B = 4095 on r16:
tiny |loss - mean| 1.1e-6 (bound 1.5e-5), straddling 1.2e-4 (9.8e-4); the ticket form at B = 4097: tiny 2.6e-11 (1.3e-9),
straddling 9.7e-4 (3.6e-2).  What the tests found outside the sum: noblank_xr.hpp reported a sample with a NaN logit as
"no alignment" (nll = 1e13, a finite loss) where the header promises a NaN loss; its clamp, and the same clamp of the
pipelined and fused kernels (fmaxf answers its other operand for a NaN), now keep the NaN.  The blank loss drops a NaN
log-prob in its max-based log-sum-exp; the header now says so, and test_one_nan_logit says what is held there.
"""
import numpy as np
import pytest
import torch

from oracle import ctc_c
from tests import batch_sum_ref as ref
from tests.helpers import np_, synth_blank

pytestmark = pytest.mark.gpu

NLL_RTOL = 1e-5                                   # tests/test_parity_gpu.py
SWEEP_B = (1, 2, 15, 16, 17, 31, 33, 255, 256, 257, 511, 513, 1023, 1025, 2049, 4094, 4095, 4096, 4097, 5000)
HEAVY_B = (1, 17, 257, 513, 4095, 4096)
SITES = {
    # name: (family, (T, C, S), batch sizes, blank schedule or None)
    "noblank-r16": ("noblank", (8, 8, 2), SWEEP_B, None),
    "noblank-xr": ("noblank", (8, 9, 2), SWEEP_B, None),
    "noblank-fused_k1": ("noblank", (169, 8, 2), SWEEP_B, None),
    "noblank-pipelined": ("noblank", (168, 9, 40), HEAVY_B, None),
    "noblank-pipelined_dual": ("noblank", (100, 9, 40), (257, 513, 4095, 4096), None),
    "noblank-fused_k2": ("noblank", (20, 8, 70), HEAVY_B, None),
    "noblank-fused_k4": ("noblank", (20, 8, 130), HEAVY_B, None),
    "noblank-glb": ("noblank", (212, 9, 64), (1, 17, 257, 513), None),
    "noblank-fused_c": ("noblank", (8, 258, 2), (17, 257), None),
    "binary-flow": ("binary", (100, 8, 2), HEAVY_B, None),
    "binary-pipe_t": ("binary", (161, 8, 2), HEAVY_B, None),
    "binary-pipe_c": ("binary", (100, 200, 2), HEAVY_B, None),
    "binary-mfma_k2": ("binary", (100, 8, 70), HEAVY_B, None),
    "binary-fused": ("binary", (100, 257, 2), HEAVY_B, None),
    "blank-three": ("blank", (8, 8, 2), HEAVY_B, 0),
    "blank-persistent": ("blank", (130, 8, 2), (1, 17, 64), 1),
    "blank-wide": ("blank", (8, 8, 300), (1, 17, 257), None),
}
RAGGED_LO = {"noblank": None, "binary": 95, "blank": None}     # (binary: 100 per frame at most, 8192 needs T_b >= 82)


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


def _fn(family):
    import ctc_amd
    return {"noblank": ctc_amd.noblank_ctc_loss, "binary": ctc_amd.binary_ctc_loss, "blank": ctc_amd.blank_ctc_loss}[family]


class Device:
    """a batch_sum_ref.Batch on the device"""

    def __init__(self, batch, dev, dtype=None):
        self.B = batch.x.shape[1]
        self.x = torch.from_numpy(batch.x).to(dev)
        if dtype is not None:
            self.x = self.x.to(dtype)
        self.tgt, self.Tb, self.L = (torch.from_numpy(a).to(dev) for a in (batch.tgt, batch.Tb, batch.L))


def enqueue(family, d, grad, batch_total=None, x=None):
    """one call, nothing synchronised -> (loss, nll, x) device tensors"""
    x = (d.x if x is None else x).detach().requires_grad_(grad)
    loss, nll = _fn(family)(x, d.tgt, d.Tb, d.L, batch_total=batch_total)
    if grad:
        loss.backward()
    return loss, nll, x


def fetch(out, B, batch_total=None, keep_grad=False):
    loss, nll, x = out
    return {"loss": np.float32(np_(loss)), "nll": np_(nll), "grad": np_(x.grad.float()) if keep_grad else None,
            "scale": np.float32(1.0 / (B if batch_total is None else batch_total))}


def run(family, d, grad, batch_total=None, x=None, keep_grad=False):
    out = enqueue(family, d, grad, batch_total, x)
    torch.cuda.synchronize()
    return fetch(out, d.B, batch_total, keep_grad)


def check(family, r, batch, what):
    """the launch's loss against what its own nll and the header say -> the Expected it was held to"""
    B = len(batch.L)
    e = ref.expected_loss(family, r["nll"], B, r["scale"], L=batch.L)
    wrong = ref.check_loss(r["loss"], e)
    print("%s: B=%d loss %.9g predicted %.9g |loss - mean| %.3g bound %.3g all_fit=%s"
          % (what, B, r["loss"], e.value, abs(float(r["loss"]) - e.mean), e.bound, e.all_fit))
    assert not wrong, (what, B, wrong)
    return e


def sweep_targets(B, family="noblank"):
    """every value fits: ordinary ones and, on every third sample, small ones.  The binary kernels form the emission as a
    difference of two sums over the classes of magnitude C |x| each, whose fp32 residue on these constant inputs reaches
    C |x| T 2^-24 (9e-3 at C = 200, |x| = 8, T = 100): an nll asked for below that can come back negative -- a value
    for the list, not for the fixed-point sum -- so the small values of the binary sites start at 0.05."""
    b = np.arange(B)
    small = 0.05 * (1.0 + b % 5) if family == "binary" else ref.regime_targets("tiny", B)
    return np.where(b % 3 == 0, small, ref.regime_targets("ordinary", B))


def build(family, shape, B, targets, ragged=True, **kw):
    T, C, S = shape
    Tb = ref.ragged_lengths(B, T, RAGGED_LO[family]) if ragged else T
    return ref.BUILDERS[family](T, C, S, Tb, targets, **kw)


def permuted(batch, perm):
    return ref.Batch(np.ascontiguousarray(batch.x[:, perm]), batch.tgt[perm], batch.Tb[perm], batch.L[perm],
                     batch.nll64[perm], batch.infeasible[perm])


CASES = [(name, B) for name, site in SITES.items() for B in site[2]]


# ------------------------------------------------------------------------------------------------ a. the B sweep
@pytest.mark.parametrize("name,B", CASES, ids=["%s-%d" % c for c in CASES])
def test_batch_sweep_at_every_call_site(dev, name, B):
    """All values fit.  With and without a gradient (the forward-only launches publish from other code positions), one
    call with batch_total = 3 B: the contract bound, and for B <= 4095 the loss bit for bit as predicted from the nll.
    A permuted batch: where its nll are the same bits, so is the loss ("order-independent")."""
    import ctc_amd
    family, shape, _, schedule = SITES[name]
    if schedule is not None:
        ctc_amd.set_blank_schedule(schedule)
    batch = build(family, shape, B, sweep_targets(B, family))
    d = Device(batch, dev)
    packed = family != "blank" and B <= ref.ACC_MAX_B
    got = {}
    for grad, total in ((True, None), (False, None), (True, 3 * B)):
        r = run(family, d, grad, total)
        what = "%s %s%s" % (name, "grad" if grad else "forward", "" if total is None else " batch_total=3B")
        assert np.isfinite(r["nll"]).all() and (r["nll"] < ref.ACC_LIMIT).all() and (r["nll"] >= 0).all(), what
        e = check(family, r, batch, what)
        assert e.all_fit == packed, what
        got[grad, total] = r
    if packed:
        perm = np.random.RandomState(B).permutation(B)
        pb = permuted(batch, perm)
        r, p = got[True, None], run(family, Device(pb, dev), True)
        check(family, p, pb, name + " permuted")
        if np.array_equal(p["nll"], r["nll"][perm]):
            assert p["loss"] == r["loss"], (name, B)
        else:
            print("%s B=%d: the permuted batch's nll differ in %d samples: nothing asserted about the order"
                  % (name, B, (p["nll"] != r["nll"][perm]).sum()))


@pytest.mark.parametrize("B", SWEEP_B)
def test_bf16_loss_is_the_fp32_loss_on_the_same_values(dev, B):
    """r16 shapes, 2-byte logits: nll and loss bit for bit those of the fp32 call on x.float() (include/ctc_amd.h), and
    the loss as predicted"""
    batch = build("noblank", (8, 8, 2), B, sweep_targets(B))
    d = Device(batch, dev, torch.bfloat16)
    for grad in (True, False):
        lo = run("noblank", d, grad)
        hi = run("noblank", d, grad, x=d.x.float())
        check("noblank", lo, batch, "bf16 %s" % ("grad" if grad else "forward"))
        assert np.array_equal(lo["nll"], hi["nll"]) and lo["loss"] == hi["loss"], (B, grad)


# ------------------------------------------------------------------------------------------------ b. the regimes
REGIME_SITES = {"noblank-r16": (17, 257, 513, 4095, 4097), "noblank-xr": (17, 257, 513, 4095),
                "binary-flow": (17, 257, 513, 4095, 4097), "blank-three": (17, 257, 513, 4095)}
REGIME_CASES = [(name, B) for name, bs in REGIME_SITES.items() for B in bs]
# the NaN case also at every other no-blank call site: each builds its emission from the row's log-sum-exp on its own
NAN_SITES = {"noblank-pipelined": (17, 257), "noblank-pipelined_dual": (257,), "noblank-fused_k1": (17, 257),
             "noblank-fused_k2": (17, 257), "noblank-fused_k4": (17, 257), "noblank-glb": (17, 257), "noblank-fused_c": (17, 257)}
NAN_CASES = REGIME_CASES + [(name, B) for name, bs in NAN_SITES.items() for B in bs]


def regime_batches(family, shape, B):
    """-> [(regime name, Batch)]: section 2 of the plan, the NaN case apart"""
    out = []
    for regime in ("tiny", "ordinary"):
        out.append((regime, build(family, shape, B, ref.regime_targets(regime, B))))
    out.append(("straddling", build(family, shape, B, ref.regime_targets("straddling", B), ragged=False)))
    ordinary = ref.regime_targets("ordinary", B)
    for k in sorted({1, B // 2, B}):
        idx = np.arange(B)[:k] if k == B else (np.arange(k) * (B // k) + B // (2 * k)) % B
        out.append(("no alignment (lengths) x%d" % k, build(family, shape, B, ordinary, no_alignment=idx)))
        if family != "binary":                      # (binary: a +-inf logit saturates the BCE at 100, it masks nothing)
            out.append(("no alignment (masked) x%d" % k, build(family, shape, B, ordinary, masked=idx)))
    b = np.arange(B)
    kw = dict(no_alignment=b[b % 11 == 5])
    if family != "binary":
        kw["masked"] = b[b % 13 == 7]
    out.append(("mixed", build(family, shape, B, ref.regime_targets("mixed", B), **kw)))
    return out


@pytest.mark.parametrize("name,B", REGIME_CASES, ids=["%s-%d" % c for c in REGIME_CASES])
def test_value_regimes(dev, name, B):
    """tiny / ordinary / straddling 8192 / no alignment at k = 1, B/2, B of the samples by both routes / all of it mixed
    over every shard: the loss the header defines for the nll the launch returned (B = 4097: the ticket form with 1e13
    and >= 8192 values; the blank loss: +inf).  Launches with a gradient (B > 512 on r16: the persistent form)."""
    import ctc_amd
    family, shape, _, schedule = SITES[name]
    if schedule is not None:
        ctc_amd.set_blank_schedule(schedule)
    for regime, batch in regime_batches(family, shape, B):
        r = run(family, Device(batch, dev), True, keep_grad=True)
        what = "%s %s" % (name, regime)
        bad = batch.infeasible
        assert not np.isnan(r["nll"]).any(), what
        assert (r["nll"][bad] >= ref.INFEASIBLE).all() and (r["nll"][~bad] < ref.INFEASIBLE).all(), what
        if regime == "straddling":
            assert (r["nll"] < ref.ACC_LIMIT).sum() >= B // 4 and (r["nll"] >= ref.ACC_LIMIT).sum() >= B // 4, what
        if regime.endswith("x%d" % B) and family == "blank":
            assert np.isposinf(r["loss"]), what
        e = check(family, r, batch, what)
        if regime == "ordinary":
            assert e.all_fit == (family != "blank" and B <= ref.ACC_MAX_B)
        if bad.any():
            assert np.abs(r["grad"][:, bad]).max() == 0.0, what


@pytest.mark.parametrize("name,B", NAN_CASES, ids=["%s-%d" % c for c in NAN_CASES])
def test_one_nan_logit(dev, name, B):
    """NaN logits are outside the lattice's contract, but the loss is then NaN (include/ctc_amd.h, no-blank and binary):
    that sample's nll is NaN, every other nll is bit for bit that of the batch without the NaN, and the next launch on
    the workspace is right.  The blank loss promises nothing for a NaN log-prob (its max-based log-sum-exp drops it: the
    sample reports +inf or, where other paths avoid the cell, a finite nll); there the loss must still be what the
    returned nll say, the other samples untouched and the next launch right."""
    import ctc_amd
    family, shape, _, schedule = SITES[name]
    if schedule is not None:
        ctc_amd.set_blank_schedule(schedule)
    j = B // 2
    clean = build(family, shape, B, ref.regime_targets("mixed", B))
    dirty = build(family, shape, B, ref.regime_targets("mixed", B), nan=[j])
    dc, dd = Device(clean, dev), Device(dirty, dev)
    first = run(family, dc, True)
    r = run(family, dd, True)
    again = run(family, dc, True)
    if family != "blank":
        assert np.isnan(r["loss"]) and np.isnan(r["nll"][j]), name
    keep = np.arange(B) != j
    assert np.array_equal(r["nll"][keep], first["nll"][keep]), name
    check(family, r, dirty, name + " one NaN")
    check(family, again, clean, name + " after the NaN")
    assert np.array_equal(again["nll"], first["nll"]), name
    if family != "blank" and B <= ref.ACC_MAX_B:
        assert again["loss"] == first["loss"], name


# ------------------------------------------------------------------------------------------------ c. nll and gradient
@pytest.mark.parametrize("name,B", [("noblank-r16", 4097), ("noblank-r16", 5000), ("noblank-xr", 4097), ("noblank-xr", 5000),
                                    ("binary-flow", 4097), ("binary-flow", 5000)])
def test_nll_and_gradient_at_large_batches(dev, name, B):
    """beyond the batch sizes the parity tests run: nll against the closed form, the gradient against its closed form
    scale (softmax - onehot) (no-blank) or the float64 oracle (binary); nll at NLL_RTOL, the gradient at the suite's bounds
    in the form that keeps shrinking with the batch, 2e-6 * 256 / B (test_noblank_r16_small_shape_sweep) and
    2e-7 * 256 / B: the largest gradient element is 1 / B; rows beyond T_b and samples without an alignment exactly zero.
    Measured on the MI355X: nll 2.4e-6 (r16), 4.4e-6 (xr), 1.4e-6 (binary) relative; gradient at B = 4097 3.6e-11 / 3.0e-11
    (bound 1.25e-7) and 5.4e-12 (binary, bound 1.25e-8).  On the
    CONSTANT logits of batch_sum_ref.binary_batch the streamed binary kernel's nll is 2.4e-5 off at nll = 1 (x = 4.6 on
    all 8 classes of all 100 frames: one rounding error of its emission, 2.3e-7, a hundred times) -- the reason why the
    binary case draws random logits; the sum tests take the nll as returned and do not depend on it."""
    family, shape, _, _ = SITES[name]
    T, C, S = shape
    b = np.arange(B)
    if family == "noblank":
        batch = build(family, shape, B, sweep_targets(B), no_alignment=b[b % 97 == 11])
    else:                                           # (random logits: batch_sum_ref.binary_random_batch says why)
        batch = ref.binary_random_batch(T, C, S, ref.ragged_lengths(B, T, RAGGED_LO[family]), B, no_alignment=b[b % 97 == 11])
    r = run(family, Device(batch, dev), True, keep_grad=True)
    ok = ~batch.infeasible
    assert (r["nll"][~ok] >= ref.INFEASIBLE).all()
    err = np.abs(r["nll"][ok] - batch.nll64[ok]) / np.maximum(1.0, batch.nll64[ok])
    print("%s B=%d: nll rel err %.3g" % (name, B, err.max()))
    assert err.max() <= NLL_RTOL
    check(family, r, batch, name)
    live = (np.arange(T)[:, None] < batch.Tb[None, :]) & ok[None, :]
    assert np.abs(r["grad"][~live]).max() == 0.0
    if family == "noblank":
        x = batch.x.astype(np.float64)
        p = np.exp(x - x.max(axis=2, keepdims=True))
        p /= p.sum(axis=2, keepdims=True)
        p[:, b, batch.tgt[:, 0]] -= 1.0
        want, tol = np.where(live[:, :, None], p / B, 0.0), 2e-6 * 256.0 / B
    else:
        want = ctc_c.binary_ctc(batch.x, batch.tgt, batch.Tb, batch.L, np.float64, threads=8)["grad"]
        tol = 2e-7 * 256.0 / B
    gerr = np.abs(r["grad"] - want).max()
    print("%s B=%d: grad err %.3g (bound %.3g)" % (name, B, gerr, tol))
    assert gerr <= tol


@pytest.mark.parametrize("B", [257, 600, 4097])
def test_blank_nll_and_gradient_at_large_batches(dev, B):
    """the three launches beyond B = 64 (gather and chain grids of B workgroups, the gradient grid capped at 2048 from
    B = 1025 on): L_b = 0 and L_b = 1 samples, ragged T_b, three samples without an alignment, against the float64 oracle
    with the bounds of test_blank_vs_oracle_shapes"""
    import ctc_amd
    ctc_amd.set_blank_schedule(0)
    T, C, S = 8, 8, 2
    lp, tgt, _, _ = synth_blank(B, T, B, C, S)
    Tb = torch.from_numpy(ref.ragged_lengths(B, T, 1))
    L = torch.arange(B) % 2
    for b in (5, B // 2, B - 1):
        L[b], Tb[b] = 2, 1
    o = ctc_c.blank_ctc(np_(lp), np_(tgt), np_(Tb), np_(L), np.float64, threads=8)
    batch = ref.Batch(np_(lp), np_(tgt), np_(Tb), np_(L), o["nll"], ~np.isfinite(o["nll"]))
    assert batch.infeasible.sum() == 3
    r = run("blank", Device(batch, dev), True, keep_grad=True)
    fin = ~batch.infeasible
    assert (np.isinf(r["nll"]) == ~fin).all() and np.isposinf(r["loss"])
    assert np.abs(r["nll"][fin] - o["nll"][fin]).max() <= 1e-5 * max(1.0, np.abs(o["nll"][fin]).max())
    gerr = np.abs(r["grad"][:, fin] - o["grad"][:, fin]).max()
    print("blank B=%d: grad err %.3g (bound %.3g)" % (B, gerr, 2e-6 * 64.0 / B))
    assert gerr < 2e-6 * 64.0 / B
    live = (np.arange(T)[:, None] < np_(Tb)[None, :]) & fin[None, :]
    assert np.abs(r["grad"][~live]).max() == 0.0
    # the same batch without the three: a finite loss, as the header's mean_b(nll_b / max(L_b, 1))
    keep = np.nonzero(fin)[0]
    sub = ref.Batch(batch.x[:, keep].copy(), batch.tgt[keep], batch.Tb[keep], batch.L[keep], batch.nll64[keep], batch.infeasible[keep])
    rs = run("blank", Device(sub, dev), True)
    check("blank", rs, sub, "blank-three feasible")
    assert np.array_equal(rs["nll"], r["nll"][keep])


# ------------------------------------------------------------------------------------------------ d. state between launches
def state_sequence(family, shape, sizes):
    """all fit / mixed with 40 not fitting / none fits / all fit, smaller / the ticket form / all fit, small"""
    b0, b1, big, b2 = sizes
    over = np.arange(40) * (b0 // 40) + 3
    mixed = ref.regime_targets("ordinary", b0)
    mixed[over[::2]] = ref.ACC_LIMIT + 50.0 + np.arange(20)
    return [build(family, shape, b0, sweep_targets(b0, family)),
            build(family, shape, b0, mixed, ragged=False, no_alignment=over[1::2]),
            build(family, shape, b0, ref.regime_targets("ordinary", b0), no_alignment=np.arange(b0)),
            build(family, shape, b1, sweep_targets(b1, family)),
            build(family, shape, big, ref.regime_targets("mixed", big), ragged=False),
            build(family, shape, b2, sweep_targets(b2, family))]


@pytest.mark.parametrize("name,grad,sizes", [("noblank-r16", False, (257, 33, 4097, 17)), ("noblank-r16", True, (1025, 513, 4097, 600)),
                                             ("binary-flow", True, (257, 33, 4097, 17))], ids=["r16", "r16_ps", "binary_flow"])
def test_state_left_for_the_next_launch(dev, name, grad, sizes):
    """six launches back to back on one stream and ONE workspace (sized by a first launch of the largest batch), nothing
    synchronised in between: shard words, top word, list length and ticket are put back by each launch's last workgroup,
    so a stale one shows in the loss of the launch after it.  (r16 without a gradient: one sample per workgroup at every
    B; with one and B > 512: the persistent form.)"""
    import ctc_amd
    family, shape, _, _ = SITES[name]
    batches = state_sequence(family, shape, sizes)
    ds = [Device(bt, dev) for bt in batches]
    check(family, run(family, ds[4], grad), batches[4], name + " first")            # (allocates the largest workspace)
    outs = [enqueue(family, d, grad) for d in ds]
    torch.cuda.synchronize()
    assert (~ref.fits(np_(outs[1][1]))).sum() == 40 and not ref.fits(np_(outs[2][1])).any()
    for i, (out, bt) in enumerate(zip(outs, batches)):
        check(family, fetch(out, len(bt.L)), bt, "%s launch %d" % (name, i + 1))
    assert ctc_amd.workspace_status() == 0


@pytest.mark.parametrize("name,B", [("noblank-r16", 257), ("noblank-r16", 1025), ("binary-flow", 257)], ids=["r16", "r16_ps", "binary_flow"])
def test_state_under_graph_replay(dev, name, B):
    """one forward + backward call captured after a warm-up, replayed with the logits rewritten in place: the batch goes
    all fitting -> mixed (values >= 8192 and, no-blank, masked labels) -> all fitting"""
    import ctc_amd
    family, shape, _, _ = SITES[name]
    b = np.arange(B)
    kw = dict(masked=b[b % 13 == 7]) if family == "noblank" else {}
    fit = build(family, shape, B, sweep_targets(B, family), ragged=False)
    mixed = build(family, shape, B, ref.regime_targets("mixed", B), ragged=False, **kw)
    d = Device(fit, dev)
    xs = d.x.clone().requires_grad_(True)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                     # warm-up on the capture stream (workspace, grads)
        for _ in range(2):
            xs.grad = None
            loss, nll = _fn(family)(xs, d.tgt, d.Tb, d.L)
            loss.backward()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    xs.grad = None
    with torch.cuda.graph(g):
        loss, nll = _fn(family)(xs, d.tgt, d.Tb, d.L)
        loss.backward()
    for i, bt in enumerate((fit, mixed, fit)):
        with torch.no_grad():
            xs.copy_(torch.from_numpy(bt.x).to(dev))
        g.replay()
        torch.cuda.synchronize()
        r = {"loss": np.float32(np_(loss)), "nll": np_(nll), "scale": np.float32(1.0 / B)}
        e = check(family, r, bt, "%s replay %d" % (name, i + 1))
        assert e.all_fit == (i != 1)
        assert np.isfinite(np_(xs.grad)).all()
    assert ctc_amd.workspace_status() == 0
