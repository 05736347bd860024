"""The float64 training-step reference of tests/train_step_ref.py: its three losses against oracle/ctc_numpy in float64, and
the conditions each case must meet for tests/test_train_step_gpu.py to mean something -- the ReLU margin at every step, the
ragged lengths, the kernel family the table claims, a finite float32 yardstick -- and the float64 fact about label smoothing
behind a padded producer (runs without a GPU)."""
import numpy as np
import pytest
import torch

from oracle import ctc_numpy
from tests import train_step_ref as R
from tests.head_backward_ref import MARGIN
from tests.test_lattice_inputs_ref import plan  # noqa: F401 -- the fixture that asks ctc_amd_debug_noblank_plan
from tests.test_noblank_plan import CUS, F32, PS_PAIRS, Query

NAMES = list(R.CASES)


def test_constants_are_the_projects():
    from ctc_amd import producer
    from tests import lattice_inputs_ref, test_head_backward_gpu, test_parity_gpu
    assert R.PAD_LOGIT == producer.PAD_LOGIT
    assert R.NLL_RTOL == test_parity_gpu.NLL_RTOL == lattice_inputs_ref.NLL_RTOL
    assert R.GRAD_TOL == test_head_backward_gpu.TOL
    assert set(R.ENTRIES) == set(R.SEEDS) == set(NAMES)


def _oracle(case, series, b):
    Tb, L = b.Tb.numpy(), b.L.numpy()
    if case.loss == "noblank":
        return ctc_numpy.noblank_ctc(series, b.targets.numpy(), Tb, L, np.float64, label_smoothing=case.smoothing)
    if case.loss == "binary":
        return ctc_numpy.binary_ctc(series, b.y.numpy(), Tb, L, np.float64)
    return ctc_numpy.blank_ctc(ctc_numpy._log_softmax(series), b.targets.numpy(), Tb, L, np.float64, blank=0)


@pytest.mark.parametrize("name", NAMES)
def test_torch_losses_reproduce_the_oracle_in_float64(name):
    """loss, nll and d loss / d series of the differentiable torch losses against oracle/ctc_numpy on the case's own series"""
    case, r = R.CASES[name], R.reference(name)
    ref = r["ref"]
    o = _oracle(case, ref["series_cols"], r["batch"])
    assert abs(float(o["loss"]) - float(ref["loss"])) <= 1e-9
    assert np.abs(o["nll"] - ref["nll"]).max() <= 1e-9
    assert o["grad"].shape == ref["d_series"].shape and np.abs(o["grad"] - ref["d_series"]).max() <= 1e-9
    assert (ref["nll"] < R.NO_ALIGNMENT).all()               # every sample has an alignment
    if case.cols > case.C:                                   # the pad column: a constant, its gradient exactly 0
        assert (ref["series_cols"][:, :, case.C:] == R.PAD_LOGIT).all() and (ref["d_series"][:, :, case.C:] == 0).all()


@pytest.mark.parametrize("name", NAMES)
def test_no_relu_decision_hangs_on_a_rounding(name):
    """the seed recorded in SEEDS keeps every BatchNorm output of every float64 forward MARGIN away from 0"""
    m = R.margins(name)
    assert set(m) >= {"step"} and (name not in R.MULTI_STEP or set(m) == {"step", "accum1", "accum2", "eval", "sgd0", "sgd1", "sgd2"})
    assert min(m.values()) >= MARGIN, m
    for what in (("step", "two", "eval", "accum", "sgd") if name in R.MULTI_STEP else ("step",)):
        r = R.reference(name, what)                          # the runs the GPU tests compare against are those runs
        assert r["ref"]["ymin"].min() >= MARGIN and r["r32"]["ymin"].min() >= 0.5 * MARGIN


@pytest.mark.parametrize("name", NAMES)
def test_lengths_are_ragged_and_feasible(name):
    case = R.CASES[name]
    for index in range(3 if name in R.MULTI_STEP else 1):
        b = R.draw_batch(case, R.SEEDS[name], index)
        Tb, L = b.Tb.numpy(), b.L.numpy()
        assert Tb.shape == L.shape == (case.B,) and (Tb >= 1).all() and (Tb <= case.T).all() and (L <= case.S).all()
        assert Tb.max() == case.T and (Tb < case.T).any()
        assert (L == 1).any() and (L == min(case.S, case.T)).sum() >= 1
        if case.loss == "blank":                             # torch's feasibility: T_b >= L_b + adjacent repeats
            tg = b.targets.numpy()
            rep = np.array([(tg[i, 1:L[i]] == tg[i, :max(L[i] - 1, 0)]).sum() for i in range(case.B)])
            assert (L == 0).sum() == 1 and (rep > 0).sum() == 1 and (Tb >= L + rep).all()
            assert (tg[np.arange(case.S)[None, :] < L[:, None]] >= 1).all() and (tg < case.C).all()
        else:
            assert (L >= 1).all() and (L <= Tb).all()
            assert (L < Tb).any()                            # more than one alignment somewhere
        if case.loss == "noblank":
            tg = b.targets.numpy()
            live = np.arange(case.S)[None, :] < L[:, None]
            assert (tg[live] >= 0).all() and (tg[live] < case.C).all() and (tg[~live] == -1).all()
        if case.loss == "binary":                            # the rows hold duplicates; the dedup leaves L_b of them
            tg, ln = ctc_numpy.dedup_multihot_targets(b.rows.numpy(), case.exact_rows)
            assert np.array_equal(ln, L) and (L < case.S).any()
            assert np.array_equal(b.y.numpy(), np.clip(tg, 0, None).astype(np.float32))
            assert (b.y.numpy()[~(np.arange(case.S)[None, :] < L[:, None])] == 0).all()


@pytest.mark.parametrize("name", [n for n in NAMES if R.CASES[n].loss == "noblank"])
def test_noblank_loss_reaches_the_family_the_table_claims(plan, name):
    """ctc_amd_debug_noblank_plan on the series the producer hands over: [T,B,cols] float32, contiguous"""
    case = R.CASES[name]
    got = plan(Query(case.T, case.B, case.cols, case.S, dtype=F32, want_grad=True, smooth=case.smoothing is not None))
    assert got["family"] == R.FAMILY[name], (name, got)
    assert got["ps"] == int(name in R.PERSISTENT), (name, got)
    if got["ps"]:
        assert case.B > 2 * CUS and (got["n4"], got["n2"]) in PS_PAIRS and got["grid"] == CUS
    assert set(R.FAMILY) == {n for n in NAMES if R.CASES[n].loss == "noblank"}
    assert (R.FAMILY[name] == "r16") == (case.cols % 2 == 0)


@pytest.mark.parametrize("name", NAMES)
def test_float32_yardstick_is_finite_and_a_zero_gradient_cannot_pass(name):
    for what in (("step", "two", "accum", "sgd") if name in R.MULTI_STEP else ("step",)):
        r = R.reference(name, what)
        names = R.QUANTITIES if what in ("step", "two") else ("loss",) + R.GRADS[1:] + R.STATS if what == "accum" \
            else ("loss",) + R.PARAMS + R.STATS
        for q, (e32, bound, scale) in R.yardstick(r["ref"], r["r32"], names).items():
            assert np.isfinite(e32) and np.isfinite(bound) and np.isfinite(scale), (name, what, q)
            assert np.isfinite(r["r32"][q]).all() and np.isfinite(r["ref"][q]).all()
            if q.startswith("d_"):                           # the reference's gradient is larger than its bound
                assert scale > bound, (name, what, q, scale, bound)


def test_float64_loss_falls_over_three_sgd_steps():
    loss = R.reference("ref33_pad", "sgd")["ref"]["loss"]
    assert loss.shape == (3,) and loss[0] > loss[1] > loss[2]
    assert float(loss[0]) == float(R.reference("ref33_pad")["ref"]["loss"])


def test_second_consumer_changes_the_gradient_of_the_series():
    one, two = R.reference("ref33_pad")["ref"], R.reference("ref33_pad", "two")["ref"]
    T, C = R.CASES["ref33_pad"].T, R.CASES["ref33_pad"].C
    d = two["d_series"] - one["d_series"]
    assert np.abs(d[T - 1, :, :C]).max() > R.GRAD_TOL and (d[:T - 1] == 0).all() and (d[:, :, C:] == 0).all()
    for q in R.GRADS[1:]:                                    # a dropped second consumer shows in every parameter gradient
        assert np.abs(two[q] - one[q]).max() > 2.0 * R.GRAD_TOL, q


def test_label_smoothing_counts_the_pad_column_as_a_class():
    """The hole this file pins down: the smoothed emission b * sum_n lp[n] takes in the pad column's lp = -1e30, so behind
    LSTM_cell(pad_classes=True) every sample reports an nll of some frames times (1 - lambda) / (C + 1) 1e30 -- beyond the 1e12
    that means "no alignment" -- where the unpadded series gives an ordinary loss.  float64, T = 20, B = 4, C = 33, 0.9."""
    T, B, C, S, lam = 20, 4, 33, 5, 0.9
    g = torch.Generator().manual_seed(5)
    x = (torch.rand(T, B, C, generator=g) * 2 - 1).double().numpy()
    Tb, L = np.array([20, 11, 16, 20]), np.array([5, 1, 3, 4])
    lab = torch.randint(0, C, (B, S), generator=g).numpy()
    lab[np.arange(S)[None, :] >= L[:, None]] = -1
    padded = np.concatenate([x, np.full((T, B, 1), R.PAD_LOGIT)], axis=2)
    plain = ctc_numpy.noblank_ctc(x, lab, Tb, L, np.float64, label_smoothing=lam)
    hole = ctc_numpy.noblank_ctc(padded, lab, Tb, L, np.float64, label_smoothing=lam)
    assert (plain["nll"] < 1e3).all() and float(plain["loss"]) < 1e3
    assert (hole["nll"] >= R.NO_ALIGNMENT).all() and float(hole["loss"]) > 1e27
    frames = hole["nll"] / ((1.0 - lam) / (C + 1) * 1e30)    # the pad column's share of one frame's emission, counted 1 .. T_b times
    assert (frames >= 1.0 - 1e-10).all() and (frames <= Tb + 1e-10).all()
    # without smoothing the pad column changes nothing: that is what pad_classes promises
    a = ctc_numpy.noblank_ctc(x, lab, Tb, L, np.float64)
    b = ctc_numpy.noblank_ctc(padded, lab, Tb, L, np.float64)
    assert np.abs(a["nll"] - b["nll"]).max() <= 1e-9 and np.abs(a["grad"] - b["grad"][:, :, :C]).max() <= 1e-12
