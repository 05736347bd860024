"""The float64 reference of the label-smoothed no-blank loss (tests/smoothing_ref.py) against finite differences, against
oracle/ctc_numpy in float64 and against its own invariances, and the conditions each case must meet for
tests/test_smoothing_gpu.py to mean something (runs without a GPU)."""
import numpy as np
import pytest
import torch

from tests.helpers import np_
from tests.lattice_inputs_ref import NLL_RTOL, NOBLANK_SHAPES, R16
from tests.lattice_inputs_ref import reference as plain_reference
from tests.smoothing_ref import (CASES, OFFSET, PATHS, REGIMES, case_id, coefficients, inputs, lams, port, reference,
                                 smoothed_ref)

ids = case_id


def test_the_cases_are_the_r16_forms():
    assert PATHS == R16 == ["r16", "r16_n4", "r16_n2", "r16_c158", "r16_s31", "r16_t168", "r16_ps"]
    assert max(NOBLANK_SHAPES[p][1] for p in PATHS) == 520 and NOBLANK_SHAPES["r16_ps"] == (24, 520, 10, 6)
    assert len(CASES) == 7 * (4 * 4 + 2 + 1)
    for p in PATHS:
        C = NOBLANK_SHAPES[p][2]
        assert lams(p, "masked") == (0.9, 0.5)                   # a > 0 wherever a logit is -inf
        signs = [np.sign(round(coefficients(lam, C)[0], 12)) for lam in lams(p, "aligned")]
        assert signs == [1, 1, 0, -1]


@pytest.mark.parametrize("lam", [0.9, 0.2, 0.0], ids=["a>0", "a=0", "a<0"])
def test_closed_form_gradient_against_finite_differences(lam):
    T, B, C, S = 5, 2, 4, 3
    assert [1, 0, -1][[0.9, 0.2, 0.0].index(lam)] == np.sign(round(coefficients(lam, C)[0], 12))
    g = torch.Generator().manual_seed(3)
    x = torch.randn(T, B, C, generator=g, dtype=torch.float64).numpy() * 2.0
    lab = np.array([[1, 3, 1], [0, 2, -1]], np.int32)
    Tb, L = np.array([5, 4]), np.array([3, 2])
    r = smoothed_ref(x, lab, Tb, L, lam)
    assert r["fin"].all()
    h, fd = 1e-5, np.zeros_like(x)
    for i in np.ndindex(*x.shape):
        xp, xm = x.copy(), x.copy()
        xp[i] += h
        xm[i] -= h
        fd[i] = (smoothed_ref(xp, lab, Tb, L, lam)["nll"].mean() - smoothed_ref(xm, lab, Tb, L, lam)["nll"].mean()) / (2 * h)
    assert np.abs(fd - r["grad"]).max() <= 1e-8, np.abs(fd - r["grad"]).max()
    assert np.abs(r["grad"][4, 1]).max() == 0.0 and np.abs(r["grad"]).max() > 1e-2


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_agrees_with_the_oracle_in_float64(case):
    """wherever oracle/ctc_numpy is defined: every sample outside `masked`, the samples without a -inf logit there"""
    r = reference(*case)
    x, lab, Tb, L = r["inputs"]
    p = port(x, lab, Tb, L, case[2], np.float64)
    ok = r["fin"] & np.isfinite(p["nll"]) & (p["nll"] < 1e12)
    if case[1] != "masked":
        assert ok.all()
    assert ok.any()
    assert (np.abs(r["nll"][ok] - p["nll"][ok]) <= 1e-9 * np.maximum(1.0, np.abs(r["nll"][ok]))).all()
    assert np.abs(r["grad"][:, ok] - p["grad"][:, ok]).max() <= 1e-9


@pytest.mark.parametrize("path", PATHS)
def test_lam_one_is_the_plain_reference(path):
    r, q = reference(path, "aligned", 1.0), plain_reference("noblank", path, "aligned")
    assert np.array_equal(r["nll"], q["nll"]) and np.array_equal(r["grad"], q["grad"])


@pytest.mark.parametrize("case", [c for c in CASES if c[1] == "offset"], ids=ids)
def test_offset_leaves_the_loss_alone(case):
    """a common offset is softmax-invariant: in float64, the float64 logits shifted in float64, nll moves by < 1e-9
    relative; the float32 inputs of the `offset` case (rounded once more after the shift) are what the kernel gets"""
    path, _, lam = case
    x, lab, Tb, L, _ = inputs(path, "aligned")
    base = reference(path, "aligned", lam)
    shifted = smoothed_ref(np_(x).astype(np.float64) + OFFSET, lab, Tb, L, lam)
    assert (np.abs(shifted["nll"] - base["nll"]) <= 1e-9 * np.maximum(1.0, np.abs(base["nll"]))).all()
    assert np.abs(shifted["grad"] - base["grad"]).max() <= 1e-9
    xo = np_(inputs(path, "offset")[0])
    assert xo.dtype == np.float32 and np.abs(xo - OFFSET).max() < 20.0
    C = xo.shape[2]
    assert abs(float(xo[0, 0].astype(np.float32).sum(dtype=np.float32)) - C * OFFSET) < 20.0 * C   # a sum near C x 3e4


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_feasibility_is_what_the_case_was_built_to_contain(case):
    """every batch holds a feasible sample; `masked`: only kind c (no -inf, no pad logit in a live row) keeps an alignment,
    everything else is feasible throughout"""
    r = reference(*case)
    x, _, Tb, _ = r["inputs"]
    fin = r["fin"]
    assert fin.any()
    if case[1] == "masked":
        assert (~fin).any()
        assert np.array_equal(fin, np.array([k == "c" for k in r["kinds"]]))
        xn = np_(x)
        assert np.isneginf(xn).any() and coefficients(case[2], xn.shape[2])[0] > 0
    else:
        assert fin.all() and np.isfinite(np_(x)).all()
    assert np.array_equal(np.isinf(r["nll"]), ~fin) and not np.isnan(r["nll"]).any()
    assert np.isfinite(r["grad"]).all()
    for b in range(x.shape[1]):
        assert (r["grad"][int(Tb[b]):, b] == 0).all() and (fin[b] or (r["grad"][:, b] == 0).all())


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_float32_reaches_the_tolerances(case):
    """the float32 port keeps nll within NLL_RTOL, so the kernel can be asked to; a zero or stale gradient must not
    pass: max |grad| >= 10 x the bound -- except on ties at a = 0, where the gradient (a / C per element) IS zero"""
    r = reference(*case)
    assert r["err32_nll"] <= NLL_RTOL, r["err32_nll"]
    if case[1] == "ties" and case[2] not in (0.9, 0.5, 0.0, 1.0):
        assert r["gmax"] <= 1e-12
    else:
        assert r["gmax"] >= 10.0 * r["bound"], (r["gmax"], r["bound"], r["err32"])


def test_regimes():
    assert REGIMES == ("aligned", "wrongpeak", "masked", "ties", "offset")
