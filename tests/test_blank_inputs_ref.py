"""The float64 blank-CTC gradient reference of tests/blank_grad_ref.py against torch's float64 CPU kernel, and the
conditions each peaked / masked input case must meet for tests/test_blank_inputs_gpu.py to mean something (runs without
a GPU)."""
import numpy as np
import pytest

from tests.blank_grad_ref import CASES, DIFFUSE, SHAPES, blank_loss_grad_ref, exact_case, feasible_by_length, reference
from tests.helpers import np_

MASKED = [c for c in CASES if c[1].startswith("masked")]
UNMASKED = [c for c in CASES + DIFFUSE if not c[1].startswith("masked")]
ids = "-".join


def _lengths_forced(inputs):
    lp, tgt, Tb, L = inputs
    T, B, _ = lp.shape
    return (int(Tb[0]) == T and int(L[0]) == tgt.shape[1] and int(tgt[1, 1]) == int(tgt[1, 0]) and int(L[1]) >= 2
            and int(Tb[1]) % 2 == 1 and (B < 4 or int(L[2]) == 0) and int(L[B - 1]) >= 1)


@pytest.mark.parametrize("case", UNMASKED, ids=ids)
def test_agrees_with_torch_float64(case):
    r = reference(*case)
    assert not np.isinf(np_(r["inputs"][0])).any() and r["fin"].all() and r["t64"]["fin"].all()
    assert np.abs(r["nll"] - r["t64"]["nll"]).max() <= 1e-12 * np.abs(r["nll"]).max()
    assert np.abs(r["grad"] - r["t64"]["grad"]).max() <= 1e-12


@pytest.mark.parametrize("case", MASKED, ids=ids)
def test_masked_agrees_with_torch_float64_where_torch_is_a_number(case):
    r = reference(*case)
    fin, g64 = r["fin"], r["t64"]["grad"]
    assert np.array_equal(fin, r["t64"]["fin"])
    assert np.abs(r["nll"][fin] - r["t64"]["nll"][fin]).max() <= 1e-12 * np.abs(r["nll"][fin]).max()
    ok = ~np.isnan(g64)
    assert np.abs(r["grad"][ok] - g64[ok]).max() <= 1e-12


@pytest.mark.parametrize("case", MASKED, ids=ids)
def test_torch_nans_sit_only_at_masked_entries_of_feasible_samples(case):
    r = reference(*case)
    masked = np.isinf(np_(r["inputs"][0]))
    assert not (np.isnan(r["t64"]["grad"]) & ~masked)[:, r["fin"]].any()


@pytest.mark.parametrize("case", MASKED, ids=ids)
def test_reference_is_finite_and_zero_at_masked_entries(case):
    r = reference(*case)
    assert np.isfinite(r["grad"]).all() and (r["grad"][np.isinf(np_(r["inputs"][0]))] == 0).all()


@pytest.mark.parametrize("case", CASES + DIFFUSE, ids=ids)
def test_zero_beyond_the_input_length_and_without_an_alignment(case):
    r = reference(*case)
    Tb = np_(r["inputs"][2])
    assert all((r["grad"][int(Tb[b]):, b] == 0).all() and (r["fin"][b] or (r["grad"][:, b] == 0).all())
               for b in range(len(Tb)))


@pytest.mark.parametrize("case", CASES + DIFFUSE, ids=ids)
def test_lengths_and_nll_pattern(case):
    """sample 0 full, sample 1 with an adjacent repeat on an odd T_b, an empty target where B >= 4; only the masked
    regimes have samples without an alignment: sample B-1 (its first label is never emitted) and the empty target
    (its only path is all blanks, and the blank has holes)"""
    r = reference(*case)
    want = np.ones(len(r["fin"]), dtype=bool)
    if case[1].startswith("masked"):
        want[-1] = False
        if len(want) >= 4:
            want[2] = False
    assert _lengths_forced(r["inputs"]) and np.array_equal(r["fin"], want) and not np.isnan(r["nll"]).any()


@pytest.mark.parametrize("case", MASKED, ids=ids)
def test_masked_case_has_a_sample_infeasible_through_its_emissions_alone(case):
    r = reference(*case)
    _, tgt, Tb, L = r["inputs"]
    assert (feasible_by_length(tgt, Tb, L) & ~r["fin"]).any()


@pytest.mark.parametrize("case", MASKED, ids=ids)
def test_masked_case_has_a_feasible_sample_masked_on_its_own_classes(case):
    r = reference(*case)
    lp, tgt, Tb, L = r["inputs"]
    assert any(r["fin"][b] and bool(np.isinf(np_(lp)[:int(Tb[b]), b][:, np_(tgt)[b, :int(L[b])]]).any())
               for b in range(len(Tb)))


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_reference_gradient_is_large_against_the_bound(case):
    """a zero or stale gradient must not pass: max |grad| over the feasible samples >= 40 x the case's bound"""
    r = reference(*case)
    assert r["gmax"] >= 40.0 * r["bound"], (r["gmax"], r["bound"], r["err32"])


@pytest.mark.parametrize("path", list(SHAPES))
def test_recorded_case_is_exact_and_feasible(path):
    """the inputs behind tests/golden/blank_loss_bits.npz: multiples of 1/512 (no rounding in their making), every
    sample with an alignment"""
    lp, tgt, Tb, L = exact_case(path)
    assert (np_(lp) * 512 == np.round(np_(lp) * 512)).all() and blank_loss_grad_ref(lp, tgt, Tb, L)[2].all()
