"""The float64 lattice reference of tests/lattice_inputs_ref.py against oracle/ctc_numpy in float64 and against the
closed form on tied inputs, and the conditions each peaked / masked / tied input case must meet for
tests/test_lattice_inputs_gpu.py to mean something (runs without a GPU)."""
import ctypes

import numpy as np
import pytest

from tests.lattice_inputs_ref import (BINARY_KERNEL, BINARY_SHAPES, CAP, KINDS, LOSS_PATHS, NOBLANK_FAMILY, NOBLANK_LOSS,
                                      NLL_RTOL, NOBLANK_SHAPES, PAD_LOGIT, PATH_SHAPES, POSTERIOR_SHAPES, R16, REGIMES, SHAPES,
                                      port64, reference, ties_closed_form)
from tests.helpers import binary_plan_entry, np_
from tests.test_binary_plan import kernel_name
from tests.test_noblank_plan import BF16, CUS, F32, FAMILIES, FIELDS, PS_PAIRS, Query

CASES = [(f, p, r) for f in SHAPES for p in SHAPES[f] for r in REGIMES]
ids = "-".join


def _label_cells(case):
    """[T,B,S] logits at the label classes (no-blank)"""
    x, lab, Tb, L = reference(*case)["inputs"]
    T, _, C = x.shape
    return np.take_along_axis(np_(x), (np_(lab).astype(np.int64) % C)[None].repeat(T, 0), axis=2)


def _comparable(case):
    """the samples on which oracle/ctc_numpy is defined: no -inf and no -1e30 on a live label class"""
    r = reference(*case)
    x, _, Tb, L = r["inputs"]
    B = x.shape[1]
    if case[0] == "binary":
        return np.ones(B, bool)
    cells = _label_cells(case)
    ok = np.ones(B, bool)
    for b in range(B):
        ok[b] = (cells[:int(Tb[b]), b, :int(L[b])] > -1e29).all()
    return ok


def test_pad_logit_is_the_producers():
    from ctc_amd import producer
    assert PAD_LOGIT == producer.PAD_LOGIT


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_agrees_with_the_oracle_in_float64(case):
    r, p = reference(*case), port64(*case)
    ok = _comparable(case)
    if case[2] != "masked":
        assert ok.all() and r["fin"].all()
    else:
        assert ok.any()
    assert np.array_equal(r["fin"][ok], np.ones(int(ok.sum()), bool))
    assert np.abs(r["nll"][ok] - p["nll"][ok]).max() <= 1e-9 * np.maximum(1.0, np.abs(r["nll"][ok])).max()
    assert np.abs(r["grad"][:, ok] - p["grad"][:, ok]).max() <= 1e-9
    assert np.abs(r["gamma"][ok] - p["gamma"][ok]).max() <= 1e-9


@pytest.mark.parametrize("case", [c for c in CASES if c[2] == "ties"], ids=ids)
def test_agrees_with_the_closed_form_on_ties(case):
    r = reference(*case)
    x, tg, Tb, L = r["inputs"]
    T, _, C = x.shape
    nll, gamma, path = ties_closed_form(case[0], T, C, tg.shape[1], np_(Tb), np_(L))
    assert np.abs(r["nll"] - nll).max() <= 1e-9 * np.abs(nll).max()
    assert np.abs(r["gamma"] - gamma).max() <= 1e-9
    assert np.array_equal(r["path"], path)


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_feasibility_is_what_the_case_was_built_to_contain(case):
    """only kinds d and e of a masked no-blank batch have no alignment; every such batch holds all five kinds"""
    r = reference(*case)
    kinds = r["kinds"]
    if case[0] == "noblank" and case[2] == "masked":
        assert set(kinds) == set(KINDS)
    else:
        assert set(kinds) == {"-"}
    assert np.array_equal(r["fin"], np.array([k not in "de" for k in kinds]))
    assert np.array_equal(np.isinf(r["nll"]), ~r["fin"]) and not np.isnan(r["nll"]).any() and (r["nll"][~r["fin"]] > 0).all()
    assert (r["path"][~r["fin"]] == -1).all() and (r["score"][~r["fin"]] == -np.inf).all()
    _, _, Tb, L = r["inputs"]
    assert bool((L >= 1).all() and (L <= Tb).all() and (Tb <= r["inputs"][0].shape[0]).all())
    assert int(Tb[0]) == r["inputs"][0].shape[0] and len(set(np_(Tb).tolist())) > 1       # ragged
    assert int(L[-1]) < int(Tb[-1])                          # more than one alignment: "ties stay" can fail


@pytest.mark.parametrize("case", [c for c in CASES if c[0] == "noblank" and c[2] == "masked"], ids=ids)
def test_masked_kinds_hold_what_they_say(case):
    r = reference(*case)
    x, lab, Tb, L = r["inputs"]
    xn, cells = np_(x), _label_cells(case)
    C = xn.shape[2]
    for b, k in enumerate(r["kinds"]):
        tb, l = int(Tb[b]), int(L[b])
        live = cells[:tb, b, :l]
        own = set((np_(lab)[b, :l].astype(np.int64) % C).tolist())
        if k == "a":
            assert np.isneginf(xn[:, b, 0]).all() and np.isneginf(xn[:, b, C - 1]).all() and (xn[:, b, 2] == PAD_LOGIT).all()
            assert not own & {0, 2, C - 1} and np.isfinite(live).all()
        elif k == "b":                                       # -inf on an own class, on frames where other states are reachable
            masked = np.isneginf(live)
            assert masked.any() and (r["gamma"][b, :tb, :l][~masked].reshape(-1) > 0).any()
            assert (np.abs(r["gamma"][b, :tb].sum(1) - 1.0) < 1e-9).all() and (r["gamma"][b, :tb, :l][masked] == 0).all()
        elif k == "c":
            assert (live == -1e4).any() and np.isfinite(live).all() and 1e3 < r["nll"][b] < 1e4
        elif k == "d":
            assert np.isneginf(live).all(axis=1).sum() == 1
        else:
            assert (live == PAD_LOGIT).all(axis=1).sum() == 1 and np.isfinite(live).all()


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_gradient_is_finite_and_zero_at_masked_entries(case):
    r = reference(*case)
    x, _, Tb, _ = r["inputs"]
    assert np.isfinite(r["grad"]).all() and np.isfinite(r["gamma"]).all()
    assert (r["grad"][np.isinf(np_(x))] == 0).all()
    for b in range(x.shape[1]):
        assert (r["grad"][int(Tb[b]):, b] == 0).all() and (r["fin"][b] or (r["grad"][:, b] == 0).all())
        assert r["fin"][b] or (r["gamma"][b] == 0).all()
    if case[2] == "masked":
        assert np.isinf(np_(x)).any()


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_the_cap(case):
    """the float32 port of the reference itself stays within 0.2 % of full scale on every case: 2 err32 <= 2e-3 on the
    per-sample gradient B * grad (|B * grad| <= 1) and on gamma.  A condition on the inputs: a case that breaks it gets
    milder inputs, the cap stays."""
    r = reference(*case)
    B = r["inputs"][0].shape[1]
    assert 2.0 * r["err32"] * B <= CAP, (2.0 * r["err32"] * B, r["err32"])
    assert 2.0 * r["err32_gamma"] <= CAP, r["err32_gamma"]
    # and its nll within the kernels' own tolerance: where the reference's float32 arithmetic misses it, nothing can be asked
    assert r["err32_nll"] <= NLL_RTOL, r["err32_nll"]


@pytest.mark.parametrize("case", [(f, p, r) for f in SHAPES for p in LOSS_PATHS[f] for r in REGIMES], ids=ids)
def test_reference_gradient_is_large_against_the_bound(case):
    """a zero or stale gradient must not pass: max |grad| >= 10 x the case's bound (the binary gradient carries 1 / (B C))"""
    r = reference(*case)
    assert r["gmax"] >= 10.0 * r["bound"], (r["gmax"], r["bound"], r["err32"])


# ---- which kernel each shape reaches ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plan():
    from ctc_amd import build
    fn = ctypes.CDLL(build.build_diag()).ctc_amd_debug_noblank_plan
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_int] * 5 + [ctypes.c_int64] * 2 + [ctypes.c_uint] * 2 + [ctypes.c_int] * 5 + \
        [ctypes.POINTER(ctypes.c_int64)]
    out = (ctypes.c_int64 * len(FIELDS))()

    def call(q):
        assert fn(q.T, q.B, q.C, q.S, q.dtype, q.st, q.sb, q.x_low, q.grad_low, int(q.want_grad), int(q.want_gamma),
                  int(q.smooth), CUS, q.sw, out) == 0
        got = dict(zip(FIELDS, out))
        got["family"] = FAMILIES[got["family"]]
        return got
    return call


def _family(path):
    return NOBLANK_FAMILY.get(path, path.split("_")[0])


@pytest.mark.parametrize("path", NOBLANK_LOSS)
def test_noblank_loss_shape_gets_the_family_its_name_says(plan, path):
    chunking = {"r16": (0, 1), "r16_n4": (1, 0), "r16_n2": (0, 2)}
    kk = {"fused_t": 1, "fused_c": 1, "fused_k2": 2, "fused_k4": 4, "glb": 1}
    for want_grad in (True, False):
        got = plan(Query(*NOBLANK_SHAPES[path], dtype=F32, want_grad=want_grad))
        assert got["family"] == ("fused" if path == "glb" else _family(path)), (path, got)
        if path in chunking:
            assert (got["n4"], got["n2"]) == chunking[path]
        if path in kk:
            assert got["K"] == kk[path] and got["glb"] == int(path == "glb")
        assert got["ps"] == int(path == "r16_ps" and want_grad)
        if got["ps"]:
            assert (got["n4"], got["n2"]) in PS_PAIRS and got["grid"] == CUS


@pytest.mark.parametrize("path", R16)
def test_two_byte_logits_get_r16(plan, path):
    assert plan(Query(*NOBLANK_SHAPES[path], dtype=BF16))["family"] == "r16"


def test_posteriors_and_read_out_shapes(plan, binary_plan):
    fam = [plan(Query(*NOBLANK_SHAPES[p], want_gamma=True))["family"] for p in POSTERIOR_SHAPES["noblank"]]
    assert fam == ["r16", "fused"]
    for family in SHAPES:                                     # the read-outs: one, two and four states per lane
        assert [1 if SHAPES[family][p][3] <= 64 else 2 if SHAPES[family][p][3] <= 128 else 4
                for p in PATH_SHAPES[family]] == [1, 2, 4]
    for p in POSTERIOR_SHAPES["binary"]:                      # ctc_amd_binary_posteriors: the pipelined kernel's domain
        T, _, C, S = BINARY_SHAPES[p]
        assert S <= 64 and T <= 168 and C <= 256
    assert [BINARY_KERNEL[p] for p in POSTERIOR_SHAPES["binary"]] == ["flow", "pipe"]
    assert [binary_plan(*BINARY_SHAPES[p], want_gamma=True) for p in POSTERIOR_SHAPES["binary"]] == ["flow", "pipe"]


@pytest.fixture(scope="module")
def binary_plan():
    entry = binary_plan_entry()
    return lambda T, B, C, S, want_gamma=False: kernel_name(entry(T, B, C, S, F32, want_gamma, 0))


@pytest.mark.parametrize("path", list(BINARY_SHAPES))
def test_binary_loss_shape_gets_the_kernel_its_name_says(binary_plan, path):
    """binary_plan() of ctc_amd/csrc/binary.hip, asked through the diagnostics build (tests/test_binary_plan.py)"""
    assert binary_plan(*BINARY_SHAPES[path]) == BINARY_KERNEL[path]
    assert {BINARY_KERNEL[p] for p in BINARY_SHAPES} == {"flow", "pipe", "mfma2", "mfma4", "valu1"}
