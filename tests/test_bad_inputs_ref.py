"""The cases of tests/bad_inputs_ref.py without a GPU: they cover every path of the tables they are built from, they hold
the bad samples where they say, no address an UNGUARDED kernel would touch leaves the test's own buffers (so that
tests/test_bad_inputs_gpu.py never depends on a guard for memory safety), the padded layout reaches the same kernels as
the contiguous one, and the float64 restatement is defined on every good sample."""
import numpy as np
import pytest

from tests import bad_inputs_ref as ref
from tests import blank_grad_ref as bg
from tests import lattice_inputs_ref as li
from tests.helpers import noblank_plan_entry, np_
from tests.test_noblank_plan import BF16, CUS, F32, FAMILIES as PLAN_FAMILIES, Query

CASES = ref.CASES
ids = ref.case_id


def test_cases_cover_exactly_the_path_tables():
    """a path added to a table later fails here until it has a case"""
    for family, table in (("noblank", li.NOBLANK_SHAPES), ("binary", li.BINARY_SHAPES), ("blank", bg.SHAPES)):
        assert {p for f, p, _ in CASES if f == family} == set(table)
        for p in table:
            assert [c for f, q, c in CASES if (f, q) == (family, p)] == list(range(len(ref.compositions(table[p][1]))))
    assert {f for f, _, _ in CASES} == {"noblank", "binary", "blank"}
    # the tables the GPU test draws its runs from name nothing else
    for family in ("noblank", "binary"):
        named = set(li.LOSS_PATHS[family]) | set(li.PATH_SHAPES[family]) | set(li.POSTERIOR_SHAPES[family])
        assert named == set(li.SHAPES[family]), named ^ set(li.SHAPES[family])
    assert "spans_k4" in li.NOBLANK_SHAPES and "spans_k4" not in li.NOBLANK_LOSS
    assert set(bg.SCHEDULES) == set(bg.SHAPES)
    assert {"k2", "k8", "w2", "w3"} <= set(bg.SHAPES)         # the blank read-outs' narrow and wide paths


@pytest.mark.parametrize("B", sorted({s[1] for t in ref.SHAPES.values() for s in t.values()}))
def test_compositions(B):
    comps = ref.compositions(B)
    bad = [set(c) for c in comps]
    every = set().union(*bad)
    assert all(0 <= b < B for b in every)
    assert {0, B - 1} <= every
    for c in bad:
        assert c and len(c) < B, "a composition without a good sample"
    if B >= 3:
        assert any(0 < b < B - 1 for b in every), "one in the middle"
        assert any(any(lo < g < hi and g not in c for g in range(B)) for c in bad for lo in c for hi in c), \
            "a good sample between bad ones"
    if B >= 4:
        assert any(b + 1 in c for c in bad for b in c), "two adjacent bad samples"
    if B > 64:                                                # the persistent form: hand-overs both ways, at fixed places
        (c,) = bad
        assert {0, 1, 255, 256, 257, B - 1} <= c and {b for b in range(B) if b % 13 == 5} <= c
        assert any(b - 1 not in c and b in c for b in range(1, B)) and any(b - 1 in c and b not in c for b in range(1, B))
    else:
        assert len(comps) == 2 and not bad[0] & bad[1], "every sample is good in one of the two launches"


@pytest.mark.parametrize("family", ref.FAMILIES)
def test_kinds_of_bad_lengths(family):
    """every kind but `infeasible` leaves the contract's range; together the cases of a family use every kind, and the
    persistent batch holds all of them by itself"""
    T, S = 24, 6
    for name, f in ref.BAD_LENGTHS[family]:
        for tb, l in ((24, 6), (12, 1), (20, 3)) + (((10, 0),) if family == "blank" else ()):
            got = f(T, S, tb, l)
            assert ref.in_range(family, T, S, *got) == (name == "infeasible"), (name, tb, l, got)
    names = {n for n, _ in ref.BAD_LENGTHS[family]}
    assert {"T=0", "T=-1", "T=T+1", "T=T+8", "L=-1", "L=S+1", "L=S+4", "both beyond", "infeasible", "T=2^32+3", "T=-2^32+3",
            "L=2^40+L_b"} <= names
    assert ("both below" in names) == (family != "binary")
    assert ("L=0" in names) == (family != "blank")
    used = set()
    for c in CASES:
        if c[0] == family:
            used |= {k for k in ref.make_case(*c)["kind"] if k}
    assert used == names, names - used
    if family == "noblank":
        assert {k for k in ref.make_case("noblank", "r16_ps", 0)["kind"] if k} == names


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_case_holds_what_it_says(case):
    c = ref.make_case(*case)
    f, T, B, C, S = (c[k] for k in ("family", "T", "B", "C", "S"))
    assert (T, B, C, S) == ref.SHAPES[f][case[1]], "the tables' shapes, unchanged"
    bad, badlab = c["bad"], c["badlab"]
    assert list(np.nonzero(bad)[0]) == ref.compositions(B)[case[2]]
    assert not (bad & badlab).any(), "bad labels never sit on a bad-length sample"
    x = np_(c["x"])
    assert x.shape == (T, B, C) and x.dtype == np.float32 and np.isfinite(x).all() and np.abs(x).max() < 20.0
    for b in range(B):
        tb, l = int(c["Tb"][b]), int(c["L"][b])
        vt, vl = int(c["valid"][0][b]), int(c["valid"][1][b])
        assert ref.in_range(f, T, S, vt, vl)
        if bad[b]:
            assert c["kind"][b] and ref.in_range(f, T, S, tb, l) == (c["kind"][b] == "infeasible")
            assert (int(c["Tb_twin"][b]), int(c["L_twin"][b])) == ref.INFEASIBLE
        else:
            assert c["kind"][b] is None and (tb, l) == (vt, vl) == (int(c["Tb_twin"][b]), int(c["L_twin"][b]))
    if f == "binary":
        return
    tg = np_(c["tg"]).astype(np.int64)
    assert np_(c["tg"]).dtype == (np.int64 if c["lab64"] else np.int32)
    outside = (tg < 0) | (tg >= C)
    for b in range(B):
        inside = outside[b, :max(int(c["valid"][1][b]), 0)]
        assert inside.any() == bool(badlab[b]), b
        if badlab[b]:
            v = tg[b, :int(c["L"][b])][inside]
            assert ((v >= -C) & (v < 2 * C) | (v >= ref.HI) & (v < ref.HI + C)).all()
    if f == "blank":
        for b in np.nonzero(bad)[0]:
            assert tg[b, 0] != tg[b, 1] and 1 <= tg[b, 0] < C and 1 <= tg[b, 1] < C


def test_bad_labels_reach_both_ranges_and_the_high_word():
    for family in ("noblank", "blank"):
        seen = {"below": False, "above": False, "high": False, "int32": False, "int64": False}
        for case in CASES:
            if case[0] != family:
                continue
            c = ref.make_case(*case)
            tg, C = np_(c["tg"]).astype(np.int64), c["C"]
            for b in np.nonzero(c["badlab"])[0]:
                v = tg[b, :int(c["L"][b])]
                seen["below"] |= bool(((v < 0) & (v >= -C)).any())
                seen["above"] |= bool(((v >= C) & (v < 2 * C)).any())
                seen["high"] |= bool((v >= ref.HI).any())
                seen["int64" if c["lab64"] else "int32"] = True
        assert all(seen.values()), (family, seen)
    # the rule the expected outputs go by
    assert list(ref.effective_classes("noblank", np.array([-1, -10, 10, 19, ref.HI + 3, 7]), 10)) == [9, 0, 0, 9, 3, 7]
    assert list(ref.effective_classes("blank", np.array([-1, -10, 10, 19, ref.HI + 3, 7]), 10)) == [0, 0, 9, 9, 3, 7]
    assert list(ref.low_word(np.array([ref.HI + 3, -ref.HI + 3, (1 << 40) + 5, -1, 7]))) == [3, 3, 5, -1, 7]


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_no_unguarded_address_leaves_the_buffers(case):
    """THE condition that lets the GPU test run on a shared machine: a kernel with no guard at all would stay inside the
    test's own allocations on every case.  Not a measurement: a case that violates it is changed."""
    c = ref.make_case(*case)
    f, T, B, C, S = (c[k] for k in ("family", "T", "B", "C", "S"))
    lay = ref.layout(f, T, B, C, S)
    ext, problems = ref.unguarded_extents(c)
    assert not problems, problems
    assert set(ext) == set(lay)
    for name, (lo, hi) in ext.items():
        n, tail = lay[name]
        assert 0 <= lo <= hi < n + tail, (name, lo, hi, n, tail)
    # ... with the margins the kinds were written for, whatever this case happens to hold
    worst = dict(c, Tb=np.full(B, T + ref.T_MARGIN), L=np.full(B, S + ref.S_MARGIN))
    for name, (lo, hi) in ref.unguarded_extents(worst)[0].items():
        n, tail = lay[name]
        assert 0 <= lo <= hi < n + tail, ("worst", name, lo, hi, n, tail)
    # x: the centre of X, a whole class row of canaries on either side
    off, st, sb = ref.x_strides(B, C)
    assert off == C and sb == 3 * C and st == (B + 1) * sb and lay["X"][0] == (T + ref.T_MARGIN) * st
    assert all(0 <= k < C for k in ref.label_tail(C))


@pytest.fixture(scope="module")
def plan():
    entry = noblank_plan_entry()

    def call(q):
        got = entry(q.T, q.B, q.C, q.S, q.dtype, q.st, q.sb, q.x_low, q.grad_low, q.want_grad, q.want_gamma, q.smooth, CUS,
                    q.sw)
        got["family"] = PLAN_FAMILIES[got["family"]]
        return got
    return call


@pytest.mark.parametrize("path", list(li.NOBLANK_SHAPES))
def test_padded_layout_reaches_the_same_noblank_kernel(plan, path):
    """x inside X changes the strides and the address: the plan answers as for the contiguous tensor (the allocator
    aligns X to 256 bytes at least, so x starts 4 C bytes into an aligned block)"""
    T, B, C, S = li.NOBLANK_SHAPES[path]
    off, st, sb = ref.x_strides(B, C)
    modes = [dict(want_gamma=True)] if path == "spans_k4" else [dict(), dict(want_grad=False), dict(want_gamma=True)]
    if path == "r16":
        modes += [dict(dtype=BF16), dict(smooth=True)]
    for m in modes:
        esz = 2 if m.get("dtype", F32) != F32 else 4
        plain, padded = plan(Query(T, B, C, S, **m)), plan(Query(T, B, C, S, st=st, sb=sb, x_low=(off * esz) % 256, **m))
        assert plain["family"] != "unsupported" and padded == plain, (path, m, plain, padded)


@pytest.mark.parametrize("path", list(bg.SHAPES))
def test_padded_layout_keeps_the_blank_rows_form(path):
    """blank_rows_vec4 (ctc_amd/csrc/blank.hip): C % 4 == 0, strides % 4 == 0, 16-byte aligned rows"""
    T, B, C, S = bg.SHAPES[path]
    off, st, sb = ref.x_strides(B, C)
    plain = C % 4 == 0 and (B * C) % 4 == 0
    padded = C % 4 == 0 and st % 4 == 0 and sb % 4 == 0 and (4 * off) % 16 == 0
    assert plain == padded == (path != "k2_scalar" and C % 4 == 0)


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_expected_outputs(case):
    c, e = ref.make_case(*case), ref.expected(*case)
    T, B, C, S = (c[k] for k in "TBCS")
    bad, fin = c["bad"], e["fin"]
    assert not fin[bad].any(), "the twin's (1, 2) has no alignment"
    assert np.isposinf(e["nll"][bad]).all() and (e["grad"][:, bad] == 0).all() and (e["gamma"][bad] == 0).all()
    assert (e["path"][bad] == -1).all() and np.isneginf(e["score"][bad]).all()
    good = ~bad
    assert fin[good].all() and np.isfinite(e["nll"][good]).all(), "the restatement is defined on every good sample"
    assert np.isfinite(e["grad"]).all() and np.isfinite(e["gamma"]).all()
    assert e["gamma"].shape == (B, T, ref.states(c["family"], S)) and e["grad"].shape == (T, B, C)
    for b in np.nonzero(good)[0]:
        tb = int(c["Tb_twin"][b])
        assert np.abs(e["gamma"][b, :tb].sum(1) - 1.0).max() < 1e-9 and (e["gamma"][b, tb:] == 0).all()
        assert (e["path"][b, :tb] >= 0).all() and (e["path"][b, tb:] == -1).all()
    # a bad-label sample is computed on the classes the kernels read: different from the raw labels' modulo where the
    # value lies beyond 32 bits, and a sample of its own right (its gradient is not the neighbour's)
    assert float(np.abs(e["grad"][:, good]).max()) > 0
