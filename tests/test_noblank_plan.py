"""Which kernel a no-blank call gets (runs without a GPU).

Every no-blank kernel is correct on every shape it accepts, so the parity tests pass whichever kernel runs: a slip in
the selection rules would show only as a slower benchmark.  This test calls `noblank_plan()` of ctc_amd/csrc/noblank.hip
through the diagnostics build's `ctc_amd_debug_noblank_plan` over a grid of argument combinations, with the CU count
fixed at 256, and compares every answer with `expected()` below: the selection rules restated in plain Python from
`noblank_run` and `ctc_amd_noblank_posteriors` as they stood before the plan function existed (one copy of the rules
per entry point and element type, as they were written there).  `expected()` is the yardstick: a change of a rule is
made there on purpose, never by copying what the C++ answers."""
import ctypes
import itertools
import math

import pytest

from tests.helpers import NOBLANK_PLAN_FAMILIES, NOBLANK_PLAN_FIELDS, noblank_plan_entry

F32, BF16, F16 = 0, 1, 2
CUS = 256
MAX_LDS = 160 * 1024
WAVE, PREFETCH = 64, 4
PIPE_WORKERS, PIPE_MAX_T, KM_WORKERS = 14, 168, 12
NT_BYTES = 230 << 20
NOPIPE, NOXR, NOR16, NOPS, KM = 1, 2, 4, 8, 16
FIELDS, FAMILIES = NOBLANK_PLAN_FIELDS, NOBLANK_PLAN_FAMILIES
PS_PAIRS = {(0, 1), (0, 2), (1, 0), (1, 1), (1, 2), (2, 0), (2, 1), (2, 2), (3, 0)}


# ---- sizes, as the kernels' headers compute them ---------------------------------------------------------------------
def lattice_floats(T, SP):
    return (3 * T + 2 * PREFETCH) * SP + 2 * T


def tables_bytes(SP, C):
    return (8 + 16 + 3 * SP + C + 4) * 4


def smem_bytes(T, SP, C):
    return lattice_floats(T, SP) * 4 + tables_bytes(SP, C)


def xr_smem_bytes(T, SP, C):
    return (3 * T + 2 * PREFETCH) * SP * 8 + tables_bytes(SP, C) + PIPE_WORKERS * 12 * 4


def _pitch(tp, mask, rem):
    while tp & mask != rem:
        tp += 1
    return tp


def _worker_tables(SP, C, workers):
    return (8 + 16 + 2 * ((SP + 3) & ~3) + 4 + 64) * 4 + workers * 4 * (32 * ((C + 31) // 32)) * 4


def r16_smem_bytes(T, SP, C):
    return 3 * (SP + 1) * _pitch(T + 2 * 9 + 1, 3, 2) * 8 + _worker_tables(SP, C, PIPE_WORKERS)


def km_smem_bytes(T, SP, C):
    return (3 * (SP + 1) * _pitch(T + 16, 3, 2) * 8 + 2 * (SP + 1) * _pitch(T + 16, 7, 4) * 4 +
            _worker_tables(SP, C, KM_WORKERS))


def km_offset(T, S):
    n, k = T - 1, min(S - 1, (T - 1) // 2)
    lg = (math.lgamma(n + 1.0) - math.lgamma(k + 1.0) - math.lgamma(n - k + 1.0)) / 0.6931471805599453
    return -1 if lg > 88.0 else int(lg / 2.0 + 1.0)


def r16_shape(C):
    if C < 2 or C > 256 or C & 1:
        return None
    U = (C + 31) // 32
    if U & 1:
        return U // 2, 1
    if C & 3 == 0:
        return U // 2, 0
    return U // 2 - 1, 2


def lane_states(S):
    K = 1
    while K <= 4 and S > WAVE * K:
        K *= 2
    return K, (S + K - 1) // K * K


# ---- the rules -------------------------------------------------------------------------------------------------------
def _answer(family, **kw):
    out = dict.fromkeys(FIELDS, 0)
    out.update(kw, family=FAMILIES.index(family))
    return out


def _unsupported(why):
    return dict(_answer("unsupported"), why=why)


def _r16(q, n4, n2, nt, rsmem, esz):
    """launch_r16: the persistent form for its nine chunkings, else one sample per workgroup"""
    ps = q.B > 2 * CUS and not q.sw & NOPS and q.want_grad and (n4, n2) in PS_PAIRS
    nxt = CUS if q.B > CUS and q.T * ((q.C * esz + 127) // 128) <= PIPE_WORKERS * WAVE else 0
    return _answer("r16", n4=n4, n2=n2, nt=int(nt), ps=int(ps), grid=CUS if ps else q.B, lds=rsmem, next_round=nxt)


def _fused(q, K, smem, glb):
    ch = (q.C + WAVE - 1) // WAVE if q.C <= 256 and not glb else 0
    return _answer("fused", K=K, ch=ch, glb=int(glb), grid=q.B, lds=smem)


def expected_loss(q):
    K, SP = lane_states(q.S)
    if K > 4:
        return _unsupported("S > 256")
    even = q.C % 2 == 0 and q.st % 2 == 0 and q.sb % 2 == 0
    rsmem = r16_smem_bytes(q.T, SP, q.C)
    if q.dtype != F32:                                       # 2-byte logits: r16 or nothing, 4-byte aligned rows
        aligned = even and q.x_low % 4 == 0 and q.grad_low % 4 == 0
        if K != 1 or q.T > PIPE_MAX_T or not aligned or not r16_shape(q.C) or SP > 31 or rsmem > MAX_LDS:
            return _unsupported("2-byte logits outside r16")
        return _r16(q, *r16_shape(q.C), 4 * q.T * q.B * q.C > NT_BYTES, rsmem, 2)
    smem, glb = smem_bytes(q.T, SP, q.C), False
    if smem > MAX_LDS:                                       # long sequence: lattice in the workspace
        if q.smooth:
            return _unsupported("smoothing with a long sequence")
        smem, glb = tables_bytes(SP, q.C), True
        if smem > MAX_LDS:
            return _unsupported("tables beyond LDS")
    ch = (q.C + WAVE - 1) // WAVE if q.C <= 256 else 0
    if K == 1 and ch >= 1 and q.T <= PIPE_MAX_T and not q.sw & NOPIPE and not glb:
        dual = q.B > CUS and 2 * smem <= MAX_LDS
        aligned = even and q.x_low % 8 == 0 and q.grad_low % 8 == 0
        if not q.sw & NOR16 and aligned and r16_shape(q.C) and SP <= 31 and rsmem <= MAX_LDS:
            n4, n2 = r16_shape(q.C)
            nt = 8 * q.T * q.B * q.C > NT_BYTES
            ksmem, koff = km_smem_bytes(q.T, SP, q.C), km_offset(q.T, q.S)
            if q.sw & KM and ksmem <= MAX_LDS and koff >= 0:
                nxt = CUS if q.B > CUS and q.T * ((q.C * 4 + 127) // 128) <= KM_WORKERS * WAVE else 0
                return _answer("km", n4=n4, n2=n2, nt=int(nt), grid=q.B, lds=ksmem, next_round=nxt, koff=koff)
            return _r16(q, n4, n2, nt, rsmem, 4)
        if q.smooth:
            return _unsupported("smoothing outside r16")
        xsmem = xr_smem_bytes(q.T, SP, q.C)
        if not q.sw & NOXR and xsmem <= MAX_LDS and (not dual or 2 * xsmem <= MAX_LDS):
            return _answer("xr", ch=ch, dual=int(dual), grid=q.B, lds=xsmem)
        return _answer("pipelined", ch=ch, dual=int(dual), grid=q.B, lds=smem)
    if q.smooth:
        return _unsupported("smoothing outside r16")
    return _fused(q, K, smem, glb)


def expected_posteriors(q):
    """reads no diagnostic switch; r16 without gradient (8-byte aligned x), else the phase-serial kernel"""
    K, SP = lane_states(q.S)
    if K > 4:
        return _unsupported("S > 256")
    smem, glb = smem_bytes(q.T, SP, q.C), False
    if smem > MAX_LDS:
        smem, glb = tables_bytes(SP, q.C), True
        if smem > MAX_LDS:
            return _unsupported("tables beyond LDS")
    aligned = q.C % 2 == 0 and q.st % 2 == 0 and q.sb % 2 == 0 and q.x_low % 8 == 0
    rsmem = r16_smem_bytes(q.T, SP, q.C)
    if K == 1 and q.T <= PIPE_MAX_T and not glb and aligned and r16_shape(q.C) and SP <= 31 and rsmem <= MAX_LDS:
        n4, n2 = r16_shape(q.C)
        return _answer("r16", n4=n4, n2=n2, grid=q.B, lds=rsmem)
    return _fused(q, K, smem, glb)


class Query:
    def __init__(self, T, B, C, S, dtype=F32, st=None, sb=None, x_low=0, grad_low=0, want_grad=True, want_gamma=False,
                 smooth=False, sw=0):
        self.T, self.B, self.C, self.S, self.dtype = T, B, C, S, dtype
        self.st, self.sb = B * C if st is None else st, C if sb is None else sb
        self.want_grad, self.want_gamma, self.smooth = want_grad and not want_gamma, want_gamma, smooth
        self.x_low, self.grad_low = x_low, grad_low if self.want_grad else 0     # (no gradient: a null pointer)
        self.sw = 0 if want_gamma else sw                    # (the posteriors entry point hands the plan no switch)
        self.SP = lane_states(S)[1]

    def key(self):
        return (self.T, self.B, self.C, self.S, self.dtype, self.st, self.sb, self.x_low, self.grad_low, self.want_grad,
                self.want_gamma, self.smooth, self.sw)


def expected(q):
    return expected_posteriors(q) if q.want_gamma else expected_loss(q)


MODES = [dict(), dict(want_grad=False), dict(smooth=True), dict(dtype=BF16), dict(dtype=F16, smooth=True),
         dict(dtype=BF16, want_grad=False), dict(want_gamma=True)]
TS = (1, 150, 168, 169, 1000)
CS = (1, 63, 100, 158, 192, 194, 256, 258, 41000)
SS = (1, 20, 31, 32, 39, 40, 63, 64, 65, 128, 129, 256, 257)
BS = (1, 256, 257, 512, 513)


def grid():
    qs = [Query(T, B, C, S, **m) for T, B, C, S, m in itertools.product(TS, BS, CS, SS, MODES)]
    # alignment of the two addresses and parity of the strides, for every element type and the posteriors
    for C, S, (x_low, grad_low), (st, sb), m in itertools.product(
            (158, 160), (20, 40), itertools.product((0, 2, 4, 8, 12), (0, 4, 8)),
            ((None, None), (512 * 160 + 1, None), (None, 161)), MODES):
        qs.append(Query(150, 512, C, S, x_low=x_low, grad_low=grad_low, st=st, sb=sb, **m))
    # the diagnostic switches, one at a time and all together, on shapes of every fast family
    for sw, B, C, S, m in itertools.product((NOPIPE, NOXR, NOR16, NOPS, KM, KM | NOPS, 31), (256, 513, 1024), (158, 256),
                                            (8, 20, 31, 40, 64), MODES):
        qs.append(Query(150, B, C, S, sw=sw, **m))
        qs.append(Query(168, B, C, S, sw=sw, **m))
    # logits + gradient on either side of 230 MB: 8 T B C (fp32), 4 T B C (2-byte)
    for B, m in itertools.product((1272, 1273, 2544, 2545), MODES):
        qs.append(Query(150, B, 158, 20, **m))
    # the r16 and km arrays on either side of LDS at the largest rows
    for S, C, sw in itertools.product(range(20, 32), (158, 192, 224, 256), (0, KM)):
        qs.append(Query(168, 300, C, S, sw=sw))
    return list({q.key(): q for q in qs}.values())


@pytest.fixture(scope="module")
def plan():
    entry = noblank_plan_entry()

    def call(q):
        return entry(q.T, q.B, q.C, q.S, q.dtype, q.st, q.sb, q.x_low, q.grad_low, q.want_grad, q.want_gamma, q.smooth, CUS,
                     q.sw)
    return call


def test_grid_covers_every_family_and_threshold():
    qs = grid()
    ans = [expected(q) for q in qs]
    assert len(qs) >= 3000
    loss = [(q, a) for q, a in zip(qs, ans) if not q.want_gamma]
    for fam in FAMILIES:                                     # every family, from the loss and (r16, fused) the posteriors
        assert any(FAMILIES[a["family"]] == fam for _, a in loss), fam
    assert {FAMILIES[a["family"]] for q, a in zip(qs, ans) if q.want_gamma} == {"unsupported", "r16", "fused"}
    assert {a["why"] for a in ans if "why" in a} == {
        "S > 256", "2-byte logits outside r16", "smoothing with a long sequence", "tables beyond LDS",
        "smoothing outside r16"}
    have = lambda attr, *vals: all(any(getattr(q, attr) == v for q in qs) for v in vals)
    assert have("T", 168, 169) and have("SP", 31, 32, 63, 64) and have("B", 256, 257, 512, 513)
    assert have("C", 192, 194, 256, 258) and any(q.C % 2 and q.C > 1 for q in qs)
    assert have("dtype", F32, BF16, F16) and have("smooth", False, True) and have("want_grad", False, True)
    assert have("x_low", 0, 4, 8) and have("grad_low", 0, 4, 8)
    # both sides of every LDS limit and of the 230 MB threshold, among shapes where that limit decides
    def both(f, pick=lambda q: True):
        vals = {f(q) for q in qs if pick(q)}
        return vals == {False, True}
    fast = lambda q: q.SP <= 64 and q.S <= 64 and q.T <= PIPE_MAX_T and q.C <= 256
    assert both(lambda q: smem_bytes(q.T, q.SP, q.C) > MAX_LDS, lambda q: q.S <= 256)
    assert both(lambda q: tables_bytes(q.SP, q.C) > MAX_LDS, lambda q: q.S <= 256)
    assert both(lambda q: r16_smem_bytes(q.T, q.SP, q.C) > MAX_LDS, lambda q: fast(q) and q.SP <= 31 and r16_shape(q.C))
    assert both(lambda q: km_smem_bytes(q.T, q.SP, q.C) > MAX_LDS,
                lambda q: q.sw & KM and FAMILIES[expected(q)["family"]] in ("r16", "km"))
    assert both(lambda q: xr_smem_bytes(q.T, q.SP, q.C) > MAX_LDS, fast)
    assert both(lambda q: 2 * xr_smem_bytes(q.T, q.SP, q.C) > MAX_LDS, lambda q: fast(q) and q.B > CUS)
    assert both(lambda q: 2 * smem_bytes(q.T, q.SP, q.C) > MAX_LDS, lambda q: fast(q) and q.B > CUS)
    assert both(lambda q: 8 * q.T * q.B * q.C > NT_BYTES, lambda q: q.dtype == F32 and (q.T, q.C) == (150, 158))
    assert both(lambda q: 4 * q.T * q.B * q.C > NT_BYTES, lambda q: q.dtype != F32 and (q.T, q.C) == (150, 158))
    for field in ("nt", "ps", "dual", "glb"):                # and the selectors they feed take both values
        assert {a[field] for a in ans} == {0, 1}, field
    assert {a["next_round"] for a in ans} == {0, CUS}
    assert {(a["n4"], a["n2"]) for a in ans if FAMILIES[a["family"]] == "r16" and a["ps"]} <= PS_PAIRS
    assert {a["K"] for a in ans if FAMILIES[a["family"]] == "fused"} == {1, 2, 4}
    assert {a["ch"] for a in ans if FAMILIES[a["family"]] == "fused"} == {0, 1, 2, 3, 4}


def test_plan_matches_the_restated_rules(plan):
    wrong = []
    for q in grid():
        want = {k: v for k, v in expected(q).items() if k != "why"}
        got = plan(q)
        if got != want:
            wrong.append((q.key(), {k: (got[k], want[k]) for k in FIELDS if got[k] != want[k]}))
    assert not wrong, "%d calls planned differently, the first: %r" % (len(wrong), wrong[:5])


def test_plan_entry_rejects_empty_shapes():
    from ctc_amd import build
    fn = ctypes.CDLL(build.build_diag()).ctc_amd_debug_noblank_plan
    assert fn(0, 1, 2, 1, 0, ctypes.c_int64(2), ctypes.c_int64(2), 0, 0, 1, 0, 0, CUS, 0, None) == -1
