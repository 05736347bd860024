"""Which kernel a binary call gets (runs without a GPU).

Every binary kernel is correct on every shape it accepts, so the parity tests pass whichever kernel runs: a slip in the
selection rules would show only as a slower benchmark, or as a test shape that quietly stopped reaching the kernel it
was chosen for.  This test calls `binary_plan()` of ctc_amd/csrc/binary.hip through the diagnostics build's
`ctc_amd_debug_binary_plan` over a grid of argument combinations and compares every field of every answer with
`expected()` below: the selection rules restated in plain Python from `ctc_amd_binary_loss_grad` and
`binary_posteriors_entry` as they stood before the plan function existed (one copy of the rules per entry point, as
they were written there).  `expected()` is the yardstick: a change of a rule is made there on purpose, never by copying
what the C++ answers.  The shapes that the GPU tests name after a kernel are asked here too (`kernel_name`)."""
import ctypes
import itertools

import pytest

from tests.helpers import BINARY_PLAN_FAMILIES, BINARY_PLAN_FIELDS, binary_plan_entry

F32, BF16, F16 = 0, 1, 2
MAX_LDS = 160 * 1024
WAVE, PREFETCH = 64, 4
FLOW_MAX_T, PIPE_MAX_T, MFMA_MAX_T = 160, 168, 160
WT_BYTES = 230 << 20
VALU, NOPIPE, NOFLOW = 1, 2, 4
FIELDS, FAMILIES = BINARY_PLAN_FIELDS, BINARY_PLAN_FAMILIES


# ---- sizes, as the kernels' headers compute them ---------------------------------------------------------------------
def lane_states(S):
    K = 1
    while K <= 4 and S > WAVE * K:
        K *= 2
    return K, (S + K - 1) // K * K


def image_pitch(C):
    PD = (C + 3) // 4 * 4 + 2
    while PD % 32 != 2:
        PD += 2
    return PD


def flow_pitch(C):
    PF = (C + 15) // 16 * 16 + 4
    while PF % 32 != 4:
        PF += 4
    return PF


def flow_smem_bytes(T, SP, PF, C):
    halfs = (SP + 1) * ((C + 31) // 32 * 32 + 8)            # the bf16 target image behind the fp32 one
    images = ((SP * PF + 3) & ~3) + (((halfs + 1) // 2 + 3) & ~3)
    return ((3 * T + 2 * PREFETCH) * SP + 64 + ((T + 7) & ~3) + 64 + images + (T + 1) * PF) * 4


def pipe_smem_bytes(T, SP, PD):
    return ((3 * T + 2 * PREFETCH) * SP + 32 + ((T + 3) & ~3) + 64 + SP * PD + T * PD) * 4


def mfma_smem_bytes(T, Tpad, SP, PD):
    return ((3 * T + 2 * PREFETCH) * SP + 8 + Tpad + SP * PD + Tpad * PD) * 4


def fused_smem_bytes(T, SP, S, CP):
    return ((3 * T + 2 * PREFETCH) * SP + 8 + S * CP + 16 * CP) * 4


def image_states(SP, K):
    """the K padding of the gamma . Y product: a multiple of 4, and of 4 K where it was no multiple of K"""
    SP = (SP + 3) // 4 * 4
    if SP % K:
        SP = (SP + 4 * K - 1) // (4 * K) * (4 * K)
    return SP


# ---- the rules -------------------------------------------------------------------------------------------------------
def _answer(family, **kw):
    out = dict.fromkeys(FIELDS, 0)
    out.update(kw, family=FAMILIES.index(family))
    return out


def _unsupported(why):
    return dict(_answer("unsupported"), why=why)


def expected_loss(q):
    K, SP = lane_states(q.S)
    if K > 4:
        return _unsupported("S > 256")
    T, B, C = q.T, q.B, q.C
    if T <= (PIPE_MAX_T if K == 1 else MFMA_MAX_T) and C <= 256 and not q.sw & VALU:
        SPq = image_states(SP, K)
        Tpad, PD, ch = (T + 15) // 16 * 16, image_pitch(C), (C + WAVE - 1) // WAVE
        wt = int(8 * T * B * C <= WT_BYTES)
        if K == 1 and not q.sw & NOPIPE and not q.sw & NOFLOW and T <= FLOW_MAX_T and ch <= 3:
            PF = flow_pitch(C)
            if flow_smem_bytes(T, SPq, PF, C) <= MAX_LDS:
                return _answer("flow", K=1, SP=SPq, ch=ch, wt=wt, pd=PF, grid=B, lds=flow_smem_bytes(T, SPq, PF, C))
        if K == 1 and not q.sw & NOPIPE and pipe_smem_bytes(T, SPq, PD) <= MAX_LDS:
            return _answer("pipe", K=1, SP=SPq, ch=ch, wt=wt, pd=PD, grid=B, lds=pipe_smem_bytes(T, SPq, PD))
        if mfma_smem_bytes(T, Tpad, SPq, PD) <= MAX_LDS and T <= MFMA_MAX_T:
            return _answer("mfma", K=K, SP=SPq, ch=ch, wt=wt, Tpad=Tpad, pd=PD, grid=B,
                           lds=mfma_smem_bytes(T, Tpad, SPq, PD))
    smem = fused_smem_bytes(T, SP, q.S, C | 1)              # (the unpadded SP; it has no write-through form)
    if smem > MAX_LDS:
        return _unsupported("fused arrays beyond LDS")
    return _answer("fused", K=K, SP=SP, grid=B, lds=smem)


def expected_posteriors(q):
    """reads no diagnostic switch; the streamed or the pipelined kernel, always with write-through stores"""
    T, B, C, S = q.T, q.B, q.C, q.S
    if S > WAVE or T > PIPE_MAX_T or C > 256:
        return _unsupported("posteriors outside the pipelined kernel's shapes")
    SP, ch = (S + 3) // 4 * 4, (C + WAVE - 1) // WAVE
    if T <= FLOW_MAX_T and ch <= 3:
        PF = flow_pitch(C)
        if flow_smem_bytes(T, SP, PF, C) <= MAX_LDS:
            return _answer("flow", K=1, SP=SP, ch=ch, wt=1, pd=PF, grid=B, lds=flow_smem_bytes(T, SP, PF, C))
    PD = image_pitch(C)
    if pipe_smem_bytes(T, SP, PD) > MAX_LDS:
        return _unsupported("posteriors: images beyond LDS")
    return _answer("pipe", K=1, SP=SP, ch=ch, wt=1, pd=PD, grid=B, lds=pipe_smem_bytes(T, SP, PD))


class Query:
    def __init__(self, T, B, C, S, dtype=F32, want_gamma=False, sw=0):
        self.T, self.B, self.C, self.S, self.dtype, self.want_gamma, self.sw = T, B, C, S, dtype, want_gamma, sw

    def key(self):
        return (self.T, self.B, self.C, self.S, self.dtype, self.want_gamma, self.sw)


def expected(q):
    return expected_posteriors(q) if q.want_gamma else expected_loss(q)


def kernel_name(got):
    """the names tests/lattice_inputs_ref.py gives the binary kernels: flow, pipe, mfma<K>, valu<K> (the fused kernel)"""
    family = FAMILIES[got["family"]]
    return {"flow": "flow", "pipe": "pipe", "mfma": "mfma%d" % got["K"], "fused": "valu%d" % got["K"]}.get(family, family)


CALLS = [dict(), dict(want_gamma=True), dict(want_gamma=True, dtype=BF16), dict(want_gamma=True, dtype=F16)]
TS = (1, 15, 16, 17, 159, 160, 161, 167, 168, 169, 400)
CS = (1, 63, 64, 65, 128, 129, 158, 192, 193, 255, 256, 257)
SS = (1, 20, 61, 62, 63, 64, 65, 66, 127, 128, 129, 130, 255, 256, 257)
BS = (1, 2, 256, 2048)
SWITCHES = range(8)
# (T, C, S) where a kernel's own LDS need decides, found by a search over T <= 168, C <= 256, S <= 256 with these
# formulas: the last shape a kernel takes and the first it does not, along T and along S
LDS_EDGES = {
    # one, two and three column chunks; the first of each pair has 163 248, 163 136 and 163 312 of 163 840 bytes
    "flow": [(128, 64, 64), (129, 64, 64), (127, 128, 40), (128, 128, 40), (157, 158, 20), (158, 158, 20)],
    # (168, 158, 20) needs 163 840 bytes exactly; behind the streamed kernel's own limit; four column chunks
    "pipe": [(168, 158, 20), (139, 64, 64), (140, 64, 64), (140, 128, 40), (141, 128, 40), (111, 256, 20), (112, 256, 20)],
    # K = 4: 160 128 bytes at T = 80; K = 2: 163 264 bytes at T = 149
    "mfma": [(80, 12, 130), (81, 12, 130), (90, 12, 130), (149, 12, 70), (150, 12, 70)],
    # the last shape of all, one, two and four states per lane: beyond it nothing takes the call
    "fused": [(150, 158, 62), (151, 158, 62), (165, 64, 70), (166, 64, 70), (95, 12, 130), (96, 12, 130)],
}


def wt_edge(T, C):
    """the largest batch whose logits + gradient stay within the write-through threshold"""
    return max(1, WT_BYTES // (8 * T * C))


def grid():
    qs = []
    for T, C in itertools.product(TS, CS):
        for B, S, sw, call in itertools.product(BS + (wt_edge(T, C), wt_edge(T, C) + 1), SS, SWITCHES, CALLS):
            qs.append(Query(T, B, C, S, sw=sw, **call))
    for T, C, S in itertools.chain(*LDS_EDGES.values()):
        for B, sw, call in itertools.product((2, wt_edge(T, C) + 1), SWITCHES, CALLS):
            qs.append(Query(T, B, C, S, sw=sw, **call))
    return list({q.key(): q for q in qs}.values())


@pytest.fixture(scope="module")
def plan():
    entry = binary_plan_entry()
    return lambda q: entry(q.T, q.B, q.C, q.S, q.dtype, q.want_gamma, q.sw)


def test_grid_covers_every_family_and_threshold():
    qs = grid()
    ans = [expected(q) for q in qs]
    fam = lambda a: FAMILIES[a["family"]]
    plain = [(q, a) for q, a in zip(qs, ans) if not q.want_gamma and q.sw == 0]      # the loss, default switches
    assert {(fam(a), a["ch"]) for _, a in plain if fam(a) == "flow"} == {("flow", 1), ("flow", 2), ("flow", 3)}
    assert any(fam(a) == "pipe" and q.T > FLOW_MAX_T for q, a in plain)
    assert any(fam(a) == "pipe" and a["ch"] == 4 and q.T <= FLOW_MAX_T for q, a in plain)
    assert {a["K"] for _, a in plain if fam(a) == "mfma"} == {2, 4}
    assert {a["K"] for _, a in plain if fam(a) == "fused"} == {1, 2, 4}
    assert any(fam(a) == "mfma" and a["K"] == 1 and q.sw & NOPIPE for q, a in zip(qs, ans))
    assert {a["ch"] for a in ans if fam(a) == "mfma"} == {1, 2, 3, 4}
    for dtype in (F32, BF16, F16):                           # the posteriors: streamed, pipelined or nothing
        assert {fam(a) for q, a in zip(qs, ans) if q.want_gamma and q.dtype == dtype} == {"unsupported", "flow", "pipe"}
    assert {a["why"] for a in ans if "why" in a} == {
        "S > 256", "fused arrays beyond LDS", "posteriors outside the pipelined kernel's shapes",
        "posteriors: images beyond LDS"}
    assert {q.sw for q in qs} == set(SWITCHES)
    # both sides of every LDS limit among the shapes where that limit decides, of both time limits, of the three column
    # chunks and of the write-through threshold in every family that has the two forms
    def both(f, pick=lambda q: True):
        return {f(q) for q in qs if pick(q)} == {False, True}
    sp = lambda q: image_states(lane_states(q.S)[1], lane_states(q.S)[0])
    k1 = lambda q: not q.want_gamma and q.sw == 0 and q.S <= WAVE and q.C <= 256
    assert both(lambda q: flow_smem_bytes(q.T, sp(q), flow_pitch(q.C), q.C) > MAX_LDS,
                lambda q: k1(q) and q.T <= FLOW_MAX_T and q.C <= 192)
    assert both(lambda q: pipe_smem_bytes(q.T, sp(q), image_pitch(q.C)) > MAX_LDS,
                lambda q: k1(q) and q.T <= PIPE_MAX_T and fam(expected(q)) != "flow")
    assert both(lambda q: mfma_smem_bytes(q.T, (q.T + 15) // 16 * 16, sp(q), image_pitch(q.C)) > MAX_LDS,
                lambda q: not q.want_gamma and q.sw == 0 and WAVE < q.S <= 256 and q.T <= MFMA_MAX_T and q.C <= 256)
    assert both(lambda q: fused_smem_bytes(q.T, lane_states(q.S)[1], q.S, q.C | 1) > MAX_LDS,
                lambda q: not q.want_gamma and q.S <= 256 and fam(expected(q)) in ("fused", "unsupported"))
    assert any(pipe_smem_bytes(q.T, sp(q), image_pitch(q.C)) == MAX_LDS for q in qs if k1(q))
    have = lambda attr, *vals: all(any(getattr(q, attr) == v for q in qs) for v in vals)
    assert have("T", 160, 161, 168, 169) and have("C", 64, 65, 128, 129, 192, 193, 256, 257)
    assert have("S", 61, 64, 65, 66, 128, 129, 130, 256, 257)
    assert {a["SP"] - lane_states(q.S)[1] for q, a in plain if fam(a) in ("flow", "pipe", "mfma")} == {0, 1, 2, 3}
    assert {a["SP"] - lane_states(q.S)[1] for q, a in plain if fam(a) == "fused"} == {0}
    for family in ("flow", "pipe", "mfma"):
        assert {a["wt"] for q, a in zip(qs, ans) if not q.want_gamma and fam(a) == family} == {0, 1}, family
    assert {a["wt"] for q, a in zip(qs, ans) if q.want_gamma and fam(a) != "unsupported"} == {1}
    assert {a["wt"] for a in ans if fam(a) == "fused"} == {0}
    assert both(lambda q: 8 * q.T * q.B * q.C > WT_BYTES, lambda q: (q.T, q.C) == (160, 158))


def test_plan_matches_the_restated_rules(plan):
    wrong = []
    for q in grid():
        want = {k: v for k, v in expected(q).items() if k != "why"}
        got = plan(q)
        if got != want:
            wrong.append((q.key(), {k: (got[k], want[k]) for k in FIELDS if got[k] != want[k]}))
    assert not wrong, "%d calls planned differently, the first: %r" % (len(wrong), wrong[:5])


def test_named_shapes_reach_the_kernels_they_are_named_after(plan):
    """what the GPU tests rely on and only say in words: the shapes of tests/lattice_inputs_ref.py, the binary rows of the
    call-site table of tests/test_batch_sum_gpu.py at every batch size they run, the binary shapes of
    tests/test_token_spans_gpu.py (the loss on them: one, one and two states per lane)"""
    from tests.lattice_inputs_ref import BINARY_KERNEL, BINARY_SHAPES, POSTERIOR_SHAPES
    from tests.test_batch_sum_gpu import SITES
    from tests.test_token_spans_gpu import BINARY
    loss = lambda T, B, C, S: plan(Query(T, B, C, S))
    for name, (T, B, C, S) in BINARY_SHAPES.items():
        assert kernel_name(loss(T, B, C, S)) == BINARY_KERNEL[name], name
    assert {BINARY_KERNEL[p] for p in BINARY_SHAPES} == {"flow", "pipe", "mfma2", "mfma4", "valu1"}
    assert loss(*BINARY_SHAPES["flow"])["ch"] == 1 and loss(*BINARY_SHAPES["flow_c158"])["ch"] == 3
    assert loss(*BINARY_SHAPES["pipe_c"])["ch"] == 4 and loss(*BINARY_SHAPES["mfma_k4"])["lds"] == 160128
    got = [kernel_name(plan(Query(*BINARY_SHAPES[p], want_gamma=True))) for p in POSTERIOR_SHAPES["binary"]]
    assert got == ["flow", "pipe"]
    rows = {"binary-flow": "flow", "binary-pipe_t": "pipe", "binary-pipe_c": "pipe", "binary-mfma_k2": "mfma2",
            "binary-fused": "valu1"}
    assert sorted(rows) == sorted(n for n in SITES if SITES[n][0] == "binary")
    for name, want in rows.items():
        _, (T, C, S), batches, _ = SITES[name]
        for B in batches:
            assert kernel_name(loss(T, B, C, S)) == want, (name, B)
    assert [kernel_name(loss(*shape)) for shape in BINARY] == ["flow", "flow", "flow", "mfma2"]
    assert [loss(*shape)["ch"] for shape in BINARY] == [1, 3, 1, 1]


def test_plan_entry_rejects_empty_shapes():
    from ctc_amd import build
    fn = ctypes.CDLL(build.build_diag()).ctc_amd_debug_binary_plan
    assert fn(0, 1, 2, 1, 0, 0, 0, None) == -1
