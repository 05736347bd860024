"""tests/batch_sum_ref.py without a GPU: the packed word's fields cannot carry, the shards count every sample, the two
expected-loss functions on hand-worked examples, the closed-form nll of the steerable inputs against the float64 oracle,
and (the diagnostics build, as tests/test_noblank_plan.py) which kernel every no-blank shape of the GPU tests reaches."""
import numpy as np
import pytest

from oracle import ctc_numpy
from tests import batch_sum_ref as ref
from tests.helpers import NOBLANK_PLAN_FAMILIES as FAMILIES, noblank_plan_entry
from tests.test_noblank_plan import CUS

f32 = np.float32


# ---------------------------------------------------------------------------------------------- the packed word
def test_no_field_of_the_packed_word_can_carry():
    for B in range(1, ref.ACC_MAX_B + 1):
        assert ref.field_width_problems(B) == [], B
    assert ref.frac_bits(1) == 27 and ref.frac_bits(2) == 26 and ref.frac_bits(256) == 19 and ref.frac_bits(257) == 18
    assert ref.frac_bits(4095) == 15
    # the margins: 4095 arrivals / non-fitting values fill twelve bits exactly, a shard has at most 256 members
    assert ref.ACC_MAX_B == (1 << ref.COUNT_BITS) - 1
    assert max(ref.shard_members(4095, sh) for sh in range(16)) == 256
    # ... and the check itself notices a field that is one bit short
    largest = np.nextafter(f32(8192), f32(0))
    assert 4096 * ref.quantum(largest, ref.frac_bits(4095)) < 1 << 40 <= 4097 * ref.quantum(f32(8192), 15)


def test_shards_count_every_sample_once():
    for B in range(1, 4201):
        members = [ref.shard_members(B, sh) for sh in range(ref.ACC_SHARDS)]
        assert sum(members) == B, B
        assert min(members) >= 0
        if B in (1, 2, 15, 16, 17, 31, 33, 255, 257, 4095, 4200):
            assert members == [len(range(sh, B, 16)) for sh in range(16)], B
    assert [ref.shard_members(3, sh) for sh in range(16)] == [1, 1, 1] + [0] * 13          # empty shards
    assert [ref.shard_members(17, sh) for sh in range(16)] == [2] + [1] * 15              # uneven ones


# ---------------------------------------------------------------------------------------------- expected_sum_loss
def test_sum_loss_rounds_ties_to_even():
    # B = 2: F = 26.  Values k + 1/2 quanta: 0.5 -> 0, 1.5 -> 2, 2.5 -> 2 (half to even); the sum is 4 quanta, not 4.5
    q = 2.0 ** -26
    nll = np.array([1.5 * q, 2.5 * q], f32)
    e = ref.expected_sum_loss(nll, 2, f32(0.5))
    assert e.all_fit and e.value == f32(4 * q * 0.5) and e.mean == 4 * q * 0.5
    e = ref.expected_sum_loss(np.array([0.5 * q, 2.5 * q], f32), 2, f32(0.5))
    assert e.value == f32(2 * q * 0.5) and abs(float(e.value) - e.mean) == 0.5 * q      # one whole quantum lost in the sum
    assert e.bound >= 0.5 * q                                                           # ... which is the contract's B 2^-(F+1) scale
    assert ref.check_loss(e.value, e) == []
    assert ref.check_loss(f32(3 * q * 0.5), e) != []                                    # round-half-up: caught, bit for bit
    # B = 1: F = 27, an fp32 value below 2^-3 is a multiple of 2^-27 only if its mantissa allows it
    e = ref.expected_sum_loss(np.array([3.0 * 2.0 ** -27], f32), 1, f32(1.0))
    assert e.value == f32(3.0 * 2.0 ** -27)


def test_sum_loss_adds_what_does_not_fit_in_double():
    B = 4
    nll = np.array([1.0, 1e13, 2.0, 0.25], f32)
    e = ref.expected_sum_loss(nll, B, f32(0.25))
    total = float(f32(1e13)) + 3.25
    assert not e.all_fit and e.value == f32(total * 0.25) and e.mean == total * 0.25
    assert ref.check_loss(f32(total * 0.25), e) == []
    assert ref.check_loss(f32(3.25 * 0.25), e) != []                 # the sentinel dropped
    # 8192 itself does not fit; the value just below does; a negative residue and -0.0
    e = ref.expected_sum_loss(np.array([8192.0, np.nextafter(f32(8192), f32(0)), -1e-6, -0.0], f32), 4, f32(1.0))
    assert list(ref.fits(np.array([8192.0, np.nextafter(f32(8192), f32(0)), -1e-6, -0.0], f32))) == [False, True, False, True]
    assert e.value == f32(8192.0 + float(np.nextafter(f32(8192), f32(0))) + float(f32(-1e-6)))
    # overflow of the fp32 loss is np.float32's: +inf
    e = ref.expected_sum_loss(np.array([3e38, 3e38], f32), 2, f32(1.0))
    assert np.isposinf(e.value) and ref.check_loss(f32(np.inf), e) == [] and ref.check_loss(f32(3e38), e) != []
    e = ref.expected_sum_loss(np.array([np.inf, 1.0], f32), 2, f32(0.5))
    assert np.isposinf(e.value)


def test_all_nan_and_one_nan():
    for nll in ([np.nan] * 3, [1.0, np.nan, 1e13]):
        e = ref.expected_sum_loss(np.array(nll, f32), 3, f32(1 / 3))
        assert np.isnan(e.value) and ref.check_loss(f32(np.nan), e) == [] and ref.check_loss(f32(1.0), e) != []
        e = ref.expected_ticket_loss(np.array(nll, f32), f32(1 / 3))
        assert np.isnan(e.value) and ref.check_loss(f32(np.nan), e) == [] and ref.check_loss(f32(np.inf), e) != []


def test_ticket_loss():
    t = np.array([1.0, 2.0, 3.5], f32)
    e = ref.expected_ticket_loss(t, f32(0.5))
    assert e.value == f32(3.25) and e.mean == 3.25
    assert e.bound == 7 * 2.0 ** -24 * 6.5 * 0.5 + float(np.spacing(f32(3.25)))
    e = ref.expected_ticket_loss(np.ones(4097, f32), f32(1.0))
    assert e.bound == (65 + 6) * 2.0 ** -24 * 4097 + float(np.spacing(f32(4097)))
    e = ref.expected_ticket_loss(np.array([1.0, np.inf], f32), f32(0.5))
    assert np.isposinf(e.value) and ref.check_loss(f32(np.inf), e) == [] and ref.check_loss(f32(1e30), e) != []
    # the blank loss: nll_b / max(L_b, 1) in fp32
    e = ref.expected_loss("blank", np.array([3.0, 5.0, 7.0], f32), 3, f32(1 / 3), L=np.array([0, 1, 2]))
    assert abs(e.mean - (3.0 + 5.0 + 3.5) * float(f32(1 / 3))) < 1e-15
    # which form serves which batch
    assert ref.expected_loss("noblank", np.ones(4095, f32), 4095, f32(1.0)).all_fit
    assert not ref.expected_loss("binary", np.ones(4096, f32), 4096, f32(1.0)).all_fit


def simulate_packed_sum(nll32, B, scale32, order):
    """NOT part of the reference (tests/batch_sum_ref.py states the result from the header's definition alone): the packed
    word of ctc_amd/csrc/common.hpp walked step by step in Python integers, samples arriving in `order` -- sixteen shard
    words, the top word, the list -> float32 loss.  It exists for one CPU test below: the reference's prediction must not
    depend on the arrival order, and no field may carry on the way."""
    F = ref.frac_bits(B)
    shards, top, lst, loss = [0] * ref.ACC_SHARDS, 0, [], None
    for b in order:
        v = np.float32(nll32[b])
        add = 1 << 52
        if ref.fits(v):
            add += ref.quantum(v, F)
        else:
            lst.append(b)
            add += 1 << ref.SUM_BITS
        sh = b % ref.ACC_SHARDS
        old = shards[sh]
        shards[sh] = old + add
        if old >> 52 != ref.shard_members(B, sh) - 1:
            continue
        word = old + add
        assert word < 1 << 64 and word >> 52 == ref.shard_members(B, sh)
        shards[sh] = 0
        old, top = top, top + word
        assert top < 1 << 64
        if (old >> 52) + (word >> 52) != B:
            continue
        assert loss is None
        s = np.float64(top & ((1 << ref.SUM_BITS) - 1)) * np.float64(2.0 ** -F)
        n = (top >> ref.SUM_BITS) & 0xFFF
        assert n == len(lst)
        with np.errstate(invalid="ignore"):
            for i in lst:
                s = s + np.float64(nll32[i])
        loss = ref._f32(s * np.float64(np.float32(scale32)))
        top, lst = 0, []
    assert loss is not None and not any(shards) and top == 0
    return loss


@pytest.mark.parametrize("B", [1, 3, 17, 33, 257])
def test_prediction_is_what_the_packed_word_gives_in_any_order(B):
    """the design, restated in integers (simulate_packed_sum), arrives at expected_sum_loss whatever the arrival order:
    all fitting (bit for bit), one sentinel among small values (bit for bit), several (within the float64 slack)"""
    rng = np.random.RandomState(B)
    scale = f32(1.0 / B)
    tiny = (rng.rand(B) * 1e-3).astype(f32)
    edge = np.where(rng.rand(B) < 0.5, np.nextafter(f32(8192), f32(0)), f32(8191.99)).astype(f32)
    one = tiny.copy()
    one[B // 2] = 1e13
    several = (rng.rand(B) * 9000).astype(f32)
    several[::3] = 1e13
    several[1::5] = 8192.0 + rng.rand(len(several[1::5])) * 100
    for nll in (tiny, edge, one, several):
        e = ref.expected_sum_loss(nll, B, scale)
        for _ in range(4):
            got = simulate_packed_sum(nll, B, scale, rng.permutation(B))
            assert ref.check_loss(got, e) == []
            if e.all_fit or e.slack == 0.0:
                assert got == e.value


# ---------------------------------------------------------------------------------------------- the inputs
def test_closed_forms_are_the_oracles_nll():
    """the per-sample nll the steerable inputs promise is what the float64 oracle computes on them (small batches, every
    regime, ragged lengths)"""
    for regime in ("tiny", "ordinary", "straddling", "mixed"):
        B = 12
        want = ref.regime_targets(regime, B)
        nb = ref.noblank_batch(8, 8, 2, ref.ragged_lengths(B, 8), want, no_alignment=[3], masked=[5])
        o = ctc_numpy.noblank_ctc(nb.x, nb.tgt, nb.Tb, nb.L, np.float64, want_grad=False)
        ok = ~nb.infeasible
        assert np.abs(o["nll"][ok] - nb.nll64[ok]).max() <= 1e-12 * np.maximum(1.0, nb.nll64[ok]).max(), regime
        assert (o["nll"][~ok] >= ref.INFEASIBLE).all() and list(np.nonzero(~ok)[0]) == [3, 5]
        assert np.abs(nb.nll64[ok] - want[ok]).max() <= 1e-3 * np.maximum(1.0, want[ok] / 100).max(), regime   # (M rounded to fp32)
        bi = ref.binary_batch(100, 8, 2, ref.ragged_lengths(B, 100, 95), want, no_alignment=[3])
        o = ctc_numpy.binary_ctc(bi.x, bi.tgt, bi.Tb, bi.L, np.float64, want_grad=False)
        ok = ~bi.infeasible
        assert np.abs(o["nll"][ok] - bi.nll64[ok]).max() <= 1e-11 * np.maximum(1.0, bi.nll64[ok]).max(), regime
        assert (o["nll"][~ok] >= ref.INFEASIBLE).all()
        br = ref.binary_random_batch(100, 8, 2, ref.ragged_lengths(B, 100, 95), B, no_alignment=[3])
        o = ctc_numpy.binary_ctc(br.x, br.tgt, br.Tb, br.L, np.float64, want_grad=False)
        ok = ~br.infeasible
        assert np.abs(o["nll"][ok] - br.nll64[ok]).max() <= 1e-11 * br.nll64[ok].max() and (o["nll"][~ok] >= ref.INFEASIBLE).all()
        bl = ref.blank_batch(8, 8, 2, ref.ragged_lengths(B, 8), want, no_alignment=[3], masked=[5])
        o = ctc_numpy.blank_ctc(bl.x, bl.tgt, bl.Tb, bl.L, np.float64, want_grad=False)
        ok = ~bl.infeasible
        assert np.abs(o["nll"][ok] - bl.nll64[ok]).max() <= 1e-11 * np.maximum(1.0, np.abs(bl.nll64[ok])).max(), regime
        assert np.isposinf(o["nll"][~ok]).all() and list(np.nonzero(~ok)[0]) == [3, 5]


@pytest.mark.parametrize("family,T,C", [("noblank", 8, 8), ("noblank", 8, 9), ("binary", 100, 8), ("blank", 8, 8)])
def test_straddling_values_keep_clear_of_the_limit(family, T, C):
    """half of a straddling batch on either side of 8192, none within 0.25 of it (the kernels' fp32 nll is good to 1e-5
    relative: 0.08 there), at every batch size the GPU tests use"""
    for B in (17, 257, 513, 4095, 4097):
        b = ref.BUILDERS[family](T, C, 2, T, ref.regime_targets("straddling", B))
        d = b.nll64 - ref.ACC_LIMIT
        assert np.abs(d).min() >= 0.25, (B, np.abs(d).min())
        assert (d < 0).sum() >= B // 4 and (d > 0).sum() >= B // 4
        assert (d < 0).sum() + (d > 0).sum() == B


def test_mixed_batches_reach_every_shard_with_both_kinds():
    for B in (257, 513, 4095):
        want = ref.regime_targets("mixed", B)
        fit = want < ref.ACC_LIMIT
        for sh in range(16):
            assert fit[sh::16].any() and (~fit[sh::16]).any(), (B, sh)


# ---------------------------------------------------------------------------------------------- which kernel runs
# The no-blank shapes of tests/test_batch_sum_gpu.py (T, C, S) -> what each must reach, by batch size.
NOBLANK_SITES = {
    # name: (T, C, S), batch sizes, want_grad, (family, {field: value})
    "r16":            ((8, 8, 2), (1, 17, 512, 513, 4095, 4096, 5000), False, ("r16", dict(ps=0))),
    "r16 small":      ((8, 8, 2), (1, 17, 256, 512), True, ("r16", dict(ps=0))),
    "r16 ps":         ((8, 8, 2), (513, 1023, 4095, 4096, 5000), True, ("r16", dict(ps=1, grid=CUS))),
    "xr":             ((8, 9, 2), (1, 256, 257, 4095, 4096, 5000), True, ("xr", dict())),
    "xr dual":        ((8, 9, 2), (257, 4095, 4096), True, ("xr", dict(dual=1))),
    "pipelined":      ((168, 9, 40), (1, 17, 257, 513, 4095, 4096), True, ("pipelined", dict(dual=0))),
    "pipelined dual": ((100, 9, 40), (257, 513, 4095, 4096), True, ("pipelined", dict(dual=1))),
    "fused K=1":      ((169, 8, 2), (1, 257, 4095, 4096, 5000), True, ("fused", dict(K=1, glb=0))),
    "fused K=2":      ((20, 8, 70), (1, 513, 4095, 4096), True, ("fused", dict(K=2, glb=0))),
    "fused K=4":      ((20, 8, 130), (1, 513, 4095, 4096), True, ("fused", dict(K=4, glb=0))),
    "fused glb":      ((212, 9, 64), (1, 17, 257, 513), True, ("fused", dict(glb=1))),
    "fused C>256":    ((8, 258, 2), (17, 257), True, ("fused", dict(K=1, ch=0, glb=0))),          # the generic rows
}


@pytest.fixture(scope="module")
def plan():
    entry = noblank_plan_entry()
    return lambda T, B, C, S, want_grad: entry(T, B, C, S, 0, B * C, C, 0, 0, want_grad, 0, 0, CUS, 0)   # contiguous fp32


@pytest.mark.parametrize("name", sorted(NOBLANK_SITES))
def test_gpu_shapes_reach_their_call_sites(plan, name):
    """with 256 compute units, contiguous fp32 logits: every row of the table reaches its kernel, on both sides of
    B = 4095 where the row has both -- a changed selection rule cannot quietly empty a row of the GPU tests"""
    (T, C, S), batches, want_grad, (family, fields) = NOBLANK_SITES[name]
    for B in batches:
        got = plan(T, B, C, S, want_grad)
        assert FAMILIES[got["family"]] == family, (name, B, FAMILIES[got["family"]])
        for k, v in fields.items():
            assert got[k] == v, (name, B, k, got[k])
