"""The read-outs of the no-blank and the binary lattice on bf16 / fp16 logits read natively (the *_typed entries behind
noblank_/binary_ best_path, posteriors and token_spans) on the device.  The contract is bitwise, no tolerances:
every output -- path, score, nll, gamma, frame_conf, start, end, conf -- equals what the same function returns on
logits.float(), compared through int32 views so that -inf / +inf count.  That is derived, not measured: a 2-byte element
widens to fp32 exactly, the same lane reads the same element, and everything behind the load is the fp32 kernel's code.

Shapes: the smallest at which the new loads can go wrong -- the reference's own sizes (odd C: rows that are only 2-byte
aligned), three column chunks with a tail, both binary posterior kernels on both kinds of tiles, two and four states per lane,
views (transposed, an odd row stride behind a base offset of one element, a class stride of 2), special values, a sample
without an alignment; and which entry ran: the typed one wherever it takes the shape, the cast in front of the untyped one
only for noblank_posteriors outside the r16 kernel's domain."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
dt_id = lambda d: str(d).split(".")[-1]        # noqa: E731
NAMES = ["noblank_best_path", "noblank_posteriors", "noblank_token_spans",
         "binary_best_path", "binary_posteriors", "binary_token_spans"]
SPAN_FIELDS = ("start", "end", "conf", "frame_conf", "path", "score", "nll")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    import ctc_amd  # noqa: F401
    return torch.device("cuda:0")


@pytest.fixture
def calls(monkeypatch):
    """(entry, x_dtype code or None, stride_t, stride_b, return code) of every read-out call that reaches the library"""
    from ctc_amd import _lib
    seen = []
    real = _lib.load()

    class Spy:
        def __getattr__(self, name):
            fn = getattr(real, name)
            if not any(k in name for k in ("best_path", "posteriors", "token_spans")):
                return fn

            def call(*a):
                rc = fn(*a)
                typed = name.endswith("_typed")
                seen.append((name, a[1] if typed else None, a[2 if typed else 1], a[3 if typed else 2], rc))
                return rc
            return call
    monkeypatch.setattr(_lib, "load", lambda: Spy())
    return seen


def _entries(calls):
    return [c[0] for c in calls]


def _fn(name):
    import ctc_amd
    return getattr(ctc_amd, name)


def _code(dtype):
    from ctc_amd import _lib
    return {torch.bfloat16: _lib.BF16, torch.float16: _lib.F16}[dtype]


def _case(dev, seed, T, B, C, S, dtype, lattice, soft=False, no_align=None, max_len=None, classes=None):
    """seeded inputs: logits 3 randn rounded to dtype, ragged lengths (1 <= L_b <= min(S, max_len), L_b <= T_b <= T, the first
    sample short of both T and S); no_align: a sample with L_b > T_b; classes: the labels / multi-hot columns come from
    [0, classes)"""
    g = torch.Generator().manual_seed(seed)
    x = (3 * torch.randn(T, B, C, generator=g)).to(dtype)
    top = min(S, T, max_len or S)
    L = torch.randint(1, top + 1, (B,), generator=g)
    Tb = torch.stack([torch.randint(int(l), T + 1, (1,), generator=g)[0] for l in L])
    L[0] = max(1, min(int(L[0]), S - 1, T - 1))
    Tb[0] = max(int(L[0]), min(int(Tb[0]), T - 1))
    if no_align is not None:
        L[no_align] = max(2, int(L[no_align]))
        Tb[no_align] = int(L[no_align]) - 1
    nc = C if classes is None else classes
    if lattice == "noblank":
        tg = torch.randint(0, nc, (B, S), generator=g, dtype=torch.int32)
        tg[torch.arange(S)[None, :] >= L[:, None]] = -1
    else:
        tg = torch.rand(B, S, C, generator=g) if soft else (torch.rand(B, S, C, generator=g) < 0.1).float()
        tg[:, :, nc:] = 0.0
        tg[torch.arange(S)[None, :] >= L[:, None]] = 0.0
    return x.to(dev), tg.to(dev), Tb.long().to(dev), L.long().to(dev)


def _flat(out):
    return list(zip(SPAN_FIELDS, out)) if len(out) == 7 else list(zip(("out", "per_sample"), out))


def _assert_bitwise(got, want, what):
    got, want = _flat(got), _flat(want)
    assert len(got) == len(want)
    for (k, a), (_, b) in zip(got, want):
        assert a.dtype is b.dtype and a.shape == b.shape and a.dtype in (torch.int32, torch.float32), (what, k)
        assert torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)), "%s: %s differs" % (what, k)


def _check(name, calls, xl, tg, Tb, L, typed=True, what=""):
    """name on xl against name on xl.float(): bits, and which entries ran"""
    fn = _fn(name)
    del calls[:]
    got = fn(xl, tg, Tb, L)
    mine = list(calls)
    del calls[:]
    want = fn(xl.float(), tg, Tb, L)
    torch.cuda.synchronize()
    assert _entries(calls) == ["ctc_amd_" + name] and calls[0][4] == 0, (name, what, calls)
    if typed:
        assert _entries(mine) == ["ctc_amd_%s_typed" % name], (name, what, mine)
        assert mine[0][1] == _code(xl.dtype) and mine[0][4] == 0, (name, what, mine)
    else:                                       # refused by the typed entry, then the cast and the untyped one
        assert _entries(mine) == ["ctc_amd_%s_typed" % name, "ctc_amd_" + name], (name, what, mine)
        assert mine[0][4] == -2 and mine[1][4] == 0, (name, what, mine)
    _assert_bitwise(got, want, "%s %s" % (name, what))
    return got


# ---------------------------------------------------------------------------------------------- 1. the reference's sizes
@pytest.mark.parametrize("dtype", DTYPES, ids=dt_id)
@pytest.mark.parametrize("name", NAMES)
def test_reference_sizes(dev, calls, name, dtype):
    """T = 10, B = 10, C = 33, S = 5: C is odd, so every row but the first starts at an address that is only 2-byte aligned.
    noblank_posteriors is outside the r16 kernel's domain here (odd C): the cast, and what the fp32 call answers"""
    lattice = name.split("_")[0]
    xl, tg, Tb, L = _case(dev, 1, 10, 10, 33, 5, dtype, lattice)
    assert int(Tb.min()) < 10 and int(L.min()) < 5
    if name != "noblank_posteriors":
        _check(name, calls, xl, tg, Tb, L)
        return
    fn = _fn(name)
    try:
        want = fn(xl.float(), tg, Tb, L)
    except Exception as e:          # noqa: BLE001 -- whatever the fp32 call raises, the 2-byte call raises too
        with pytest.raises(type(e)):
            fn(xl, tg, Tb, L)
        return
    _check(name, calls, xl, tg, Tb, L, typed=False)
    assert want[0].shape == (10, 10, 5)


# ---------------------------------------------------------------------------------------- 2. column chunks and their tails
@pytest.mark.parametrize("dtype", DTYPES, ids=dt_id)
@pytest.mark.parametrize("name,C", [(n, 158) for n in NAMES] + [("noblank_posteriors", 34)])
def test_column_chunks_and_no_alignment(dev, calls, name, C, dtype):
    """T = 37, B = 3, S = 20; C = 158: three 64-column chunks, a tail of 30; C = 34: one short chunk.  Sample 1 has
    L_b > T_b: path -1, score -inf, nll +inf (the posteriors' nll: the loss's sentinel), gamma zeros, as fp32 gives"""
    lattice = name.split("_")[0]
    xl, tg, Tb, L = _case(dev, 2 + C, 37, 3, C, 20, dtype, lattice, no_align=1)
    assert int(L[1]) > int(Tb[1])
    got = _check(name, calls, xl, tg, Tb, L, what="C=%d" % C)
    inf = float("inf")
    if "best_path" in name:
        assert bool((got[0][1] == -1).all()) and float(got[1][1]) == -inf and bool((got[0][0, :int(Tb[0])] >= 0).all())
    elif "posteriors" in name:
        # (the posteriors report a sample without an alignment as the loss does: the reference's sentinel magnitude, 1e13)
        assert float(got[0][1].abs().max()) == 0.0 and float(got[1][1]) > 1e12
        rows = got[0][0, :int(Tb[0])].sum(1)
        assert bool(((rows - 1).abs() < 1e-3).all())
    else:
        assert bool((got.path[1] == -1).all()) and float(got.score[1]) == -inf and float(got.nll[1]) == inf
        assert bool((got.start[1] == -1).all()) and float(got.conf[1].abs().max()) == 0.0
        assert int(got.start[0, 0]) == 0 and int(got.end[0, int(L[0]) - 1]) == int(Tb[0])


# ------------------------------------------------------------------------------------------ 3. both binary posterior kernels
@pytest.mark.parametrize("dtype", DTYPES, ids=dt_id)
@pytest.mark.parametrize("soft", [False, True], ids=["multihot", "soft"])
@pytest.mark.parametrize("C,T", [(200, 24), (33, 165), (33, 24), (158, 24)], ids=["pipe-4chunks", "pipe-165rows", "flow-33", "flow-158"])
def test_binary_posterior_kernels(dev, calls, C, T, soft, dtype):
    """C = 200: four chunks, and T = 165: beyond the flow kernel's 160 rows -- the pipe kernel; the other two the flow kernel.
    Multi-hot targets are exact in bf16 (the bf16 MFMA tiles), soft ones are not (the fp32 tiles)"""
    xl, tg, Tb, L = _case(dev, 3 + C + T, T, 3, C, 6, dtype, "binary", soft=soft)
    got = _check("binary_posteriors", calls, xl, tg, Tb, L, what="C=%d T=%d soft=%s" % (C, T, soft))
    rows = got[0][0, :int(Tb[0])].sum(1)
    assert bool(((rows - 1).abs() < 1e-3).all())


# ------------------------------------------------------------------------------ 4. more than one state per lane (decode kernels)
@pytest.mark.parametrize("dtype", DTYPES, ids=dt_id)
@pytest.mark.parametrize("S", [70, 130], ids=["K2", "K4"])
@pytest.mark.parametrize("name", [n for n in NAMES if "posteriors" not in n])
def test_states_per_lane(dev, calls, name, S, dtype):
    """S = 70: two states per lane, S = 130: four; T = 40, B = 2, C = 7, L_b <= 30"""
    lattice = name.split("_")[0]
    xl, tg, Tb, L = _case(dev, 4 + S, 40, 2, 7, S, dtype, lattice, max_len=30)
    assert int(L.max()) <= 30
    got = _check(name, calls, xl, tg, Tb, L, what="S=%d" % S)
    path = got[0] if "best_path" in name else got.path
    assert bool((path[0, :int(Tb[0])] >= 0).all()) and int(path[0, int(Tb[0]) - 1]) == int(L[0]) - 1


# ---------------------------------------------------------------------------------------------------------------- 5. views
def _view(xl, layout):
    """the same values behind another layout"""
    T, B, C = xl.shape
    if layout == "transposed":                  # the [T,B,C] transpose of a [B,T,C] tensor
        v = xl.transpose(0, 1).contiguous().transpose(0, 1)
        assert v.stride() == (C, T * C, 1)
    elif layout == "offset":                    # wide[..., 1:]: unit class stride, odd row stride, base offset of one element
        wide = torch.zeros(T, B, C + 1, dtype=xl.dtype, device=xl.device)
        wide[..., 1:] = xl
        v = wide[..., 1:]
        assert v.stride() == (B * (C + 1), C + 1, 1) and (C + 1) % 2 == 1 and v.data_ptr() % 4 == 2
    else:                                       # a class stride of 2
        wide = torch.zeros(T, B, 2 * C, dtype=xl.dtype, device=xl.device)
        wide[..., ::2] = xl
        v = wide[..., ::2]
        assert v.stride(2) == 2
    assert torch.equal(v, xl)
    return v


@pytest.mark.parametrize("dtype", DTYPES, ids=dt_id)
@pytest.mark.parametrize("layout", ["transposed", "offset", "strided"])
@pytest.mark.parametrize("name", NAMES)
def test_views(dev, calls, name, layout, dtype):
    """T = 12, B = 4, C = 34, S = 4.  Every entry reads the view where it lies, except: noblank_posteriors behind an odd row
    stride and a 2-byte aligned base (outside the r16 kernel's domain: the cast), and a class stride of 2, which is copied in
    its own dtype and then read by the typed entry"""
    T, B, C, S = 12, 4, 34, 4
    lattice = name.split("_")[0]
    xl, tg, Tb, L = _case(dev, 5, T, B, C, S, dtype, lattice)
    v = _view(xl, layout)
    fallback = name == "noblank_posteriors" and layout == "offset"
    _check(name, calls, v, tg, Tb, L, typed=not fallback, what=layout)
    # the strides the typed entry was given: the view's own, or those of the dense copy in the view's dtype
    del calls[:]
    _fn(name)(v, tg, Tb, L)
    want = (B * C, C) if layout == "strided" else tuple(v.stride()[:2])
    assert calls[0][0] == "ctc_amd_%s_typed" % name and calls[0][1] == _code(dtype) and calls[0][2:4] == want


# -------------------------------------------------------------------------------------------------------- 6. special values
@pytest.mark.parametrize("dtype", DTYPES, ids=dt_id)
@pytest.mark.parametrize("name", NAMES)
def test_special_values(dev, calls, name, dtype):
    """T = 16, B = 2, C = 34, S = 4; targets use the classes below 30.  fp16: subnormals (a widening that flushed them would
    change every sum they enter), +-65504, and -inf on classes no target uses; bf16: +-1e30 and -inf likewise.  On the binary
    lattice -inf and +-1e30 hit the +-128 clamp of the two logs.  Sample 0 keeps the extremes off its label classes' maxima
    (it has an alignment with ordinary numbers), sample 1 takes the large positive values too"""
    T, B, C, S = 16, 2, 34, 4
    lattice = name.split("_")[0]
    xl, tg, Tb, L = _case(dev, 6, T, B, C, S, dtype, lattice, classes=30)
    x = xl.clone()
    ninf = float("-inf")
    if dtype is torch.float16:
        x[0::3, :, 3] = 6e-8
        x[1::3, :, 7] = -6e-5
        x[2::3, :, 11] = 6e-8
        x[::2, :, 31] = -65504.0
        x[1::4, 1, 32] = 65504.0
        assert float(x[0, 0, 3]) != 0.0 and float(x[1, 0, 7]) != 0.0 and abs(float(x[0, 0, 3])) < 6.2e-5   # subnormal, kept
    else:
        x[::2, :, 31] = -1e30
        x[1::4, 1, 32] = 1e30
    x[::3, :, 33] = ninf
    x[1::5, 0, 30] = ninf
    got = _check(name, calls, x, tg, Tb, L)
    path = got[0] if "best_path" in name else got.path if "spans" in name else None
    if path is not None:
        assert bool((path[0, :int(Tb[0])] >= 0).all())


# ------------------------------------------------------------------------------------------------------ 7. which entry ran
@pytest.mark.parametrize("name", NAMES)
def test_float32_takes_the_untyped_entry(dev, calls, name):
    lattice = name.split("_")[0]
    xl, tg, Tb, L = _case(dev, 7, 12, 4, 34, 4, torch.bfloat16, lattice)
    _fn(name)(xl.float(), tg, Tb, L)
    torch.cuda.synchronize()
    assert _entries(calls) == ["ctc_amd_" + name] and calls[0][4] == 0


@pytest.mark.parametrize("name", NAMES)
def test_native_path_switched_off_is_the_cast(dev, calls, name, monkeypatch):
    """with no 2-byte dtype in `_LOWP_READOUT` (what tools/readout_typed_bench.py does) every function casts: the same bits"""
    from ctc_amd import functional
    lattice = name.split("_")[0]
    xl, tg, Tb, L = _case(dev, 8, 12, 4, 34, 4, torch.bfloat16, lattice)
    on = _fn(name)(xl, tg, Tb, L)
    monkeypatch.setattr(functional, "_LOWP_READOUT", {})
    del calls[:]
    off = _fn(name)(xl, tg, Tb, L)
    torch.cuda.synchronize()
    assert _entries(calls) == ["ctc_amd_" + name]
    _assert_bitwise(on, off, name)


# ------------------------------------------------------------------------------------------------------- 8. still refused
def test_still_refused(dev):
    import ctc_amd
    T, B, C, S = 12, 4, 34, 4
    lp = torch.randn(T, B, C, device=dev).log_softmax(2)
    tgt = torch.randint(1, C, (B, S), device=dev)
    il, tl = torch.full((B,), T, device=dev), torch.full((B,), S, device=dev)
    for fn in (ctc_amd.blank_best_path, ctc_amd.blank_posteriors, ctc_amd.blank_token_spans):
        for dt in DTYPES:
            with pytest.raises(ValueError):
                fn(lp.to(dt), tgt, il, tl)
    with pytest.raises(ValueError):
        ctc_amd.noblank_best_path(lp.double(), tgt, il, tl)
    with pytest.raises(ValueError):
        ctc_amd.binary_posteriors(lp.double(), torch.zeros(B, S, C, device=dev), il, tl)
