"""Token spans on the no-blank and the binary lattice on the MI355X: noblank_token_spans / binary_token_spans against
the best-path calls (path and score bit for bit), against the float64 oracle (nll, and gamma gathered at the returned
path), and against the numpy restatement of the span stage (tests/test_token_spans_abi.py, bit for bit); the partition
property, a sample without an alignment, input forms, determinism, every element written, the LDS bound.

Tolerances are those of test_noblank_posteriors / test_binary_posteriors (tests/test_parity_gpu.py): nll within
1e-5 max(1, |nll|), gamma within 2e-4 of float64."""
import functools

import numpy as np
import pytest
import torch

from oracle import ctc_numpy
from tests.helpers import np_, synth_binary, synth_noblank
from tests.test_token_spans_abi import padded, spans_of_path

pytestmark = pytest.mark.gpu

NOBLANK = [(1, 3, 5, 1), (20, 4, 10, 5), (150, 16, 158, 20),
           (40, 3, 300, 12),                                       # C > 256
           (150, 4, 64, 64),                                       # a full wave
           (90, 2, 40, 70),                                        # K = 2
           (12, 2, 20, 256),                                       # K = 4 (S > T: lengths clamped)
           (88, 2, 16, 130)]                                       # K = 4 with live states on many lanes, 156 KB of LDS
BINARY = [(20, 4, 10, 5), (150, 8, 158, 20), (60, 2, 40, 64), (90, 2, 40, 70)]
CASES = [("noblank", s, 1) for s in NOBLANK] + [("binary", s, 1) for s in BINARY]
PEAKED = ("noblank", (150, 8, 158, 20), 4)                         # logits x 4
FIELDS = ("start", "end", "conf", "frame_conf", "path", "score", "nll")
NLL_RTOL, GAMMA_ATOL = 1e-5, 2e-4


def _id(case):
    return "%s-%s%s" % (case[0], "x".join(str(v) for v in case[1]), "" if case[2] == 1 else "-x%d" % case[2])


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    import ctc_amd  # noqa: F401  (raises if libctc_amd.so is missing)
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def inputs(case):
    """(x, targets, Tb, L) of a case, built once and left unchanged.  Where S > T the generator's lengths are clamped to
    T_b <= T and L_b <= T_b and the labels padded again."""
    family, (T, B, C, S), scale = case
    if family == "noblank":
        x, tg, Tb, L = synth_noblank(sum((T, B, C, S)) + 3, T, B, C, S, var_T=True)
    else:
        x, tg, Tb, L = synth_binary(sum((T, B, C, S)) + 5, T, B, C, S, var_T=True, density=0.2)
    Tb = Tb.clamp(max=T)
    L = torch.minimum(L, Tb)
    pad = torch.arange(S)[None, :] >= L[:, None]
    if family == "noblank":
        tg[pad] = -1
    else:
        tg[pad] = 0.0
    assert bool((L >= 1).all() and (L <= Tb).all() and (Tb <= T).all())
    return x * scale, tg, Tb, L


@functools.lru_cache(maxsize=None)
def oracle(case):
    """float64 (nll [B], gamma [B,T,S]) of a case, computed once"""
    x, tg, Tb, L = inputs(case)
    fn = ctc_numpy.noblank_ctc if case[0] == "noblank" else ctc_numpy.binary_ctc
    ref = fn(np_(x), np_(tg), np_(Tb), np_(L), np.float64)
    return ref["nll"], ref["gamma"].transpose(1, 0, 2)


def _fns(family):
    import ctc_amd
    if family == "noblank":
        return ctc_amd.noblank_token_spans, ctc_amd.noblank_best_path
    return ctc_amd.binary_token_spans, ctc_amd.binary_best_path


def _spans(dev, family, x, tg, Tb, L, xd=None):
    out = _fns(family)[0](x.to(dev) if xd is None else xd, tg.to(dev), Tb.to(dev), L.to(dev))
    torch.cuda.synchronize()
    return out


def _bits(t):
    return t.view(torch.int32) if t.dtype is torch.float32 else t


def _same(a, b, what="", rows=None):
    for name, x, y in zip(FIELDS, a, b):
        if rows is not None:
            x, y = x[rows], y[rows]
        assert torch.equal(_bits(x), _bits(y)), "%s %s" % (what, name)


def _check(dev, case, out):
    """everything the contract says about one call's outputs"""
    family = case[0]
    x, tg, Tb, L = inputs(case)
    T, B, S = x.shape[0], x.shape[1], tg.shape[1]
    assert out.path.dtype is torch.int32 and out.start.dtype is torch.int32 and out.end.dtype is torch.int32
    assert tuple(out.path.shape) == tuple(out.frame_conf.shape) == (B, T)
    assert tuple(out.start.shape) == tuple(out.end.shape) == tuple(out.conf.shape) == (B, S)
    assert tuple(out.score.shape) == tuple(out.nll.shape) == (B,)
    # path and score: the best-path call's, bit for bit
    path, score = _fns(family)[1](x.to(dev), tg.to(dev), Tb.to(dev), L.to(dev))
    torch.cuda.synchronize()
    assert torch.equal(out.path, path), "path"
    assert torch.equal(_bits(out.score), _bits(score)), "score"
    # nll and frame_conf against float64
    rnll, rgamma = oracle(case)
    path, fc, nll = np_(out.path), np_(out.frame_conf), np_(out.nll)
    dn = np.abs(nll - rnll) / np.maximum(1.0, np.abs(rnll))
    ref = np.take_along_axis(rgamma, np.maximum(path, 0)[:, :, None].astype(np.int64), 2)[:, :, 0]
    ref[path < 0] = 0.0
    dfc = np.abs(fc - ref).max()
    print("%s: max rel |dnll| %.3g (bound %.0e), max |dframe_conf| %.3g (bound %.0e)"
          % (_id(case), dn.max(), NLL_RTOL, dfc, GAMMA_ATOL))
    assert (dn <= NLL_RTOL).all()
    assert dfc <= GAMMA_ATOL
    # spans: the restatement on the returned path and confidences, bit for bit
    s, e, c = spans_of_path(path, fc, np_(Tb), np_(L))
    start, end, conf = np_(out.start), np_(out.end), np_(out.conf)
    assert np.array_equal(start, padded(s, S, -1)), "start"
    assert np.array_equal(end, padded(e, S, -1)), "end"
    assert np.array_equal(conf.view(np.int32), padded(c, S, 0).view(np.int32)), "conf"
    # structure
    for b in range(B):
        tb, l = int(Tb[b]), int(L[b])
        assert (path[b, tb:] == -1).all() and (path[b, :tb] >= 0).all()
        assert (fc[b, tb:] == 0).all()
        assert (fc[b, :tb] >= 0).all() and (fc[b, :tb] <= 1.0 + 1e-6).all()
        assert start[b, 0] == 0 and end[b, l - 1] == tb
        assert (end[b, :l - 1] == start[b, 1:l]).all() and (start[b, :l] < end[b, :l]).all()
        for j in range(l):
            assert (path[b, start[b, j]:end[b, j]] == j).all()
        assert (start[b, l:] == -1).all() and (end[b, l:] == -1).all() and (conf[b, l:] == 0).all()


# ---- 1. the contract at every shape ----------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES, ids=_id)
def test_contract(dev, case):
    _check(dev, case, _spans(dev, case[0], *inputs(case)))


def test_peaked_logits(dev):
    """logits x 4: sharper posteriors, longer exponent ranges in the chains; the same tolerances"""
    _check(dev, PEAKED, _spans(dev, PEAKED[0], *inputs(PEAKED)))


# ---- 2. a sample without an alignment among aligned ones ---------------------------------------------------

@pytest.mark.parametrize("case", [("noblank", (20, 4, 10, 5), 1), ("binary", (20, 4, 10, 5), 1)], ids=_id)
def test_sample_without_alignment(dev, case):
    family = case[0]
    x, tg, Tb, L = inputs(case)
    whole = _spans(dev, family, x, tg, Tb, L)
    Tb2, L2 = Tb.clone(), L.clone()
    Tb2[1], L2[1] = 2, 4                                            # (lengths on the device: nothing validates them)
    out = _spans(dev, family, x, tg, Tb2, L2)
    assert bool((out.path[1] == -1).all()) and float(out.score[1]) == -np.inf and float(out.nll[1]) == np.inf
    assert bool((out.frame_conf[1] == 0).all())
    assert bool((out.start[1] == -1).all()) and bool((out.end[1] == -1).all()) and bool((out.conf[1] == 0).all())
    _same(out, whole, "beside a sample without an alignment", rows=[0, 2, 3])
    path, score = _fns(family)[1](x.to(dev), tg.to(dev), Tb2.to(dev), L2.to(dev))
    torch.cuda.synchronize()
    assert torch.equal(out.path, path) and torch.equal(_bits(out.score), _bits(score))


# ---- 3. input forms, determinism ----------------------------------------------------------------------------

def test_label_dtypes(dev):
    case = ("noblank", (150, 16, 158, 20), 1)
    x, tg, Tb, L = inputs(case)
    assert tg.dtype is torch.int32
    _same(_spans(dev, "noblank", x, tg.long(), Tb, L), _spans(dev, "noblank", x, tg, Tb, L), "int64 labels")


@pytest.mark.parametrize("case", [("noblank", (150, 16, 158, 20), 1), ("binary", (150, 8, 158, 20), 1)], ids=_id)
def test_strided_and_deterministic(dev, case):
    """a view x[:, :B] of a batch twice as wide gives the bits of its contiguous copy; lengths on the host too; two calls
    give the same bits"""
    family = case[0]
    x, tg, Tb, L = inputs(case)
    T, B, C = x.shape
    wide = torch.randn(T, 2 * B, C, generator=torch.Generator().manual_seed(23))
    wide[:, :B] = x
    xv = wide.to(dev)[:, :B]
    assert xv.stride(0) == 2 * B * C and not xv.is_contiguous()
    a = _spans(dev, family, x, tg, Tb, L)
    _same(_spans(dev, family, None, tg, Tb, L, xd=xv), a, "strided")
    _same(_spans(dev, family, x, tg, Tb, L), a, "twice")
    host = _fns(family)[0](x.to(dev), tg.to(dev), Tb, L)
    torch.cuda.synchronize()
    _same(host, a, "lengths on the host")


# ---- 4. every element written ---------------------------------------------------------------------------------

@pytest.mark.parametrize("case", [("noblank", (20, 4, 10, 5), 1), ("binary", (20, 4, 10, 5), 1)], ids=_id)
def test_every_element_written(dev, case):
    """one call through the C ABI with all seven outputs pre-filled with poison: none survives"""
    from ctc_amd import _lib
    family = case[0]
    x, tg, Tb, L = inputs(case)
    T, B, C = x.shape
    S = tg.shape[1]
    assert bool((Tb < T).any()) and bool((L < S).any())
    xd, tgd, Tbd, Ld = x.to(dev), tg.to(dev), Tb.to(dev), L.to(dev)
    fl = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float32, device=dev)
    it = lambda *shape: torch.full(shape, 12345, dtype=torch.int32, device=dev)
    path, score, nll, fc, start, end, conf = it(B, T), fl(B), fl(B), fl(B, T), it(B, S), it(B, S), fl(B, S)
    outs = [t.data_ptr() for t in (path, score, nll, fc, start, end, conf)]
    stream = torch.cuda.current_stream().cuda_stream
    lib = _lib.load()
    if family == "noblank":
        rc = lib.ctc_amd_noblank_token_spans(xd.data_ptr(), xd.stride(0), xd.stride(1), tgd.data_ptr(), 0, Tbd.data_ptr(),
                                             Ld.data_ptr(), T, B, C, S, *outs, None, stream)
    else:
        rc = lib.ctc_amd_binary_token_spans(xd.data_ptr(), xd.stride(0), xd.stride(1), tgd.data_ptr(), Tbd.data_ptr(),
                                            Ld.data_ptr(), T, B, C, S, *outs, None, stream)
    assert rc == 0
    torch.cuda.synchronize()
    for name, t in (("score", score), ("nll", nll), ("frame_conf", fc), ("conf", conf)):
        assert not bool(torch.isnan(t).any()), name
    for name, t in (("path", path), ("start", start), ("end", end)):
        assert not bool((t == 12345).any()), name
    from ctc_amd import TokenSpans
    _same(TokenSpans(start, end, conf, fc, path, score, nll), _spans(dev, family, x, tg, Tb, L), "C ABI")


# ---- 5. the LDS bound -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("family", ["noblank", "binary"])
def test_shape_bound(dev, family):
    """600 x 64 cells exceed the LDS even at the best path's own 5 bytes per cell"""
    import ctc_amd
    T, B, C, S = 600, 1, 8, 64
    x = torch.zeros(T, B, C, device=dev)
    tg = torch.zeros(B, S, dtype=torch.int64, device=dev) if family == "noblank" else torch.zeros(B, S, C, device=dev)
    with pytest.raises(ctc_amd.CtcAmdError, match="LDS"):
        _fns(family)[0](x, tg, torch.tensor([T]), torch.tensor([S]))
