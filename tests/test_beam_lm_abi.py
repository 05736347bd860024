"""The fused beam search entry (ctc_amd_beam_search_lm): the C ABI -- declared, exported, bound, every argument error reported
before any HIP call (bogus host pointers, no device needed) -- and the Python surface's own refusals.
tests/test_beam_lm_gpu.py checks the kernel."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, BAD_ARGUMENT = 0, -1
P = 4096                                                       # a bogus, 16-byte aligned host address
NAME = "ctc_amd_beam_search_lm"
POINTERS = ["x", "in_len", "lm", "tokens", "lengths", "scores", "ctc_scores", "count", "scratch"]
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def lib():
    from ctc_amd import _lib, build
    build.build()
    return _lib.load()


def _declared(name, res):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ctc_amd.h")).read(), flags=re.S)
    m = re.search(r"\b%s %s\s*\(([^;]*)\);" % (res, name), header)
    assert m, "%s is not declared in include/ctc_amd.h" % name
    return [" ".join(a.split()) for a in m.group(1).split(",") if a.strip()]


def test_symbol_declared_exported_and_bound(lib):
    from ctc_amd import _lib
    c_of = {ctypes.c_void_p: "*", ctypes.c_int64: "int64_t", ctypes.c_int: "int", ctypes.c_size_t: "size_t",
            ctypes.c_float: "float"}
    decl = _declared(NAME, "int")
    assert len(decl) == 24
    assert hasattr(ctypes.CDLL(_lib.SO_PATH), NAME)
    r, args = _lib.PROTOTYPES[NAME]
    assert r is ctypes.c_int and len(args) == 24 and getattr(lib, NAME).argtypes == args
    for d, a in zip(decl, args):                               # pointer / int64_t / size_t / int / float, one by one
        kind = "*" if "*" in d else d.split()[0]
        assert kind == c_of[a], (d, a)
    # the plain entry's list with (lm, lm_stride, lm_weight, token_bonus) behind L and ctc_scores behind scores
    plain = _declared("ctc_amd_beam_search", "int")
    assert decl[:12] == plain[:12] and decl[12:16] == ["const float *lm", "int64_t lm_stride", "float lm_weight",
                                                       "float token_bonus"]
    assert decl[16:19] == plain[12:15] and decl[19] == "float *ctc_scores" and decl[20:] == plain[15:]
    header = open(os.path.join(ROOT, "include", "ctc_amd.h")).read()
    assert lib.ctc_amd_abi_version() == 2 and _lib.ABI_VERSION == 2 and "#define CTC_AMD_ABI_VERSION 2" in header


def _search(lib, T=10, B=2, C=5, blank=0, W=4, K=3, N=2, L=10, lm_stride=None, alpha=0.8, beta=0.5, scratch_bytes=None,
            **null):
    p = {k: (None if null.get(k) else P) for k in POINTERS}
    if scratch_bytes is None:
        scratch_bytes = 1 << 40                                 # (nothing is touched before the checks are through)
    return lib.ctc_amd_beam_search_lm(p["x"], B * C, C, p["in_len"], T, B, C, blank, W, K, N, L,
                                      p["lm"], C if lm_stride is None else lm_stride, alpha, beta,
                                      p["tokens"], p["lengths"], p["scores"], p["ctc_scores"], p["count"],
                                      p["scratch"], scratch_bytes, None)


@pytest.mark.parametrize("which", POINTERS)
@pytest.mark.parametrize("blank", [0, -1])
def test_null_pointers(lib, which, blank):
    assert _search(lib, blank=blank, **{which: True}) == BAD_ARGUMENT


@pytest.mark.parametrize("kw", [dict(lm_stride=4), dict(lm_stride=0), dict(lm_stride=-5),
                                dict(alpha=NAN), dict(alpha=INF), dict(alpha=-1.0), dict(alpha=-INF),
                                dict(beta=NAN), dict(beta=INF), dict(beta=-INF)])
@pytest.mark.parametrize("blank", [0, -1])
def test_bad_table_arguments(lib, kw, blank):
    assert _search(lib, blank=blank, **kw) == BAD_ARGUMENT


@pytest.mark.parametrize("kw", [dict(T=0), dict(T=-1), dict(B=0), dict(B=-3), dict(C=1), dict(C=0), dict(C=-5),
                                dict(W=0), dict(W=65), dict(W=-1), dict(K=0), dict(K=33), dict(K=-2),
                                dict(N=0), dict(N=5), dict(N=-1), dict(W=64, N=65), dict(L=0), dict(L=-1),
                                dict(T=1 << 30, W=64)])
@pytest.mark.parametrize("blank", [0, -1])
def test_bad_sizes_of_the_plain_entry(lib, kw, blank):
    assert _search(lib, blank=blank, **kw) == BAD_ARGUMENT


def test_blank_beyond_the_classes_and_scratch_too_small(lib):
    assert _search(lib, C=5, blank=5) == BAD_ARGUMENT
    need = lib.ctc_amd_beam_search_scratch_bytes(10, 2, 4)
    assert _search(lib, scratch_bytes=need - 1) == BAD_ARGUMENT
    assert _search(lib, scratch_bytes=0) == BAD_ARGUMENT
    assert _search(lib, W=8, N=8, scratch_bytes=need) == BAD_ARGUMENT        # sized for another beam width


def test_python_export():
    import ctc_amd
    assert "FusedBeamHypotheses" in ctc_amd.__all__ and hasattr(ctc_amd, "FusedBeamHypotheses")
    assert ctc_amd.FusedBeamHypotheses._fields == ("tokens", "lengths", "scores", "count", "ctc_scores")
    assert ctc_amd.BeamHypotheses._fields == ("tokens", "lengths", "scores", "count")


def test_python_refusals_before_any_launch():
    """CPU tensors never reach the library: every call is a ValueError, with or without a table"""
    import torch
    import ctc_amd
    x = torch.zeros(6, 2, 5)
    good = torch.zeros(6, 5)
    for fn in (ctc_amd.blank_beam_search, ctc_amd.noblank_beam_search):
        for kw in (dict(lm=good), dict(lm=good, lm_weight=0.5, token_bonus=1.0), dict(lm_weight=0.5), dict(token_bonus=1.0),
                   dict(lm=torch.zeros(5, 5)), dict(lm=good.double()), dict(lm=[[0.0]]), dict(lm=good, lm_weight=-1.0),
                   dict(lm=good, token_bonus=NAN), dict(lm=good, beam_width=65), dict(lm=good, max_tokens=0)):
            with pytest.raises(ValueError):
                fn(x, [6, 6], **kw)
    # an existing refusal still comes first: the table is not looked at before the logits are accepted
    with pytest.raises(ValueError, match="beam search needs 1 <= nbest"):
        ctc_amd.blank_beam_search(x, [6, 6], beam_width=65, lm="no table")
    with pytest.raises(ValueError, match="HIP"):
        ctc_amd.noblank_beam_search(x, [6, 6], lm="no table", lm_weight=NAN)


def test_python_table_rules():
    """the table as the library is given it: shape [C+1, C], float32, the logits' device; a view with unit column stride and
    a row stride >= C is passed as it lies, any other is made contiguous"""
    import torch
    from ctc_amd import functional as F
    cpu = torch.device("cpu")
    C = 5
    good = torch.randn(C + 1, C)
    assert F._beam_lm_table(good, C, cpu).data_ptr() == good.data_ptr()
    for bad, what in ((torch.zeros(C, C), "C\\+1"), (torch.zeros(C + 1, C + 1), "C\\+1"), (torch.zeros(C + 1), "C\\+1"),
                      (good.double(), "float32"), (good.half(), "float32"), (good.numpy(), "float32"), (None, "float32")):
        with pytest.raises(ValueError, match=what):
            F._beam_lm_table(bad, C, cpu)
    with pytest.raises(ValueError, match="device"):
        F._beam_lm_table(good, C, torch.device("cuda:0"))
    big = torch.randn(C + 1, C + 7)
    view = F._beam_lm_table(big[:, :C], C, cpu)
    assert view.data_ptr() == big.data_ptr() and view.stride() == (C + 7, 1)
    for other in (big.t()[:C + 1, :C], big[:, ::2][:, :C], good.unsqueeze(0).expand(3, C + 1, C)[1], good[:1].expand(C + 1, C)):
        made = F._beam_lm_table(other, C, cpu)
        assert made.stride() == (C, 1) and torch.equal(made, other)
