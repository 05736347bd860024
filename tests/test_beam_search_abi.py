"""The beam search entries (ctc_amd_beam_search, ctc_amd_beam_search_scratch_bytes): the C ABI -- declared, exported, bound,
every argument error reported before any HIP call (bogus host pointers, no device needed) -- and the Python surface's own
refusals.  tests/test_beam_search_gpu.py checks the kernel."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, BAD_ARGUMENT = 0, -1
P = 4096                                                       # a bogus, 16-byte aligned host address
SEARCH, SCRATCH = "ctc_amd_beam_search", "ctc_amd_beam_search_scratch_bytes"
POINTERS = ["x", "in_len", "tokens", "lengths", "scores", "count", "scratch"]


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


def test_symbols_declared_exported_and_bound(lib):
    from ctc_amd import _lib
    c_of = {ctypes.c_void_p: ("*",), ctypes.c_int64: ("int64_t",), ctypes.c_int: ("int",), ctypes.c_size_t: ("size_t",)}
    for name, res, cres, nargs in ((SEARCH, "int", ctypes.c_int, 19), (SCRATCH, "size_t", ctypes.c_size_t, 3)):
        decl = _declared(name, res)
        assert len(decl) == nargs
        assert hasattr(ctypes.CDLL(_lib.SO_PATH), name)
        r, args = _lib.PROTOTYPES[name]
        assert r is cres and len(args) == nargs and getattr(lib, name).argtypes == args
        for d, a in zip(decl, args):                           # pointer / int64_t / size_t / int, argument by argument
            kind = "*" if "*" in d else d.split()[0]
            assert kind in c_of[a], (name, d, a)
    assert _declared(SEARCH, "int")[-1] == "void *stream"
    header = open(os.path.join(ROOT, "include", "ctc_amd.h")).read()
    assert lib.ctc_amd_abi_version() == 2 and _lib.ABI_VERSION == 2 and "#define CTC_AMD_ABI_VERSION 2" in header


def _search(lib, T=10, B=2, C=5, blank=0, W=4, K=3, N=2, L=10, scratch_bytes=None, **null):
    p = {k: (None if null.get(k) else P) for k in POINTERS}
    if scratch_bytes is None:
        scratch_bytes = 1 << 40                                 # (nothing is touched before the checks are through)
    return lib.ctc_amd_beam_search(p["x"], B * C, C, p["in_len"], T, B, C, blank, W, K, N, L, p["tokens"], p["lengths"],
                                   p["scores"], p["count"], p["scratch"], scratch_bytes, None)


def test_scratch_bytes(lib):
    assert lib.ctc_amd_beam_search_scratch_bytes(10, 2, 4) == 2 * (10 * 4 + 1) * 8
    assert lib.ctc_amd_beam_search_scratch_bytes(2000, 64, 16) == 64 * (2000 * 16 + 1) * 8
    assert lib.ctc_amd_beam_search_scratch_bytes(1, 1, 1) == 16
    for T, B, W in ((0, 2, 4), (10, 0, 4), (10, 2, 0), (10, 2, 65), (-1, -1, -1), (1 << 30, 1, 64)):
        assert lib.ctc_amd_beam_search_scratch_bytes(T, B, W) == 0


@pytest.mark.parametrize("which", POINTERS)
@pytest.mark.parametrize("blank", [0, -1])
def test_null_pointers(lib, which, blank):
    # rejected before anything is dereferenced or launched: the other pointers are non-null but bogus
    assert _search(lib, blank=blank, **{which: True}) == BAD_ARGUMENT


@pytest.mark.parametrize("kw", [dict(T=0), dict(T=-1), dict(B=0), dict(B=-3), dict(C=1), dict(C=0), dict(C=-5),
                                dict(W=0), dict(W=65), dict(W=-1), dict(K=0), dict(K=33), dict(K=-2),
                                dict(N=0), dict(N=5), dict(N=-1), dict(W=64, N=65), dict(L=0), dict(L=-1),
                                dict(T=1 << 30, W=64)])
@pytest.mark.parametrize("blank", [0, -1])
def test_bad_sizes(lib, kw, blank):
    assert _search(lib, blank=blank, **kw) == BAD_ARGUMENT


def test_blank_beyond_the_classes(lib):
    assert _search(lib, C=5, blank=5) == BAD_ARGUMENT
    assert _search(lib, C=5, blank=1000) == BAD_ARGUMENT


def test_scratch_too_small(lib):
    need = lib.ctc_amd_beam_search_scratch_bytes(10, 2, 4)
    assert _search(lib, scratch_bytes=need - 1) == BAD_ARGUMENT
    assert _search(lib, scratch_bytes=0) == BAD_ARGUMENT
    assert _search(lib, W=8, N=8, scratch_bytes=need) == BAD_ARGUMENT        # sized for another beam width


def test_python_export():
    import ctc_amd
    for name in ("blank_beam_search", "noblank_beam_search", "BeamHypotheses"):
        assert name in ctc_amd.__all__ and hasattr(ctc_amd, name)
    assert ctc_amd.BeamHypotheses._fields == ("tokens", "lengths", "scores", "count")


def test_python_refusals_before_any_launch():
    """limits, rank, dtype and device: ValueError before the library is asked (CPU tensors never reach it)"""
    import torch
    import ctc_amd
    x = torch.zeros(6, 2, 5)
    for fn in (ctc_amd.blank_beam_search, ctc_amd.noblank_beam_search):
        for kw in (dict(beam_width=65), dict(beam_width=0), dict(nbest=0), dict(nbest=17), dict(beam_width=4, nbest=5),
                   dict(top_classes=0), dict(top_classes=33), dict(max_tokens=0), dict(max_tokens=-3)):
            with pytest.raises(ValueError):
                fn(x, [6, 6], **kw)
        with pytest.raises(ValueError):
            fn(x, [6, 6])                                                               # a CPU tensor
        with pytest.raises(ValueError):
            fn(x[0], [6])                                                               # rank
        with pytest.raises(ValueError):
            fn([[[0.0, 1.0]]], [1])                                                     # not a tensor
        for dtype in (torch.bfloat16, torch.float16, torch.float64):
            with pytest.raises(ValueError):
                fn(x.to(dtype), [6, 6])
        with pytest.raises(ValueError):
            fn(torch.zeros(6, 2, 1), [6, 6])                                            # C < 2
    for blank in (-1, 5, 99):
        with pytest.raises(ValueError):
            ctc_amd.blank_beam_search(x, [6, 6], blank=blank)
