"""The sequence-scores entry (ctc_amd_sequence_scores): the C ABI -- declared, exported, bound, every argument error reported
before any HIP call (bogus host pointers, no device needed) -- and the Python surface's own refusals.
tests/test_sequence_scores_gpu.py checks the kernel."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, BAD_ARGUMENT, UNSUPPORTED_SHAPE = 0, -1, -2
P = 4096                                                       # a bogus, 16-byte aligned host address
ENTRY = "ctc_amd_sequence_scores"
POINTERS = ["x", "in_len", "seq", "seq_len", "scores"]          # (count may be NULL)


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
    c_of = {ctypes.c_void_p: ("*",), ctypes.c_int64: ("int64_t",), ctypes.c_int: ("int",)}
    decl = _declared(ENTRY, "int")
    assert len(decl) == 19
    assert hasattr(ctypes.CDLL(_lib.SO_PATH), ENTRY)
    r, args = _lib.PROTOTYPES[ENTRY]
    assert r is ctypes.c_int and len(args) == 19 and getattr(lib, ENTRY).argtypes == args
    for d, a in zip(decl, args):                               # pointer / int64_t / int, argument by argument
        kind = "*" if "*" in d else d.split()[0]
        assert kind in c_of[a], (d, a)
    assert decl[-1] == "void *stream"
    header = open(os.path.join(ROOT, "include", "ctc_amd.h")).read()
    assert lib.ctc_amd_abi_version() == 2 and _lib.ABI_VERSION == 2 and "#define CTC_AMD_ABI_VERSION 2" in header


def _call(lib, T=10, B=2, C=5, blank=0, N=3, L=4, shared=False, i64=1, count=True, **null):
    p = {k: (None if null.get(k) else P) for k in POINTERS}
    return lib.ctc_amd_sequence_scores(p["x"], B * C, C, p["in_len"], T, B, C, blank,
                                       p["seq"], i64, 0 if shared else N * L, L, L, p["seq_len"], 0 if shared else N,
                                       P if count else None, N, p["scores"], None)


@pytest.mark.parametrize("which", POINTERS)
@pytest.mark.parametrize("blank", [0, -1])
def test_null_pointers(lib, which, blank):
    # rejected before anything is dereferenced or launched: the other pointers are non-null but bogus
    assert _call(lib, blank=blank, **{which: True}) == BAD_ARGUMENT
    assert _call(lib, blank=blank, shared=True, count=False, **{which: True}) == BAD_ARGUMENT


@pytest.mark.parametrize("kw", [dict(T=0), dict(T=-1), dict(B=0), dict(B=-3), dict(C=0), dict(C=-5), dict(N=0), dict(N=-1),
                                dict(L=0), dict(L=-1)])
@pytest.mark.parametrize("blank", [0, -1])
def test_bad_sizes(lib, kw, blank):
    assert _call(lib, blank=blank, **kw) == BAD_ARGUMENT


def test_blank_beyond_the_classes(lib):
    assert _call(lib, C=5, blank=5) == BAD_ARGUMENT
    assert _call(lib, C=5, blank=1000) == BAD_ARGUMENT


@pytest.mark.parametrize("blank", [0, -1])
def test_more_than_255_labels(lib, blank):
    assert _call(lib, blank=blank, L=256) == UNSUPPORTED_SHAPE
    assert _call(lib, blank=blank, L=100000, shared=True) == UNSUPPORTED_SHAPE
    assert _call(lib, blank=blank, L=256, x=True) == BAD_ARGUMENT          # (a NULL pointer is reported first)
    assert b"shape" in lib.ctc_amd_error_string(UNSUPPORTED_SHAPE)


def test_python_export():
    import ctc_amd
    for name in ("blank_sequence_scores", "noblank_sequence_scores"):
        assert name in ctc_amd.__all__ and hasattr(ctc_amd, name)
        assert "gradient" in getattr(ctc_amd, name).__doc__


def test_python_refusals_before_any_launch():
    """rank, dtype, shapes, the label limit and the device: refused before the library is asked (CPU tensors never reach it)"""
    import torch
    import ctc_amd
    x = torch.zeros(6, 2, 5)
    seq, sl = torch.zeros(2, 3, 4, dtype=torch.int64), torch.ones(2, 3, dtype=torch.int64)
    for fn in (ctc_amd.blank_sequence_scores, ctc_amd.noblank_sequence_scores):
        with pytest.raises(ValueError):
            fn(x, [6, 6], seq, sl)                                                      # a CPU tensor
        with pytest.raises(ValueError):
            fn(x[0], [6], seq, sl)                                                      # rank
        with pytest.raises(ValueError):
            fn([[[0.0, 1.0]]], [1], seq, sl)                                            # not a tensor
        for dtype in (torch.bfloat16, torch.float16, torch.float64):                    # no 2-byte dtype here
            with pytest.raises(ValueError):
                fn(x.to(dtype), [6, 6], seq, sl)
        for bad in (seq.float(), seq.to(torch.int16), seq[0, 0], seq[:1], seq[:, :0], seq[:, :, :0], [[1, 2]]):
            with pytest.raises(ValueError):
                fn(x, [6, 6], bad, sl)
        for bad in (sl[0], sl[:, :2], sl.float(), torch.ones(3, 2, dtype=torch.int64)):
            with pytest.raises(ValueError):
                fn(x, [6, 6], seq, bad)
        with pytest.raises(ValueError):
            fn(x, [6, 6], seq[0], sl)                                                   # shared sequences, per-sample lengths
        for bad in (torch.ones(3, dtype=torch.int32), torch.ones(2), torch.ones(2, dtype=torch.int64),
                    torch.ones(2, 1, dtype=torch.int32), [1, 1]):
            with pytest.raises(ValueError):
                fn(x, [6, 6], seq, sl, counts=bad)
        with pytest.raises(ctc_amd.CtcAmdError, match="255"):                           # the limit, named
            fn(x, [6, 6], torch.zeros(2, 3, 256, dtype=torch.int64), sl)
        with pytest.raises(ctc_amd.CtcAmdError, match="255"):
            fn(x, [6, 6], torch.zeros(3, 256, dtype=torch.int32), sl[0])
    for blank in (-1, 5, 99):
        with pytest.raises(ValueError):
            ctc_amd.blank_sequence_scores(x, [6, 6], seq, sl, blank=blank)
