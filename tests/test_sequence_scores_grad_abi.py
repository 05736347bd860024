"""The gradient entry of the sequence scores (ctc_amd_sequence_scores_grad and its scratch-bytes function): the C ABI --
declared, exported, bound, every argument error reported with its code before any HIP call (bogus host pointers, no device
needed), a bad argument before an unsupported shape -- and the scratch formula of the header.
tests/test_sequence_scores_grad_gpu.py checks the kernels."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, BAD_ARGUMENT, UNSUPPORTED_SHAPE = 0, -1, -2
P = 4096                                                       # a bogus, 16-byte aligned host address
ENTRY, BYTES = "ctc_amd_sequence_scores_grad", "ctc_amd_sequence_scores_grad_scratch_bytes"
POINTERS = ["x", "in_len", "seq", "seq_len", "w", "grad", "scratch"]    # (count and scores may be NULL)


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
    forward = _declared("ctc_amd_sequence_scores", "int")
    decl = _declared(ENTRY, "int")
    assert len(decl) == 26
    assert decl[:17] == forward[:17]                           # the forward entry's arguments up to N, name by name
    assert decl[17:] == ["const float *w", "int64_t w_stride_b", "float *grad", "int64_t grad_stride_t",
                         "int64_t grad_stride_b", "float *scores", "void *scratch", "size_t scratch_bytes", "void *stream"]
    so = ctypes.CDLL(_lib.SO_PATH)
    assert hasattr(so, ENTRY) and hasattr(so, BYTES)
    r, args = _lib.PROTOTYPES[ENTRY]
    assert r is ctypes.c_int and len(args) == 26 and getattr(lib, ENTRY).argtypes == args
    for d, a in zip(decl, args):                               # pointer / int64_t / int / size_t, argument by argument
        kind = "*" if "*" in d else d.split()[0]
        assert kind in c_of[a], (d, a)
    assert _declared(BYTES, "size_t") == ["int T", "int B", "int C", "int N", "int L", "int blank"]
    r, args = _lib.PROTOTYPES[BYTES]
    assert r is ctypes.c_size_t and args == [ctypes.c_int] * 6
    header = open(os.path.join(ROOT, "include", "ctc_amd.h")).read()
    assert lib.ctc_amd_abi_version() == 2 and _lib.ABI_VERSION == 2 and "#define CTC_AMD_ABI_VERSION 2" in header


def _call(lib, T=10, B=2, C=5, blank=0, N=3, L=4, shared=False, i64=1, count=True, scores=True, scratch_bytes=None,
          scratch_at=P, **null):
    p = {k: (None if null.get(k) else P) for k in POINTERS}
    if p["scratch"] is not None:
        p["scratch"] = scratch_at
    if scratch_bytes is None:
        scratch_bytes = 1 << 40
    return lib.ctc_amd_sequence_scores_grad(p["x"], B * C, C, p["in_len"], T, B, C, blank,
                                            p["seq"], i64, 0 if shared else N * L, L, L, p["seq_len"], 0 if shared else N,
                                            P if count else None, N, p["w"], N, p["grad"], B * C, C,
                                            P if scores else None, p["scratch"], scratch_bytes, None)


@pytest.mark.parametrize("which", POINTERS)
@pytest.mark.parametrize("blank", [0, -1])
def test_null_pointers(lib, which, blank):
    # rejected before anything is dereferenced or launched: the other pointers are non-null but bogus
    assert _call(lib, blank=blank, **{which: True}) == BAD_ARGUMENT
    assert _call(lib, blank=blank, shared=True, count=False, scores=False, **{which: True}) == BAD_ARGUMENT


@pytest.mark.parametrize("kw", [dict(T=0), dict(T=-1), dict(B=0), dict(B=-3), dict(C=0), dict(C=-5), dict(N=0), dict(N=-1),
                                dict(L=0), dict(L=-1)])
@pytest.mark.parametrize("blank", [0, -1])
def test_bad_sizes(lib, kw, blank):
    assert _call(lib, blank=blank, **kw) == BAD_ARGUMENT


def test_blank_beyond_the_classes_and_a_misaligned_scratch(lib):
    assert _call(lib, C=5, blank=5) == BAD_ARGUMENT
    assert _call(lib, C=5, blank=1000) == BAD_ARGUMENT
    assert _call(lib, scratch_at=P + 4) == BAD_ARGUMENT        # the offsets are doubles


@pytest.mark.parametrize("blank", [0, -1])
def test_unsupported_shapes(lib, blank):
    assert _call(lib, blank=blank, L=256) == UNSUPPORTED_SHAPE
    assert _call(lib, blank=blank, L=100000, shared=True) == UNSUPPORTED_SHAPE
    assert _call(lib, blank=blank, C=4097) == UNSUPPORTED_SHAPE                # beyond the staged path
    assert _call(lib, blank=blank, C=100000) == UNSUPPORTED_SHAPE
    need = lib.ctc_amd_sequence_scores_grad_scratch_bytes(10, 2, 5, 3, 4, blank)
    assert need > 0
    assert _call(lib, blank=blank, scratch_bytes=need - 1) == UNSUPPORTED_SHAPE
    assert _call(lib, blank=blank, scratch_bytes=0) == UNSUPPORTED_SHAPE
    # a bad argument is reported before an unsupported shape
    assert _call(lib, blank=blank, L=256, x=True) == BAD_ARGUMENT
    assert _call(lib, blank=blank, C=4097, w=True) == BAD_ARGUMENT
    assert _call(lib, blank=blank, scratch_bytes=0, grad=True) == BAD_ARGUMENT
    assert _call(lib, blank=blank, scratch_bytes=0, T=0) == BAD_ARGUMENT
    assert b"shape" in lib.ctc_amd_error_string(UNSUPPORTED_SHAPE)


def formula(T, B, C, N, L, blank):
    """the header's: B N (8 T (S_L + 1) + 4 (L + 2)) rounded up to a multiple of 256"""
    SL = 2 * L + 1 if blank >= 0 else L
    return (B * N * (8 * T * (SL + 1) + 4 * (L + 2)) + 255) // 256 * 256


def test_scratch_bytes_formula_and_monotony(lib):
    f = lib.ctc_amd_sequence_scores_grad_scratch_bytes
    base = dict(T=30, B=4, C=12, N=4, L=9, blank=0)
    for blank in (0, 3, -1):
        for kw in (base, dict(base, T=2000, B=64, C=1000, L=180), dict(base, T=1, B=1, C=1 if blank < 0 else 4, N=1, L=1),
                   dict(base, C=4096, L=255, N=17)):
            kw = dict(kw, blank=blank)
            assert f(kw["T"], kw["B"], kw["C"], kw["N"], kw["L"], kw["blank"]) == formula(**kw), kw
    assert abs(f(2000, 64, 1000, 4, 180, 0) - 1.48e9) < 0.01e9                 # the size the header names
    for name in ("T", "B", "C", "N", "L"):                      # monotone in each argument (C: constant)
        last = 0
        for v in (1, 2, 3, 7, 8, 9, 64, 200, 255):
            kw = dict(base, **{name: v})
            if name == "C" and v <= base["blank"]:
                continue
            got = f(kw["T"], kw["B"], kw["C"], kw["N"], kw["L"], kw["blank"])
            assert got >= last and got > 0 and got % 256 == 0, (name, v)
            last = got
    assert f(30, 4, 12, 4, 9, 0) >= f(30, 4, 12, 4, 9, -1)      # the blank lattice has the more states
    for bad in (dict(T=0), dict(B=0), dict(C=0), dict(N=0), dict(L=0), dict(L=256), dict(C=4097), dict(blank=12)):
        kw = dict(base, **bad)
        assert f(kw["T"], kw["B"], kw["C"], kw["N"], kw["L"], kw["blank"]) == 0, bad


def test_python_docstrings_state_the_gradient():
    import ctc_amd
    for name in ("blank_sequence_scores", "noblank_sequence_scores"):
        doc = getattr(ctc_amd, name).__doc__
        assert "NO gradient" not in doc and "No gradient" not in doc and "occupancy" in doc
    assert "free inputs" in ctc_amd.blank_sequence_scores.__doc__ and "softmax" in ctc_amd.noblank_sequence_scores.__doc__


def test_python_names_the_class_bound():
    from ctc_amd import functional as F
    assert F.SEQUENCE_SCORES_GRAD_MAX_CLASSES == 4096 and "4096" in F.blank_sequence_scores.__doc__
