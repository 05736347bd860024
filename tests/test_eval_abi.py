"""The evaluation entries (ctc_amd_collapse_frames, ctc_amd_edit_distance): the C ABI -- declared, exported, bound, every
argument error reported before any HIP call (bogus host pointers, no device needed) -- and the Python surface's own
refusals.  tests/test_eval_gpu.py checks the kernels."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, BAD_ARGUMENT, UNSUPPORTED_SHAPE = 0, -1, -2
P = 4096                                                       # a bogus, 16-byte aligned host address
COLLAPSE, EDIT = "ctc_amd_collapse_frames", "ctc_amd_edit_distance"
COLLAPSE_POINTERS = ["frames", "in_len", "tokens", "out_len", "start", "end"]      # frame_conf / conf: both or neither
EDIT_POINTERS = ["hyp", "hyp_len", "ref", "ref_len", "dist"]


@pytest.fixture(scope="module")
def lib():
    from ctc_amd import _lib, build
    build.build()
    return _lib.load()


def _declared(name):
    header = open(os.path.join(ROOT, "include", "ctc_amd.h")).read()
    m = re.search(r"\bint %s\s*\(([^;]*)\);" % name, header)
    assert m, "%s is not declared in include/ctc_amd.h" % name
    return [" ".join(a.split()) for a in m.group(1).split(",") if a.strip()]


def test_symbols_declared_exported_and_bound(lib):
    from ctc_amd import _lib
    c_of = {ctypes.c_void_p: ("*",), ctypes.c_int64: ("int64_t",), ctypes.c_int: ("int",)}
    for name, nargs in ((COLLAPSE, 18), (EDIT, 13)):
        decl = _declared(name)
        assert len(decl) == nargs
        assert hasattr(ctypes.CDLL(_lib.SO_PATH), name)
        res, args = _lib.PROTOTYPES[name]
        assert res is ctypes.c_int and len(args) == nargs and getattr(lib, name).argtypes == args
        for d, a in zip(decl, args):                           # pointer / int64_t / int, argument by argument
            kind = "*" if "*" in d else d.split()[0]
            assert kind in c_of[a], (name, d, a)
    assert _declared(COLLAPSE)[-1] == "void *stream" and _declared(EDIT)[-1] == "void *stream"
    header = open(os.path.join(ROOT, "include", "ctc_amd.h")).read()
    assert lib.ctc_amd_abi_version() == 2 and _lib.ABI_VERSION == 2 and "#define CTC_AMD_ABI_VERSION 2" in header


def _collapse(lib, T=10, B=2, blank=0, W=10, frame_conf=None, conf=None, i64=0, **null):
    p = {k: (None if null.get(k) else P) for k in COLLAPSE_POINTERS}
    return lib.ctc_amd_collapse_frames(p["frames"], i64, T, 1, p["in_len"], frame_conf, T, 1, T, B, blank, W,
                                       p["tokens"], p["out_len"], p["start"], p["end"], conf, None)


def _edit(lib, B=2, N=5, M=4, **null):
    p = {k: (None if null.get(k) else P) for k in EDIT_POINTERS}
    return lib.ctc_amd_edit_distance(p["hyp"], 0, N, p["hyp_len"], p["ref"], 1, M, p["ref_len"], B, N, M, p["dist"], None)


@pytest.mark.parametrize("which", COLLAPSE_POINTERS)
@pytest.mark.parametrize("with_conf", [False, True])
def test_collapse_null_pointers(lib, which, with_conf):
    # rejected before anything is dereferenced or launched: the other pointers are non-null but bogus
    kw = dict(frame_conf=P, conf=P) if with_conf else {}
    assert _collapse(lib, **{which: True}, **kw) == BAD_ARGUMENT


def test_collapse_confidence_in_and_out_go_together(lib):
    assert _collapse(lib, frame_conf=P) == BAD_ARGUMENT
    assert _collapse(lib, conf=P) == BAD_ARGUMENT


@pytest.mark.parametrize("kw", [dict(T=0), dict(T=-1), dict(B=0), dict(B=-4), dict(W=0), dict(W=-1)])
@pytest.mark.parametrize("blank", [0, -1, 5])
def test_collapse_bad_sizes(lib, kw, blank):
    assert _collapse(lib, blank=blank, **kw) == BAD_ARGUMENT
    assert _collapse(lib, blank=blank, frame_conf=P, conf=P, i64=1, **kw) == BAD_ARGUMENT


def test_collapse_beyond_lds(lib):
    """4 (T + 2 min(W, T) + 1) bytes within 160 KB (include/ctc_amd.h): refused before any launch beyond"""
    assert _collapse(lib, T=13654, W=13654) == UNSUPPORTED_SHAPE
    assert _collapse(lib, T=40958, W=1) == UNSUPPORTED_SHAPE
    assert _collapse(lib, T=1 << 20, W=1 << 20) == UNSUPPORTED_SHAPE
    assert _collapse(lib, T=1 << 20, W=1 << 20, frames=True) == BAD_ARGUMENT          # a bad argument wins over the shape


@pytest.mark.parametrize("which", EDIT_POINTERS)
def test_edit_null_pointers(lib, which):
    assert _edit(lib, **{which: True}) == BAD_ARGUMENT


@pytest.mark.parametrize("kw", [dict(B=0), dict(B=-1), dict(N=-1), dict(M=-1), dict(N=-5, M=-5)])
def test_edit_bad_sizes(lib, kw):
    assert _edit(lib, **kw) == BAD_ARGUMENT


def test_edit_reference_width_limit(lib):
    assert _edit(lib, M=1024) == UNSUPPORTED_SHAPE
    assert _edit(lib, M=5000, N=0) == UNSUPPORTED_SHAPE
    assert _edit(lib, M=1024, dist=True) == BAD_ARGUMENT         # a bad argument wins over the shape
    assert _edit(lib, M=1024, N=-1) == BAD_ARGUMENT


def test_python_export():
    import ctc_amd
    for name in ("collapse_frames", "edit_distance", "label_error_rate", "CollapsedTokens"):
        assert name in ctc_amd.__all__ and hasattr(ctc_amd, name)
    assert ctc_amd.CollapsedTokens._fields == ("tokens", "lengths", "start", "end", "conf")


def test_python_refusals_on_cpu_tensors():
    """wrong device, rank or dtype: ValueError before the library is asked"""
    import torch
    import ctc_amd
    z = torch.zeros
    with pytest.raises(ValueError):
        ctc_amd.collapse_frames(z(2, 5, dtype=torch.int64), [5, 5])                   # a CPU tensor
    with pytest.raises(ValueError):
        ctc_amd.collapse_frames(z(5, dtype=torch.int64), [5])                         # rank
    with pytest.raises(ValueError):
        ctc_amd.collapse_frames(z(2, 5), [5, 5], blank=0)                             # float frames
    with pytest.raises(ValueError):
        ctc_amd.collapse_frames([[1, 2, 3]], [3])                                     # not a tensor
    with pytest.raises(ValueError):
        ctc_amd.edit_distance(z(2, 5, dtype=torch.int32), [5, 5], z(2, 4, dtype=torch.int64), [4, 4])
    with pytest.raises(ValueError):
        ctc_amd.edit_distance(z(2, 5, dtype=torch.int16), [5, 5], z(2, 4, dtype=torch.int64), [4, 4])
    with pytest.raises(ValueError):
        ctc_amd.edit_distance(z(2, 5, 1, dtype=torch.int64), [5, 5], z(2, 4, dtype=torch.int64), [4, 4])
    with pytest.raises(ValueError):
        ctc_amd.label_error_rate(z(2, 5, dtype=torch.int64), [5, 5], z(2, 4, dtype=torch.int64), [4, 4])
