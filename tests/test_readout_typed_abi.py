"""The read-outs of the no-blank and the binary lattice on typed logits (ctc_amd_noblank_best_path_typed,
ctc_amd_noblank_posteriors_typed, ctc_amd_noblank_token_spans_typed and the three binary siblings): the C ABI -- declared,
exported, bound, each argument list its untyped sibling's with `x_dtype` behind the x pointer -- and every argument error
reported before any HIP call (bogus host pointers, no device needed).  tests/test_readout_typed_gpu.py checks the kernels."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIBLINGS = {"ctc_amd_%s_%s_typed" % (lat, what): "ctc_amd_%s_%s" % (lat, what)
            for lat in ("noblank", "binary") for what in ("best_path", "posteriors", "token_spans")}
ENTRIES = sorted(SIBLINGS)
OK, BAD_ARGUMENT, UNSUPPORTED_SHAPE = 0, -1, -2
F32, BF16, F16 = 0, 1, 2
P = 4096                                                     # a bogus, 16-byte aligned host address
N_OUT = {"best_path": 2, "posteriors": 2, "token_spans": 7}


@pytest.fixture(scope="module")
def lib():
    from ctc_amd import _lib, build
    build.build()
    return _lib.load()


def _declared(header, name):
    m = re.search(r"\bint %s\s*\(([^;]*)\);" % name, header)
    assert m, "%s is not declared in include/ctc_amd.h" % name
    return [" ".join(a.split()) for a in m.group(1).split(",") if a.strip()]


@pytest.mark.parametrize("name", ENTRIES)
def test_symbols_declared_exported_and_bound(lib, name):
    from ctc_amd import _lib
    header = open(os.path.join(ROOT, "include", "ctc_amd.h")).read()
    typed, plain = _declared(header, name), _declared(header, SIBLINGS[name])
    assert plain[0] == "const float *x"
    assert typed == ["const void *x", "int x_dtype"] + plain[1:]
    assert hasattr(ctypes.CDLL(_lib.SO_PATH), name)
    res, args = _lib.PROTOTYPES[name]
    sib = list(_lib.PROTOTYPES[SIBLINGS[name]][1])
    assert res is ctypes.c_int and args == sib[:1] + [ctypes.c_int] + sib[1:]
    assert getattr(lib, name).argtypes == args


def test_abi_version_is_still_2(lib):
    from ctc_amd import _lib
    header = open(os.path.join(ROOT, "include", "ctc_amd.h")).read()
    assert lib.ctc_amd_abi_version() == 2 and _lib.ABI_VERSION == 2 and "#define CTC_AMD_ABI_VERSION 2" in header
    assert (_lib.F32, _lib.BF16, _lib.F16) == (F32, BF16, F16)


def _pointer_count(name):
    """targets, two lengths, the outputs (x and the workspace apart)"""
    return 3 + next(n for what, n in N_OUT.items() if what in name)


def _call(lib, name, dtype=BF16, x=P, T=10, B=2, C=34, S=4, st=None, sb=None, null=None, untyped=False):
    """one typed entry on bogus host pointers: a call that got past the checks would fault or launch, not return one of the two
    codes.  null: index of the pointer argument (x excluded, in the order of the list) that is NULL; untyped: the same
    arguments without x_dtype through the sibling"""
    sb = C if sb is None else sb
    st = B * sb if st is None else st
    ptrs = [P] * (_pointer_count(name) + 1)                  # targets, two lengths, the outputs, the workspace
    if null is not None:
        ptrs[null] = None
    tgt, il, tl, outs, ws = ptrs[0], ptrs[1], ptrs[2], ptrs[3:-1], ptrs[-1]
    lab = () if "binary" in name else (0,)
    args = [x, dtype, st, sb, tgt, *lab, il, tl, T, B, C, S, *outs, ws, None]
    if untyped:
        del args[1]
        return getattr(lib, SIBLINGS[name])(*args)
    return getattr(lib, name)(*args)


@pytest.mark.parametrize("dtype", [3, -1, 7, 1 << 20])
@pytest.mark.parametrize("name", ENTRIES)
def test_unknown_x_dtype(lib, name, dtype):
    assert _call(lib, name, dtype) == BAD_ARGUMENT
    assert _call(lib, name, dtype, S=300) == BAD_ARGUMENT                        # the bad argument wins over the shape
    assert _call(lib, name, dtype, C=33, x=P + 2) == BAD_ARGUMENT


@pytest.mark.parametrize("dtype", [F32, BF16, F16])
@pytest.mark.parametrize("name", ENTRIES)
def test_null_pointers_and_empty_shapes(lib, name, dtype):
    assert _call(lib, name, dtype, x=None) == BAD_ARGUMENT
    for i in range(_pointer_count(name)):
        assert _call(lib, name, dtype, null=i) == BAD_ARGUMENT, i
    if "posteriors" in name:                                                     # the only ones that use their workspace
        assert _call(lib, name, dtype, null=_pointer_count(name)) == BAD_ARGUMENT
    for kw in (dict(T=0), dict(B=0), dict(C=0), dict(S=0), dict(T=-1), dict(S=-3)):
        assert _call(lib, name, dtype, **kw) == BAD_ARGUMENT, kw


@pytest.mark.parametrize("dtype", [F32, BF16, F16])
@pytest.mark.parametrize("name", ENTRIES)
def test_more_than_256_labels(lib, name, dtype):
    assert _call(lib, name, dtype, S=257) == UNSUPPORTED_SHAPE
    assert _call(lib, name, dtype, S=1000) == UNSUPPORTED_SHAPE


@pytest.mark.parametrize("dtype", [BF16, F16])
def test_noblank_posteriors_two_byte_domain(lib, dtype):
    """2-byte rows: the four-rows-per-wave kernel or nothing -- C even, S <= 31, T <= 168, even strides, a 4-byte aligned base"""
    name = "ctc_amd_noblank_posteriors_typed"
    for bad in (dict(C=33), dict(S=32), dict(T=169), dict(sb=35), dict(st=2 * 34 + 1), dict(x=P + 2), dict(x=P + 6),
                dict(C=258)):
        assert _call(lib, name, dtype, **bad) == UNSUPPORTED_SHAPE, bad
    # a bad argument still wins over a shape outside the domain
    assert _call(lib, name, dtype, C=33, null=0) == BAD_ARGUMENT
    assert _call(lib, name, dtype, x=P + 2, null=3) == BAD_ARGUMENT


@pytest.mark.parametrize("name", ENTRIES)
def test_f32_is_the_untyped_entry(lib, name):
    """the same answers as the sibling for the same (bogus) arguments, bad and unsupported"""
    for kw in (dict(x=None), dict(null=0), dict(null=1), dict(null=3), dict(T=0), dict(S=0), dict(S=257)):
        got = _call(lib, name, F32, **kw)
        assert got == _call(lib, name, F32, untyped=True, **kw) and got in (BAD_ARGUMENT, UNSUPPORTED_SHAPE), kw


def test_no_cpu_path_for_two_byte_logits():
    import torch
    import ctc_amd
    z = torch.zeros
    for dt in (torch.bfloat16, torch.float16):
        with pytest.raises(ctc_amd.CtcAmdError):
            ctc_amd.noblank_best_path(z(4, 2, 6, dtype=dt), z(2, 3, dtype=torch.int32), [4, 4], [3, 3])
