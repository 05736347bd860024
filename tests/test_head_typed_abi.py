"""The head entries on a bf16 / fp16 feature operand (ctc_amd_head_forward_typed, ctc_amd_head_forward_wide_typed,
ctc_amd_lstm_forward_typed, ctc_amd_head_backward_typed, ctc_amd_head_backward_wide_typed): the C ABI -- declared, exported, bound,
each argument list its untyped sibling's with `feat_dtype` behind the feat pointer -- and every argument error reported before any
HIP call (bogus host pointers, no device needed).  tests/test_head_typed_gpu.py checks the kernels."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIBLINGS = {"ctc_amd_head_forward_typed": "ctc_amd_head_forward",
            "ctc_amd_head_forward_wide_typed": "ctc_amd_head_forward_wide",
            "ctc_amd_lstm_forward_typed": "ctc_amd_lstm_forward",
            "ctc_amd_head_backward_typed": "ctc_amd_head_backward",
            "ctc_amd_head_backward_wide_typed": "ctc_amd_head_backward_wide"}
ENTRIES = sorted(SIBLINGS)
OK, BAD_ARGUMENT, UNSUPPORTED_SHAPE = 0, -1, -2
F32, BF16, F16 = 0, 1, 2
P = 4096                                                     # a bogus, 16-byte aligned host address


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
    # the sibling's list with feat -> (const void *feat, int feat_dtype) and, on the backward entries, d_feat -> void *d_feat
    want = []
    for a in plain:
        if a == "const float *feat":
            want += ["const void *feat", "int feat_dtype"]
        elif a == "float *d_feat":
            want.append("void *d_feat")
        else:
            want.append(a)
    assert typed == want and len(typed) == len(plain) + 1
    assert ("void *d_feat" in typed) == ("backward" in name)
    assert hasattr(ctypes.CDLL(_lib.SO_PATH), name)
    res, args = _lib.PROTOTYPES[name]
    sib = list(_lib.PROTOTYPES[SIBLINGS[name]][1])
    i = plain.index("const float *feat")
    assert res is ctypes.c_int and args == sib[:i + 1] + [ctypes.c_int] + sib[i + 1:]
    assert getattr(lib, name).argtypes == args


def test_abi_version_is_still_2(lib):
    from ctc_amd import _lib
    header = open(os.path.join(ROOT, "include", "ctc_amd.h")).read()
    assert lib.ctc_amd_abi_version() == 2 and _lib.ABI_VERSION == 2 and "#define CTC_AMD_ABI_VERSION 2" in header
    assert (_lib.F32, _lib.BF16, _lib.F16) == (F32, BF16, F16)
    for k, v in (("F32 ", F32), ("BF16", BF16), ("F16 ", F16)):
        assert "#define CTC_AMD_%s %d" % (k, v) in header


def _call(lib, name, dtype=BF16, feat=P, T=2, B=10, K=32, C=8, fsb=None, fst=None, out=P, d_feat=P, dfeat_sb=None, eval_mode=False,
          untyped=False):
    """one typed entry on bogus host pointers: a call that got past the checks would fault, not return.  untyped: the same
    arguments without feat_dtype through the sibling"""
    wide = "wide" in name
    if wide and B <= 256:
        B = 300
    fsb = K if fsb is None else fsb
    fst = B * fsb if fst is None else fst
    rm = P if eval_mode else None
    if name == "ctc_amd_lstm_forward_typed":
        args = [feat, dtype, fst, fsb, P, P, P, P, P, P, 1e-5, P, P, P, P, P, P, T, B, K, C, out, B * C, C, C, 0.0, None, None, None]
    elif "forward" in name:
        tail = (P, 1 << 30, None) if wide else (None,)
        stats = (None,) * 3 if eval_mode else (P,) * 3
        args = [feat, dtype, fst, fsb, P, P, P, P, rm, rm, 1e-5, None, T, B, K, C, out, B * C, C, P, *stats, *tail]
    else:
        sv = None if eval_mode else P
        dfeat_sb = K if dfeat_sb is None else dfeat_sb
        args = [P, B * C, C, feat, dtype, fst, fsb, P, P, P, P, sv, sv, rm, rm, 1e-5, None, T, B, K, C,
                d_feat, B * dfeat_sb, dfeat_sb, out, P, P, P, P, 1 << 30, None]
    if untyped:
        args.remove(dtype)                                   # (the first int among the arguments that equals it: feat_dtype)
        return getattr(lib, SIBLINGS[name])(*args)
    return getattr(lib, name)(*args)


@pytest.mark.parametrize("dtype", [F32, BF16, F16])
@pytest.mark.parametrize("name", ENTRIES)
def test_null_feat(lib, name, dtype):
    assert _call(lib, name, dtype, feat=None) == BAD_ARGUMENT
    assert _call(lib, name, dtype, feat=None, K=24) == BAD_ARGUMENT              # the bad argument wins over the shape


@pytest.mark.parametrize("dtype", [3, -1, 7, 1 << 20])
@pytest.mark.parametrize("name", ENTRIES)
def test_unknown_feat_dtype(lib, name, dtype):
    assert _call(lib, name, dtype) == BAD_ARGUMENT
    assert _call(lib, name, dtype, eval_mode=True) == BAD_ARGUMENT
    assert _call(lib, name, dtype, K=24) == BAD_ARGUMENT


@pytest.mark.parametrize("dtype", [BF16, F16])
@pytest.mark.parametrize("name", ENTRIES)
def test_two_byte_alignment_rule(lib, name, dtype):
    """the 16-byte rule on feat is an 8-byte rule for the 2-byte types: address, strides in multiples of 4 elements, K % 16"""
    for bad in (dict(feat=P + 4), dict(feat=P + 2), dict(feat=P + 12), dict(fsb=38), dict(fst=3 * 1000 * 32 + 2), dict(K=24)):
        assert _call(lib, name, dtype, **bad) == UNSUPPORTED_SHAPE, bad
        assert _call(lib, name, dtype, eval_mode=True, **bad) == UNSUPPORTED_SHAPE, bad
    assert _call(lib, name, dtype, fsb=6) == UNSUPPORTED_SHAPE
    # an address = 8 (mod 16) is not refused for its alignment: the call goes on to a later check (a NULL output)
    assert _call(lib, name, dtype, feat=P + 8, out=None) == BAD_ARGUMENT
    assert _call(lib, name, dtype, feat=P + 8, fsb=36, out=None) == BAD_ARGUMENT
    # ... which the fp32 element type refuses, as the untyped entry does (the shape is decided behind the arguments)
    assert _call(lib, name, F32, feat=P + 8) == UNSUPPORTED_SHAPE


@pytest.mark.parametrize("dtype", [BF16, F16])
@pytest.mark.parametrize("name", [n for n in ENTRIES if "backward" in n])
def test_d_feat_rules(lib, name, dtype):
    assert _call(lib, name, dtype, d_feat=P + 1) == UNSUPPORTED_SHAPE            # 2-byte stores
    assert _call(lib, name, dtype, dfeat_sb=31) == BAD_ARGUMENT                  # a row pitch below K: the sibling's code
    assert _call(lib, name, dtype, d_feat=P + 2, out=None) == BAD_ARGUMENT       # 2-byte aligned is enough
    assert _call(lib, name, dtype, d_feat=None, out=None) == BAD_ARGUMENT        # d_feat stays optional


@pytest.mark.parametrize("name", ENTRIES)
def test_f32_is_the_untyped_entry(lib, name):
    """the same answers as the sibling for the same (bogus) arguments, bad and unsupported"""
    for kw in (dict(feat=None), dict(K=24), dict(feat=P + 8), dict(feat=P + 4), dict(fsb=34), dict(out=None), dict(T=0)):
        got = _call(lib, name, F32, **kw)
        assert got == _call(lib, name, F32, untyped=True, **kw) and got in (BAD_ARGUMENT, UNSUPPORTED_SHAPE), kw


@pytest.mark.parametrize("dtype", [F32, BF16, F16])
def test_narrow_forward_one_row_in_train_mode_wins_over_the_shape(lib, dtype):
    """train mode needs two rows per frame: a bad argument, answered before the shape as in every sibling (the wide forward, both
    backward entries) -- B = 1 with K = 24, B = 1 with a misaligned feat"""
    name = "ctc_amd_head_forward_typed"
    assert _call(lib, name, dtype, B=1) == BAD_ARGUMENT
    assert _call(lib, name, dtype, B=1, K=24) == BAD_ARGUMENT
    assert _call(lib, name, dtype, B=1, feat=P + 4) == BAD_ARGUMENT
    if dtype == F32:
        assert _call(lib, name, dtype, B=1, K=24, untyped=True) == BAD_ARGUMENT
        assert _call(lib, name, dtype, B=1, feat=P + 4, untyped=True) == BAD_ARGUMENT
    # eval mode takes a single row, so there the shape answers
    assert _call(lib, name, dtype, B=1, K=24, eval_mode=True) == UNSUPPORTED_SHAPE
    assert _call(lib, name, dtype, B=1, feat=P + 4, eval_mode=True) == UNSUPPORTED_SHAPE


def test_no_cpu_path_for_two_byte_features():
    import torch
    import ctc_amd
    z = torch.zeros
    for dt in (torch.bfloat16, torch.float16):
        with pytest.raises(ctc_amd.CtcAmdError):
            ctc_amd.head_forward(z(2, 10, 16, dtype=dt), z(5, 16), z(5), z(5), z(5))
        with pytest.raises(ctc_amd.CtcAmdError):
            ctc_amd.head_backward(z(2, 10, 5), z(2, 10, 16, dtype=dt), z(5, 16), z(5), z(5), z(2, 10, 5), mean=z(2, 5),
                                  invstd=torch.ones(2, 5))
