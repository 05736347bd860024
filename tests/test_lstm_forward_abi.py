"""The eval-mode producer as one launch (ctc_amd_lstm_forward): the C ABI (declared, exported, bound, every argument
error reported before any HIP call -- host pointers, no device needed) and the Python surface.
tests/test_lstm_forward_gpu.py checks the kernel against the two launches it replaces."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "ctc_amd_lstm_forward"
POINTERS = ["feat", "weight", "bias", "bn_weight", "bn_bias", "running_mean", "running_var", "h0", "c0",
            "w_ih", "w_hh", "b_ih", "b_hh", "series"]
BAD_ARGUMENT, UNSUPPORTED_SHAPE = -1, -2


@pytest.fixture(scope="module")
def lib():
    from ctc_amd import _lib, build
    build.build()
    return _lib.load()


def test_symbol_declared_exported_and_bound(lib):
    from ctc_amd import _lib
    header = open(os.path.join(ROOT, "include", "ctc_amd.h")).read()
    m = re.search(r"\bint %s\s*\(([^;]*)\);" % NAME, header)
    assert m, "not declared in include/ctc_amd.h"
    declared = [a for a in m.group(1).split(",") if a.strip()]
    assert hasattr(ctypes.CDLL(_lib.SO_PATH), NAME)
    res, args = _lib.PROTOTYPES[NAME]
    assert res is ctypes.c_int and len(args) == len(declared) == 28
    assert lib.ctc_amd_abi_version() == 2 and _lib.ABI_VERSION == 2
    assert "#define CTC_AMD_ABI_VERSION 2" in header


def _call(lib, ptr=4096, T=10, B=10, K=1024, C=33, cols=None, stride_b=None, feat_ptr=None, fst=None, fsb=None, **null):
    """every pointer is a bogus, 16-byte aligned host address: a call that got past the checks would fault, not return"""
    p = {k: (None if null.get(k) else ptr) for k in POINTERS}
    if feat_ptr is not None:
        p["feat"] = feat_ptr
    cols = C if cols is None else cols
    stride_b = cols if stride_b is None else stride_b
    fsb = K if fsb is None else fsb
    fst = B * fsb if fst is None else fst
    return lib.ctc_amd_lstm_forward(p["feat"], fst, fsb, p["weight"], p["bias"], p["bn_weight"], p["bn_bias"],
                                    p["running_mean"], p["running_var"], 1e-5, p["h0"], p["c0"], p["w_ih"], p["w_hh"],
                                    p["b_ih"], p["b_hh"], T, B, K, C, p["series"], B * stride_b, stride_b, cols, -1.0e30,
                                    None, None, None)


@pytest.mark.parametrize("which", POINTERS)
def test_null_pointers(lib, which):
    # (running_mean / running_var among them: the entry has no train mode)
    assert _call(lib, **{which: True}) == BAD_ARGUMENT


@pytest.mark.parametrize("kw", [dict(T=0), dict(B=0), dict(K=0), dict(C=0), dict(T=-3), dict(cols=32), dict(cols=34, stride_b=33),
                                dict(T=0, C=41, cols=41), dict(running_mean=True, K=24)])
def test_bad_arguments(lib, kw):
    # non-positive sizes, series_cols < C, series_stride_b < series_cols; (the last two: a bad argument is reported
    # before the shape is looked at)
    assert _call(lib, **kw) == BAD_ARGUMENT


@pytest.mark.parametrize("kw", [dict(C=41),                      # 2 C = 82 > 80
                                dict(K=24),                      # not a multiple of 16
                                dict(feat_ptr=4096 + 4),         # feat off by 4 bytes
                                dict(fsb=1026), dict(fst=10 * 1024 + 2),        # strides that are no multiples of 4
                                dict(ptr=4096 + 8, feat_ptr=4096),              # (weight unaligned)
                                dict(T=400),                     # 4 * 400 * 33 floats = 206 KB of LDS
                                dict(T=1 << 30)])                # (no int overflow on the way to that answer)
def test_unsupported_shapes(lib, kw):
    assert _call(lib, **kw) == UNSUPPORTED_SHAPE


def test_lds_bound_is_the_slice_plus_the_staging(lib):
    # C = 33: staging 4 * (68 + 132 + 33) floats, slice 4 * T * 33 floats, 160 KiB in all.  T = 303 fits (the call would go
    # on to launch: not made here), T = 304 does not
    need = lambda T: 4 * (4 * (68 + 132 + 33) + 4 * T * 33)     # noqa: E731
    assert need(303) <= 160 * 1024 < need(304)
    assert _call(lib, T=304) == UNSUPPORTED_SHAPE


def test_python_export():
    import ctc_amd
    from ctc_amd import producer
    assert callable(producer.lstm_forward) and ctc_amd.lstm_forward is producer.lstm_forward
    assert "lstm_forward" in ctc_amd.__all__
    assert isinstance(producer.FUSED_FORWARD_MAX_WG_ROWS, int)


def test_no_cpu_path():
    import torch
    import ctc_amd
    z = torch.zeros
    with pytest.raises(ctc_amd.CtcAmdError):
        ctc_amd.lstm_forward(z(2, 2, 16), z(5, 16), z(5), z(5), z(5), z(5), torch.ones(5), 1e-5, z(2, 5), z(2, 5),
                             z(20, 5), z(20, 5), z(20), z(20))
