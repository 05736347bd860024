"""The recurrence for up to 160 classes (ctc_amd_lstm_series_wide, its scratch query, ctc_amd_lstm_series_backward_wide): the
C ABI (declared, exported, bound, every argument error reported before any HIP call -- bogus host pointers, no device
needed) and the Python surface.  tests/test_lstm_wide_gpu.py checks the kernels."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FWD, QUERY, BWD = "ctc_amd_lstm_series_wide", "ctc_amd_lstm_series_wide_scratch_bytes", "ctc_amd_lstm_series_backward_wide"
FWD_REQUIRED = ["x", "h0", "c0", "w_ih", "w_hh", "b_ih", "b_hh", "series", "scratch"]
FWD_OPTIONAL = ["gates_out", "cells_out", "h_out", "c_out"]
BIAS = "ctc_amd_lstm_bias_grad_wide"
BWD_REQUIRED = ["d_series", "gates", "cells", "w_hh", "dpre_out", "dh0_out", "dc0_out"]
BAD_ARGUMENT, UNSUPPORTED_SHAPE = -1, -2
UNSUPPORTED = [dict(I=161, H=8), dict(I=8, H=161), dict(I=161, H=161)]


@pytest.fixture(scope="module")
def lib():
    from ctc_amd import _lib, build
    build.build()
    return _lib.load()


def test_symbols_declared_exported_and_bound(lib):
    from ctc_amd import _lib
    header = open(os.path.join(ROOT, "include", "ctc_amd.h")).read()
    so = ctypes.CDLL(_lib.SO_PATH)
    for name, nargs in ((FWD, 23), (BWD, 13), (BIAS, 6)):
        m = re.search(r"\bint %s\s*\(([^;]*)\);" % name, header)
        assert m, "%s is not declared in include/ctc_amd.h" % name
        declared = [a for a in m.group(1).split(",") if a.strip()]
        assert hasattr(so, name)
        res, args = _lib.PROTOTYPES[name]
        assert res is ctypes.c_int and len(args) == len(declared) == nargs
    assert re.search(r"\bsize_t %s\s*\(int T, int B, int I, int H\);" % QUERY, header)
    assert hasattr(so, QUERY)
    res, args = _lib.PROTOTYPES[QUERY]
    assert res is ctypes.c_size_t and len(args) == 4
    # the wide entry takes the narrow entry's arguments, then the scratch, then the stream
    narrow = _lib.PROTOTYPES["ctc_amd_lstm_series"][1]
    wide = _lib.PROTOTYPES[FWD][1]
    assert wide[:len(narrow) - 1] == narrow[:-1] and wide[-3:] == [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    assert _lib.PROTOTYPES[BWD][1] == _lib.PROTOTYPES["ctc_amd_lstm_series_backward"][1]


def _fwd(lib, ptr=4096, T=7, B=9, I=158, H=158, cols=None, stride_b=None, scratch_bytes=None, **null):
    """every pointer is a bogus, 16-byte aligned host address: a call that got past the checks would fault, not return.
    null: NAME=True makes a pointer NULL."""
    present = {k: True for k in FWD_REQUIRED + FWD_OPTIONAL}
    for k, v in null.items():
        assert k in present
        present[k] = not v
    p = {k: (ptr if present[k] else None) for k in present}
    cols = H + 1 if cols is None else cols
    stride_b = cols if stride_b is None else stride_b
    if scratch_bytes is None:
        scratch_bytes = max(lib.ctc_amd_lstm_series_wide_scratch_bytes(T, B, I, H), 1)
    return lib.ctc_amd_lstm_series_wide(p["x"], p["h0"], p["c0"], p["w_ih"], p["w_hh"], p["b_ih"], p["b_hh"], T, B, I, H,
                                        p["series"], B * stride_b, stride_b, cols, -1.0e30,
                                        p["gates_out"], p["cells_out"], p["h_out"], p["c_out"], p["scratch"], scratch_bytes, None)


def _bwd(lib, ptr=4096, T=7, B=9, H=158, **null):
    present = {k: True for k in BWD_REQUIRED}
    for k, v in null.items():
        assert k in present
        present[k] = not v
    p = {k: (ptr if present[k] else None) for k in present}
    return lib.ctc_amd_lstm_series_backward_wide(p["d_series"], B * (H + 1), H + 1, p["gates"], p["cells"], p["w_hh"], T, B, H,
                                                 p["dpre_out"], p["dh0_out"], p["dc0_out"], None)


@pytest.mark.parametrize("which", FWD_REQUIRED)
def test_forward_null_pointers(lib, which):
    assert _fwd(lib, **{which: True}) == BAD_ARGUMENT
    assert _fwd(lib, gates_out=True, cells_out=True, h_out=True, c_out=True, **{which: True}) == BAD_ARGUMENT
    assert _fwd(lib, I=161, H=161, **{which: True}) == BAD_ARGUMENT         # the bad argument wins over the shape


@pytest.mark.parametrize("which", BWD_REQUIRED)
def test_backward_null_pointers(lib, which):
    assert _bwd(lib, **{which: True}) == BAD_ARGUMENT
    assert _bwd(lib, H=161, **{which: True}) == BAD_ARGUMENT


@pytest.mark.parametrize("kw", [
    dict(T=0), dict(B=0), dict(I=0), dict(H=0), dict(T=-3), dict(B=-1), dict(I=-2), dict(H=-1),
    dict(cols=157), dict(cols=158, stride_b=157), dict(cols=160, stride_b=159),
    dict(scratch_bytes=0),
    dict(T=0, H=161), dict(cols=8, I=8, H=161, stride_b=200),
])
def test_forward_bad_arguments(lib, kw):
    assert _fwd(lib, **kw) == BAD_ARGUMENT


@pytest.mark.parametrize("kw", [dict(T=0), dict(B=0), dict(H=0), dict(T=-3), dict(B=-1), dict(H=-1), dict(T=0, H=161)])
def test_backward_bad_arguments(lib, kw):
    assert _bwd(lib, **kw) == BAD_ARGUMENT


def test_bias_grad_arguments(lib):
    """the column sums behind the backward recurrence: dpre, rows, H, d_b_ih, d_b_hh, stream"""
    f, p = lib.ctc_amd_lstm_bias_grad_wide, 4096
    for args in ((None, 63, 158, p, p), (p, 63, 158, None, p), (p, 63, 158, p, None), (p, 0, 158, p, p), (p, -4, 158, p, p),
                 (p, 63, 0, p, p), (p, 63, -1, p, p), (None, 63, 161, p, p), (p, 0, 161, p, p)):
        assert f(*args, None) == BAD_ARGUMENT, args
    assert f(p, 63, 161, p, p, None) == UNSUPPORTED_SHAPE
    assert f(p, 1 << 40, 1 << 30, p, p, None) == UNSUPPORTED_SHAPE


def test_the_scratch_bound_is_the_query(lib):
    for (T, B, I, H) in ((7, 9, 158, 158), (1, 1, 1, 1), (2, 1, 160, 160), (9, 5, 17, 40)):
        need = lib.ctc_amd_lstm_series_wide_scratch_bytes(T, B, I, H)
        assert need > 0
        assert _fwd(lib, T=T, B=B, I=I, H=H, scratch_bytes=need - 1) == BAD_ARGUMENT
        assert _fwd(lib, T=T, B=B, I=I, H=H, scratch_bytes=need - 1, gates_out=True, cells_out=True) == BAD_ARGUMENT


@pytest.mark.parametrize("kw", UNSUPPORTED, ids=lambda kw: "-".join("%s%d" % kv for kv in kw.items()))
def test_unsupported_shapes(lib, kw):
    assert _fwd(lib, **kw) == UNSUPPORTED_SHAPE
    assert _fwd(lib, gates_out=True, cells_out=True, h_out=True, c_out=True, **kw) == UNSUPPORTED_SHAPE
    assert _fwd(lib, scratch_bytes=0, **kw) == UNSUPPORTED_SHAPE            # (the query is 0 there: nothing to be short of)
    assert lib.ctc_amd_lstm_series_wide_scratch_bytes(7, 9, kw["I"], kw["H"]) == 0
    assert _bwd(lib, H=161) == UNSUPPORTED_SHAPE
    assert _bwd(lib, H=1 << 30) == UNSUPPORTED_SHAPE


def test_scratch_query(lib):
    q = lib.ctc_amd_lstm_series_wide_scratch_bytes
    base = dict(T=10, B=10, I=158, H=158)
    for kw in UNSUPPORTED + [dict(T=0), dict(B=0), dict(I=0), dict(H=0), dict(T=-1), dict(B=-7), dict(I=-2), dict(H=-5),
                             dict(I=1 << 30), dict(H=1 << 30)]:
        a = dict(base, **kw)
        assert q(a["T"], a["B"], a["I"], a["H"]) == 0, kw
    for (I, H) in ((158, 158), (1, 1), (160, 160)):
        assert q(10, 10, I, H) > 0
        # the transposed weights [I + H][4H] and the x part of every row [T B][4H] at the least
        assert q(10, 10, I, H) >= 4 * ((I + H) * 4 * H + 100 * 4 * H)
    # T B near 2^22: more than 2^32 bytes, no overflow on the way; one frame beyond the row bound is not taken
    rows = 1 << 22
    assert q(rows // 8, 8, 160, 160) >= 4 * rows * 640 > 1 << 32
    assert q(rows // 8 - 1, 8, 158, 158) >= 4 * (rows - 8) * 632
    assert q(rows, 1, 1, 1) >= 4 * rows * 4
    assert q(rows // 8 + 1, 8, 158, 158) == 0
    assert q(1 << 30, 1 << 30, 158, 158) == 0
    assert _fwd(lib, T=rows // 8 + 1, B=8) == UNSUPPORTED_SHAPE


def test_python_export():
    import ctc_amd
    from ctc_amd import producer
    for name in ("lstm_series_wide", "lstm_series_backward_wide", "lstm_bias_grad_wide"):
        assert callable(getattr(producer, name)) and getattr(ctc_amd, name) is getattr(producer, name)
        assert name in ctc_amd.__all__
    assert type(producer.SERIES_WIDE_MAX_ROWS) is int and producer.SERIES_WIDE_MAX_ROWS >= 0
    import inspect
    assert "recurrence" in inspect.signature(producer._series_backward_torch).parameters
    assert producer.SERIES_WIDE_MAX_CLASSES == 160


def test_no_cpu_path():
    import torch
    import ctc_amd
    z = torch.zeros
    T, B, I, H = 2, 2, 70, 70
    with pytest.raises(ctc_amd.CtcAmdError):
        ctc_amd.lstm_series_wide(z(T, B, I), z(B, H), z(B, H), z(4 * H, I), z(4 * H, H), z(4 * H), z(4 * H))
    with pytest.raises(ctc_amd.CtcAmdError):
        ctc_amd.lstm_series_backward_wide(z(T, B, H), z(T, B, 4 * H), z(T + 1, B, H), z(4 * H, H))
    with pytest.raises(ctc_amd.CtcAmdError):
        ctc_amd.lstm_bias_grad_wide(z(T, B, 4 * H))
