"""The recurrence's backward on the HIP path, whole (ctc_amd_lstm_backward): the C ABI (declared, exported, bound, every
argument error reported before any HIP call -- bogus host pointers, no device needed) and the Python surface.
tests/test_lstm_backward_gpu.py checks the kernels against oracle.ctc_numpy.lstm_cell_series_backward."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME, QUERY = "ctc_amd_lstm_backward", "ctc_amd_lstm_backward_scratch_bytes"
REQUIRED = ["d_series", "gates", "cells", "x", "h0", "series", "w_ih", "w_hh", "dh0", "dc0", "d_w_ih", "d_w_hh", "d_b_ih",
            "d_b_hh", "scratch"]
BAD_ARGUMENT, UNSUPPORTED_SHAPE = -1, -2
# shapes the entry does not take: what ctc_amd_lstm_series refuses, and more than 2^22 rows
UNSUPPORTED = [dict(I=40, H=41),                        # I + H = 81
               dict(I=15, H=65), dict(I=65, H=15),
               dict(T=1 << 30),                         # (no int overflow on the way to that answer)
               dict(T=(1 << 22) // 8 + 1, B=8)]         # one frame beyond 2^22 rows


@pytest.fixture(scope="module")
def lib():
    from ctc_amd import _lib, build
    build.build()
    return _lib.load()


def test_symbols_declared_exported_and_bound(lib):
    from ctc_amd import _lib
    header = open(os.path.join(ROOT, "include", "ctc_amd.h")).read()
    m = re.search(r"\bint %s\s*\(([^;]*)\);" % NAME, header)
    assert m, "not declared in include/ctc_amd.h"
    declared = [a for a in m.group(1).split(",") if a.strip()]
    assert re.search(r"\bsize_t %s\s*\(int T, int B, int I, int H\);" % QUERY, header)
    so = ctypes.CDLL(_lib.SO_PATH)
    assert hasattr(so, NAME) and hasattr(so, QUERY)
    res, args = _lib.PROTOTYPES[NAME]
    assert res is ctypes.c_int and len(args) == len(declared) == 30
    res, args = _lib.PROTOTYPES[QUERY]
    assert res is ctypes.c_size_t and len(args) == 4
    assert lib.ctc_amd_abi_version() == 2 and _lib.ABI_VERSION == 2
    assert "#define CTC_AMD_ABI_VERSION 2" in header


def _call(lib, ptr=4096, T=10, B=10, I=33, H=33, ds_sb=None, x_sb=None, series_sb=None, dx_sb=None, scratch_bytes=None, **null):
    """every pointer is a bogus, 16-byte aligned host address: a call that got past the checks would fault, not return.
    null: NAME=True makes a pointer NULL."""
    present = {k: True for k in REQUIRED}
    present["d_x"] = True
    for k, v in null.items():
        assert k in present
        present[k] = not v
    p = {k: (ptr if present[k] else None) for k in present}
    ds_sb = H + 1 if ds_sb is None else ds_sb
    x_sb = I if x_sb is None else x_sb
    series_sb = H + 1 if series_sb is None else series_sb
    dx_sb = I if dx_sb is None else dx_sb
    if scratch_bytes is None:
        scratch_bytes = max(lib.ctc_amd_lstm_backward_scratch_bytes(T, B, I, H), 1)
    return lib.ctc_amd_lstm_backward(p["d_series"], B * ds_sb, ds_sb, p["gates"], p["cells"], p["x"], B * x_sb, x_sb, p["h0"],
                                     p["series"], B * series_sb, series_sb, p["w_ih"], p["w_hh"], T, B, I, H,
                                     p["d_x"], B * dx_sb, dx_sb, p["dh0"], p["dc0"], p["d_w_ih"], p["d_w_hh"], p["d_b_ih"],
                                     p["d_b_hh"], p["scratch"], scratch_bytes, None)


@pytest.mark.parametrize("which", REQUIRED)
def test_null_pointers(lib, which):
    assert _call(lib, **{which: True}) == BAD_ARGUMENT
    assert _call(lib, d_x=True, **{which: True}) == BAD_ARGUMENT


@pytest.mark.parametrize("kw", [
    dict(T=0), dict(B=0), dict(I=0), dict(H=0), dict(T=-3), dict(H=-1), dict(I=-2), dict(B=-1),
    dict(ds_sb=32), dict(series_sb=32), dict(x_sb=32), dict(dx_sb=32),
    dict(scratch_bytes=0),
    # a bad argument together with an unsupported shape: the bad argument wins
    dict(T=0, H=65), dict(d_series=True, I=40, H=41), dict(scratch=True, T=1 << 30), dict(d_b_hh=True, I=65, H=15),
    dict(ds_sb=64, I=15, H=65), dict(x_sb=39, I=40, H=41), dict(dx_sb=5, T=(1 << 22) // 8 + 1, B=8), dict(gates=True, T=1 << 30),
])
def test_bad_arguments(lib, kw):
    assert _call(lib, **kw) == BAD_ARGUMENT


def test_the_scratch_bound_is_the_query(lib):
    need = lib.ctc_amd_lstm_backward_scratch_bytes(10, 10, 33, 33)
    assert need > 0
    assert _call(lib, scratch_bytes=need - 1) == BAD_ARGUMENT
    assert _call(lib, scratch_bytes=need - 1, d_x=True) == BAD_ARGUMENT


@pytest.mark.parametrize("kw", UNSUPPORTED, ids=lambda kw: "-".join("%s%d" % kv for kv in kw.items()))
def test_unsupported_shapes(lib, kw):
    """with and without d_x (d_x = NULL passes the argument checks: the answer is the shape's, not BAD_ARGUMENT)"""
    assert _call(lib, **kw) == UNSUPPORTED_SHAPE
    assert _call(lib, d_x=True, **kw) == UNSUPPORTED_SHAPE


def test_scratch_query(lib):
    q = lib.ctc_amd_lstm_backward_scratch_bytes
    base = dict(T=10, B=10, I=33, H=33)
    for kw in UNSUPPORTED + [dict(T=0), dict(B=0), dict(I=0), dict(H=0), dict(T=-1), dict(H=-5)]:
        a = dict(base, **kw)
        assert q(a["T"], a["B"], a["I"], a["H"]) == 0, kw
    assert q(10, 10, 33, 33) > 0
    # dpre [T B][4H] at the least; the partial sums [S][4H (I + H + 1)] beyond 128 rows
    assert q(10, 10, 33, 33) >= 4 * 100 * 132
    assert q(150, 64, 33, 33) >= 4 * (9600 * 132 + 60 * 132 * 67)           # (60 ranges of 160 rows)
    assert q((1 << 22) // 8, 8, 16, 64) > 0


def test_python_export():
    import ctc_amd
    from ctc_amd import producer
    assert callable(producer.lstm_backward) and ctc_amd.lstm_backward is producer.lstm_backward
    assert "lstm_backward" in ctc_amd.__all__
    assert type(producer.SERIES_BACKWARD_MAX_ROWS) is int and producer.SERIES_BACKWARD_MAX_ROWS >= 0
    assert callable(producer._series_backward_torch)


def test_no_cpu_path():
    import torch
    import ctc_amd
    z = torch.zeros
    T, B, I, H = 2, 2, 5, 4
    with pytest.raises(ctc_amd.CtcAmdError):
        ctc_amd.lstm_backward(z(T, B, H), z(T, B, 4 * H), z(T + 1, B, H), z(T, B, I), z(B, H), z(T, B, H), z(4 * H, I), z(4 * H, H))
