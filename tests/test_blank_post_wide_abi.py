"""Blank-CTC posteriors on the wide lattice (256 <= S <= 1023): the C ABI of ctc_amd_blank_posteriors_wide -- declared,
exported, bound, argument errors before any HIP call, the range each of the two posteriors entries takes and the workspace
the wide one fits into (runs without a GPU).  tests/test_blank_post_wide_gpu.py checks the kernels against the float64
restatement."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "ctc_amd_blank_posteriors_wide"


@pytest.fixture(scope="module")
def lib():
    from ctc_amd import _lib, build
    build.build()
    return _lib.load()


def test_symbol_declared_exported_and_bound(lib):
    from ctc_amd import _lib
    header = open(os.path.join(ROOT, "include", "ctc_amd.h")).read()
    assert re.search(r"\b%s\s*\(" % NAME, header)
    assert hasattr(ctypes.CDLL(_lib.SO_PATH), NAME)
    res, args = _lib.PROTOTYPES[NAME]
    assert res is ctypes.c_int and len(args) == 16
    assert args == _lib.PROTOTYPES["ctc_amd_blank_posteriors"][1]
    assert lib.ctc_amd_abi_version() == 2


def _call(lib, entry=NAME, ptr=16, T=4, B=2, C=5, S=300, blank=0, **null):
    p = {k: (None if null.get(k) else ptr) for k in ("lp", "tgt", "il", "tl", "nll", "gamma", "ws")}
    return getattr(lib, entry)(p["lp"], 0, 0, p["tgt"], 0, p["il"], p["tl"], T, B, C, S, blank,
                               p["nll"], p["gamma"], p["ws"], None)


@pytest.mark.parametrize("which", ["lp", "tgt", "il", "tl", "nll", "gamma", "ws"])
def test_null_pointers(lib, which):
    # rejected before anything is dereferenced or launched: the other pointers are non-null but bogus
    assert _call(lib, **{which: True}) == -1


@pytest.mark.parametrize("kw", [dict(T=0), dict(B=0), dict(C=0), dict(S=0), dict(T=-3), dict(S=-1), dict(blank=-1),
                                dict(blank=5), dict(C=5, blank=7)])
def test_bad_sizes_and_blank(lib, kw):
    assert _call(lib, **kw) == -1


@pytest.mark.parametrize("S", [1, 255, 1024, 5000])
def test_outside_the_wide_range(lib, S):
    assert _call(lib, S=S) == -2


def test_bad_arguments_come_before_the_range(lib):
    assert _call(lib, S=255, lp=True) == -1
    assert _call(lib, S=1024, blank=9) == -1


def test_the_narrow_entry_keeps_its_range(lib):
    assert _call(lib, entry="ctc_amd_blank_posteriors", S=256) == -2
    assert _call(lib, entry="ctc_amd_blank_posteriors", S=1023) == -2


@pytest.mark.parametrize("S", [256, 511, 512, 1023])
def test_the_lattice_areas_hold_the_table_and_both_chains(lib, S):
    """the emission table (256 W + 4 floats per frame) and the alpha' / beta' rows (512 W each) behind the 256-byte header"""
    from ctc_amd import _lib
    W = (2 * S + 1 + 511) // 512
    for T, B, C in ((1, 1, 2), (7, 3, 5), (1250, 2, 20)):
        assert lib.ctc_amd_workspace_bytes(_lib.BLANK, T, B, C, S) >= 256 + 4 * B * T * (1280 * W + 4)


def test_cpu_tensor_raises():
    import ctc_amd
    T, B, C, S = 6, 2, 5, 300                                     # no CPU path
    lp = torch.randn(T, B, C).log_softmax(2)
    with pytest.raises(ctc_amd.CtcAmdError):
        ctc_amd.blank_posteriors(lp, torch.ones(B, S, dtype=torch.long), torch.tensor([6, 6]), torch.tensor([2, 2]))
