"""C ABI of the bf16 / fp16 no-blank loss: the typed entry points are declared, exported and bound, and reject bad
arguments before any HIP call (runs without a GPU)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TYPED = ("ctc_amd_noblank_loss_grad_typed", "ctc_amd_scale_grad_typed")


@pytest.fixture(scope="module")
def lib():
    from ctc_amd import _lib, build
    build.build()
    return _lib.load()


def test_typed_symbols_declared_exported_and_bound(lib):
    from ctc_amd import _lib
    header = open(os.path.join(ROOT, "include", "ctc_amd.h")).read()
    raw = ctypes.CDLL(_lib.SO_PATH)
    for name in TYPED:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(raw, name), name
        assert name in _lib.PROTOTYPES, name
    for macro, value in (("CTC_AMD_F32", 0), ("CTC_AMD_BF16", 1), ("CTC_AMD_F16", 2)):
        assert re.search(r"#define\s+%s\s+%d\b" % (macro, value), header), macro
    assert (_lib.F32, _lib.BF16, _lib.F16) == (0, 1, 2)
    assert lib.ctc_amd_abi_version() == 2


def _typed(lib, dtype, ptr=None, ls=-1.0):
    return lib.ctc_amd_noblank_loss_grad_typed(ptr, dtype, 0, 0, ptr, 0, ptr, ptr, 1, 1, 2, 1, ls, 1.0, 1.0,
                                               ptr, ptr, None, ptr, None)


@pytest.mark.parametrize("dtype", [0, 1, 2])
def test_typed_entry_null_pointers(lib, dtype):
    assert _typed(lib, dtype) == -1
    assert _typed(lib, dtype, ls=0.5) == -1


@pytest.mark.parametrize("dtype", [-1, 3, 7])
def test_typed_entry_unknown_dtype(lib, dtype):
    # rejected before anything is dereferenced or launched: non-null but bogus pointers are never touched
    assert _typed(lib, dtype, ptr=16) == -1


def test_typed_entry_bad_smoothing(lib):
    assert _typed(lib, 1, ptr=16, ls=1.5) == -1
    assert _typed(lib, 1, ptr=16, ls=float("nan")) == -1


def test_scale_grad_typed_rejects(lib):
    for dtype in (0, 1, 2):
        assert lib.ctc_amd_scale_grad_typed(None, dtype, None, 4, None) == -1
    assert lib.ctc_amd_scale_grad_typed(16, 5, 16, 4, None) == -1

