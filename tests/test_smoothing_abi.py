"""C ABI of the fp32 label-smoothed no-blank loss: the entry point is declared, exported and bound, and rejects a
label_smoothing outside [0, 1] before any pointer is touched or anything is launched (runs without a GPU)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "ctc_amd_noblank_smoothed_loss_grad"


@pytest.fixture(scope="module")
def lib():
    from ctc_amd import _lib, build
    build.build()
    return _lib.load()


def test_smoothed_symbol_declared_exported_and_bound(lib):
    from ctc_amd import _lib
    header = open(os.path.join(ROOT, "include", "ctc_amd.h")).read()
    assert re.search(r"\bint\s+%s\s*\(" % NAME, header)
    assert hasattr(ctypes.CDLL(_lib.SO_PATH), NAME)
    assert NAME in _lib.PROTOTYPES
    restype, argtypes = _lib.PROTOTYPES[NAME]
    # the plain entry's arguments with the float label_smoothing behind S (include/ctc_amd.h)
    plain = _lib.PROTOTYPES["ctc_amd_noblank_loss_grad"][1]
    assert restype is ctypes.c_int and len(argtypes) == len(plain) + 1 == 19
    assert argtypes[11] is ctypes.c_float and list(argtypes[:11]) + list(argtypes[12:]) == list(plain)
    decl = re.search(r"%s\s*\(([^;]*)\);" % NAME, header).group(1)
    assert re.search(r"int\s+S\s*,\s*float\s+label_smoothing\s*,\s*float\s+loss_scale", decl)


def _smoothed(lib, ls, ptr=None):
    return lib.ctc_amd_noblank_smoothed_loss_grad(ptr, 0, 0, ptr, 0, ptr, ptr, 1, 1, 2, 1, ls, 1.0, 1.0,
                                                  ptr, ptr, None, ptr, None)


@pytest.mark.parametrize("ls", [-0.5, -1e-6, 1.0 + 1e-6, 1.5, float("inf"), -float("inf"), float("nan")])
def test_smoothed_entry_bad_smoothing(lib, ls):
    # rejected before anything is dereferenced or launched: non-null but bogus pointers are never touched
    from ctc_amd import _lib
    assert _smoothed(lib, ls, ptr=16) == _lib.ERR_BAD_ARGUMENT == -1


@pytest.mark.parametrize("ls", [0.0, 0.5, 1.0])
def test_smoothed_entry_null_pointers(lib, ls):
    assert _smoothed(lib, ls) == -1
