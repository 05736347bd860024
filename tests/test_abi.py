"""C-ABI library: loads, exports every symbol include/ctc_amd.h declares; host-side
validation of the Python mirror (no compute calls: runs without a GPU)."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built():
    from ctc_amd import build
    return build.build()


def _declared():
    src = open(os.path.join(ROOT, "include", "ctc_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(ctc_amd_[a-z_0-9]+)\s*\(", src)))


def test_header_symbols_exported(built):
    lib = ctypes.CDLL(built)
    names = _declared()
    assert len(names) >= 8
    for n in names:
        assert hasattr(lib, n), "libctc_amd.so does not export %s" % n


def test_binding_covers_header(built):
    from ctc_amd import _lib
    assert sorted(_lib.PROTOTYPES) == _declared()
    lib = _lib.load()
    assert lib.ctc_amd_abi_version() == _lib.ABI_VERSION == 2
    assert lib.ctc_amd_workspace_bytes(0, 150, 256, 158, 20) >= 256
    assert lib.ctc_amd_workspace_bytes(2, 2000, 64, 1000, 100) >= 2 * 64 * 2000 * 201 * 4
    assert b"success" in lib.ctc_amd_error_string(0)


def _c_kind(decl):
    """one C parameter or return declaration -> 'ptr', 'int', 'int64', 'float', 'size_t', 'unsigned', 'void'"""
    decl = " ".join(decl.replace("*", " * ").split())
    if "*" in decl:
        return "ptr"
    words = [w for w in decl.split() if w != "const"]
    kinds = {"int": "int", "int64_t": "int64", "float": "float", "size_t": "size_t", "unsigned": "unsigned", "void": "void"}
    assert words and words[0] in kinds, decl
    return kinds[words[0]]


def _header_prototypes():
    """name -> (return kind, [argument kinds]) of every prototype of include/ctc_amd.h, comments stripped"""
    src = open(os.path.join(ROOT, "include", "ctc_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = "\n".join(l for l in src.splitlines() if not l.lstrip().startswith("#"))
    out = {}
    for ret, name, args in re.findall(r"([A-Za-z_][A-Za-z_0-9 \t\n\*]*?)\b(ctc_amd_[a-z_0-9]+)\s*\(([^()]*)\)\s*;", src):
        ret = ret.replace('extern "C"', "").replace("{", " ").strip()
        args = [a.strip() for a in args.split(",")]
        out[name] = (_c_kind(ret), [] if args == ["void"] else [_c_kind(a) for a in args])
    return out


def _ctypes_kind(t):
    if t is None:
        return "void"
    if t in (ctypes.c_void_p, ctypes.c_char_p) or isinstance(t, type(ctypes.POINTER(ctypes.c_uint))):
        return "ptr"
    return {ctypes.c_int: "int", ctypes.c_int64: "int64", ctypes.c_float: "float", ctypes.c_size_t: "size_t",
            ctypes.c_uint: "unsigned"}[t]


def test_binding_types_are_the_headers():
    """_lib.PROTOTYPES against the header position by position: pointer -> a pointer type, int, int64_t, float, size_t.
    An `int` where the header says `int64_t` would pass every call until a stride exceeds 2^31."""
    from ctc_amd import _lib
    assert ctypes.sizeof(ctypes.c_int64) == 8 and ctypes.c_int64 is not ctypes.c_int      # the kinds below tell them apart
    assert ctypes.c_size_t is not ctypes.c_int and ctypes.c_size_t is not ctypes.c_uint
    header = _header_prototypes()
    assert sorted(header) == _declared() == sorted(_lib.PROTOTYPES) and len(header) >= 59
    wrong = []
    for name, (ret, args) in header.items():
        res, argtypes = _lib.PROTOTYPES[name]
        got = (_ctypes_kind(res), [_ctypes_kind(t) for t in argtypes])
        if got != (ret, args):
            wrong.append((name, "header", (ret, args), "binding", got))
    assert not wrong, wrong
    # the parser tells the kinds apart: spot checks against prototypes read by eye
    assert header["ctc_amd_workspace_bytes"] == ("size_t", ["int"] * 5)
    assert header["ctc_amd_error_string"] == ("ptr", ["int"])
    assert header["ctc_amd_scale_grad"] == ("int", ["ptr", "ptr", "size_t", "ptr"])
    assert header["ctc_amd_noblank_loss_grad"][1][:5] == ["ptr", "int64", "int64", "ptr", "int"]
    assert header["ctc_amd_noblank_loss_grad"][1][11:13] == ["float", "float"]


def test_argument_errors_without_gpu(built):
    from ctc_amd import _lib
    lib = _lib.load()
    # null pointers / bad sizes are rejected before any HIP call
    assert lib.ctc_amd_noblank_loss_grad(None, 0, 0, None, 0, None, None, 1, 1, 1, 1, 1.0, 1.0,
                                         None, None, None, None, None) == -1
    assert lib.ctc_amd_scale_grad(None, None, 4, None) == -1


def test_no_cpu_fallback():
    import ctc_amd
    x = torch.randn(4, 2, 5, requires_grad=True)
    lab = torch.zeros(2, 3, dtype=torch.long)
    with pytest.raises(ctc_amd.CtcAmdError):
        ctc_amd.CTCLoss.apply(x, lab, torch.tensor([4, 4]), torch.tensor([3, 2]))
    with pytest.raises(ctc_amd.CtcAmdError):
        ctc_amd.NoBlankBinaryCTC()(x, torch.zeros(2, 3, 5), torch.tensor([4, 4]), torch.tensor([3, 2]))


def test_product_code_never_imports_oracle():
    for dirpath, _, files in os.walk(os.path.join(ROOT, "ctc_amd")):
        for f in files:
            if f.endswith((".py", ".hip", ".hpp", ".h")):
                txt = open(os.path.join(dirpath, f)).read()
                assert "oracle" not in txt.replace("# oracle", ""), "%s mentions the oracle" % f


def test_variant_selection_and_shape_errors():
    from ctc_amd import functional as F
    assert F._variant_of(torch.zeros(2, 3, dtype=torch.int32)) == 0
    assert F._variant_of(torch.zeros(2, 3, dtype=torch.int64)) == 0
    assert F._variant_of(torch.zeros(2, 3, 5)) == 1
    with pytest.raises(ValueError):
        F._variant_of(torch.zeros(2, 3))
    with pytest.raises(ValueError):
        F._lengths(torch.tensor([4, 9]), 2, "input_lengths", torch.device("cpu"), 8)
    with pytest.raises(ValueError):
        F._lengths(torch.tensor([0, 3]), 2, "target_lengths", torch.device("cpu"), 8)
    with pytest.raises(ValueError):
        F._lengths(torch.tensor([1, 2, 3]), 2, "target_lengths", torch.device("cpu"), 8)
    assert F._lengths([1, 8], 2, "input_lengths", torch.device("cpu"), 8).dtype == torch.int64
