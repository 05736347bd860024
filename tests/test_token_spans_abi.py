"""Token spans on the no-blank and the binary lattice (ctc_amd_noblank_token_spans, ctc_amd_binary_token_spans): the
C ABI (declared, exported, bound, argument errors before any HIP call), the Python surface, and the numpy restatement of
how a path and its per-frame confidences become one record per label, on hand-written paths with known answers (runs
without a GPU).  tests/test_token_spans_gpu.py checks the kernels against the same restatement."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUTPUTS = ["path", "score", "nll", "frame_conf", "start", "end", "conf"]
# (entry, its pointer arguments in order of appearance -- the ignored workspace is not among them --, number of arguments)
ENTRIES = {
    "noblank": ("ctc_amd_noblank_token_spans", ["x", "labels", "il", "tl"] + OUTPUTS, 20),
    "binary": ("ctc_amd_binary_token_spans", ["x", "y", "il", "tl"] + OUTPUTS, 19),
}


def spans_of_path(path, frame_conf, in_len, tgt_len):
    """restatement of the span stage on this lattice -> (start [B,S'] int32, end [B,S'] int32, conf [B,S'] float32),
    S' = max(tgt_len, 1) columns at least (callers compare the first S columns they have; the rest is -1 / -1 / 0 by the
    same rule).

    Label j of sample b owns the frames t < T_b with path[b,t] == j: start = the first, end = one past the last.
    conf = (float32 sum of frame_conf over start..end-1, from 0, ascending t) / float32(end - start), one float32
    division.  Labels the path does not visit: -1, -1, 0."""
    path = np.asarray(path)
    frame_conf = np.asarray(frame_conf, dtype=np.float32)
    B, T = path.shape
    S = max(int(np.max(tgt_len)), 1)
    start = np.full((B, S), -1, dtype=np.int32)
    end = np.full((B, S), -1, dtype=np.int32)
    conf = np.zeros((B, S), dtype=np.float32)
    for b in range(B):
        Tb, L = int(in_len[b]), int(tgt_len[b])
        if not (1 <= L <= Tb <= T):
            continue
        for j in range(L):
            own = np.nonzero(path[b, :Tb] == j)[0]
            if own.size == 0:
                continue
            t0, t1 = int(own[0]), int(own[-1]) + 1
            assert t1 - t0 == own.size, "a label's frames are contiguous on a monotone path"
            acc = np.float32(0.0)
            for t in range(t0, t1):
                acc = np.float32(acc + frame_conf[b, t])
            start[b, j], end[b, j] = t0, t1
            conf[b, j] = np.float32(acc / np.float32(t1 - t0))
    return start, end, conf


def padded(a, S, fill):
    """the restatement's columns as an [B,S] array (it returns as many as it needs; the rest is `fill`)"""
    out = np.full((a.shape[0], S), fill, dtype=a.dtype)
    n = min(S, a.shape[1])
    out[:, :n] = a[:, :n]
    assert (a[:, n:] == fill).all()
    return out


# ---- ABI ---------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    from ctc_amd import _lib, build
    build.build()
    return _lib.load()


@pytest.mark.parametrize("family", list(ENTRIES))
def test_symbol_declared_exported_and_bound(lib, family):
    from ctc_amd import _lib
    name, _, nargs = ENTRIES[family]
    header = open(os.path.join(ROOT, "include", "ctc_amd.h")).read()
    assert re.search(r"\b%s\s*\(" % name, header)
    assert hasattr(ctypes.CDLL(_lib.SO_PATH), name)
    res, args = _lib.PROTOTYPES[name]
    assert res is ctypes.c_int and len(args) == nargs
    assert lib.ctc_amd_abi_version() == 2 and _lib.ABI_VERSION == 2
    assert re.search(r"#define\s+CTC_AMD_ABI_VERSION\s+2\b", header)


def _call(lib, family, ptr=16, T=4, B=2, C=5, S=3, ws=None, **null):
    name, pointers, _ = ENTRIES[family]
    p = {k: (None if null.get(k) else ptr) for k in pointers}
    lab = (p["labels"], 0) if family == "noblank" else (p["y"],)
    return getattr(lib, name)(p["x"], 0, 0, *lab, p["il"], p["tl"], T, B, C, S, *(p[k] for k in OUTPUTS), ws, None)


@pytest.mark.parametrize("family,which", [(f, w) for f in ENTRIES for w in ENTRIES[f][1]])
def test_null_pointers(lib, family, which):
    # rejected before anything is dereferenced or launched: the other pointers are non-null but bogus
    assert _call(lib, family, **{which: True}) == -1


@pytest.mark.parametrize("family", list(ENTRIES))
@pytest.mark.parametrize("kw", [dict(T=0), dict(B=0), dict(C=0), dict(S=0), dict(S=257, T=0), dict(S=257, x=True)])
def test_bad_sizes(lib, family, kw):
    # (the last two: a bad argument is reported before S is looked at)
    assert _call(lib, family, **kw) == -1


@pytest.mark.parametrize("family", list(ENTRIES))
def test_too_many_labels(lib, family):
    assert _call(lib, family, S=257) == -2                       # dummy pointers: nothing is launched
    assert _call(lib, family, S=257, ws=16) == -2                # (the workspace is ignored: NULL or not)


@pytest.mark.parametrize("family", list(ENTRIES))
def test_lattice_beyond_lds(lib, family):
    # 600 x 64 cells are 192 KB at the best path's own 5 bytes per cell: refused before any launch
    assert _call(lib, family, T=600, B=1, C=8, S=64) == -2


def test_python_export():
    import ctc_amd
    for name in ("noblank_token_spans", "binary_token_spans", "TokenSpans"):
        assert name in ctc_amd.__all__ and hasattr(ctc_amd, name)
    assert callable(ctc_amd.noblank_token_spans) and callable(ctc_amd.binary_token_spans)
    assert ctc_amd.TokenSpans._fields == ("start", "end", "conf", "frame_conf", "path", "score", "nll")


def test_no_cpu_path():
    import torch
    import ctc_amd
    x = torch.randn(4, 2, 5)
    with pytest.raises(ctc_amd.CtcAmdError):
        ctc_amd.noblank_token_spans(x, torch.ones(2, 3, dtype=torch.int64), torch.tensor([4, 4]), torch.tensor([2, 1]))
    with pytest.raises(ctc_amd.CtcAmdError):
        ctc_amd.binary_token_spans(x, torch.ones(2, 3, 5), torch.tensor([4, 4]), torch.tensor([2, 1]))


# ---- the restatement on paths with known answers ---------------------------------------------------

def _one(path, fc, L, Tb=None):
    path = np.asarray([path], dtype=np.int32)
    fc = np.asarray([fc], dtype=np.float32)
    s, e, c = spans_of_path(path, fc, [path.shape[1] if Tb is None else Tb], [L])
    return list(s[0]), list(e[0]), c[0]


def test_partition():
    fc = [0.5, 0.25, 0.75, 1.0, 0.5, 0.125, 0.875]
    s, e, c = _one([0, 0, 1, 2, 2, 2, 3], fc, 4)
    assert s == [0, 2, 3, 6] and e == [2, 3, 6, 7]
    assert s[0] == 0 and e[:-1] == s[1:] and e[-1] == 7          # the spans partition [0, T_b)
    assert list(c) == [np.float32(0.375), np.float32(0.75), np.float32(1.625 / 3.0), np.float32(0.875)]


def test_one_frame_per_label():
    s, e, c = _one([0, 1, 2], [0.5, 0.25, 1.0], 3)
    assert s == [0, 1, 2] and e == [1, 2, 3]
    assert list(c) == [np.float32(0.5), np.float32(0.25), np.float32(1.0)]


def test_short_sample_and_padding_columns():
    # T_b = 4 of 6 frames: what lies behind T_b is not looked at; label columns j >= L stay at -1
    path = np.array([[0, 0, 1, 1, -1, -1], [0, 0, 0, -1, -1, -1]], dtype=np.int32)
    path_dirty = path.copy()
    path_dirty[0, 4:] = 1                                          # (garbage behind T_b must not extend the span)
    path_dirty[1, 3:] = 0
    fc = np.array([[0.5, 0.25, 1, 0.75, 9, 9], [1, 0.5, 0.75, 9, 9, 9]], dtype=np.float32)
    for p in (path, path_dirty):
        s, e, c = spans_of_path(p, fc, [4, 3], [2, 1])
        assert s.tolist() == [[0, 2], [0, -1]] and e.tolist() == [[2, 4], [3, -1]]
        assert c.tolist() == [[0.375, 0.875], [0.75, 0.0]]
    assert padded(s, 5, -1).tolist() == [[0, 2, -1, -1, -1], [0, -1, -1, -1, -1]]
    assert padded(c, 5, 0).tolist() == [[0.375, 0.875, 0, 0, 0], [0.75, 0, 0, 0, 0]]


def test_no_alignment():
    s, e, c = _one([-1, -1, -1], [0, 0, 0], 2)
    assert s == [-1, -1] and e == [-1, -1] and (c == 0).all()
    # L_b > T_b: no alignment whatever the path array holds
    s, e, c = spans_of_path(np.array([[0, 1, 1]]), np.ones((1, 3), np.float32), [2], [4])
    assert (s == -1).all() and (e == -1).all() and (c == 0).all() and s.shape == (1, 4)


def test_sum_order_is_sequential_float32():
    # 1 + 2^-24 + 2^-24 in float32: left to right both small terms are lost, pairwise they are not
    tiny = np.float32(2.0 ** -24)
    s, e, c = _one([0, 0, 0], [1.0, tiny, tiny], 1)
    assert c[0] == np.float32(np.float32(1.0) / np.float32(3.0))
    assert c[0] != np.float32((1.0 + 2.0 ** -23) / 3.0)
