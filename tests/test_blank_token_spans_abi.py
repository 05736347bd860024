"""Blank-CTC token spans (ctc_amd_blank_token_spans): the C ABI (declared, exported, bound, argument errors before any
HIP call), the Python surface, and the numpy restatement of how a path and its per-frame confidences become one record
per label, on hand-written paths with known answers (runs without a GPU).  tests/test_blank_token_spans_gpu.py checks
the kernels against the same restatement."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "ctc_amd_blank_token_spans"
POINTERS = ["lp", "tgt", "il", "tl", "path", "score", "nll", "frame_conf", "start", "end", "conf", "ws"]


def spans_of_path(path, frame_conf, in_len, tgt_len):
    """restatement of the span stage -> (start [B,S'] int32, end [B,S'] int32, conf [B,S'] float32), S' = max(tgt_len, 1)
    columns at least (callers compare the first S columns they have; the rest is -1 / -1 / 0 by the same rule).

    Label j of sample b owns the frames t < T_b with path[b,t] == 2j+1: start = the first, end = one past the last.
    conf = (float32 sum of frame_conf over start..end-1, from 0, ascending t) / float32(end - start), one float32
    division.  Labels the path does not visit: -1, -1, 0."""
    path = np.asarray(path)
    frame_conf = np.asarray(frame_conf, dtype=np.float32)
    B, T = path.shape
    S = max(int(np.max(tgt_len)), (int(path.max()) + 1) // 2, 1)
    start = np.full((B, S), -1, dtype=np.int32)
    end = np.full((B, S), -1, dtype=np.int32)
    conf = np.zeros((B, S), dtype=np.float32)
    for b in range(B):
        Tb, L = int(in_len[b]), int(tgt_len[b])
        if not (0 <= L and 1 <= Tb <= T):
            continue
        for j in range(L):
            own = np.nonzero(path[b, :Tb] == 2 * j + 1)[0]
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


def test_symbol_declared_exported_and_bound(lib):
    from ctc_amd import _lib
    header = open(os.path.join(ROOT, "include", "ctc_amd.h")).read()
    assert re.search(r"\b%s\s*\(" % NAME, header)
    assert hasattr(ctypes.CDLL(_lib.SO_PATH), NAME)
    res, args = _lib.PROTOTYPES[NAME]
    assert res is ctypes.c_int and len(args) == 21
    assert lib.ctc_amd_abi_version() == 2


def _call(lib, ptr=16, T=4, B=2, C=5, S=3, blank=0, **null):
    p = {k: (None if null.get(k) else ptr) for k in POINTERS}
    return lib.ctc_amd_blank_token_spans(p["lp"], 0, 0, p["tgt"], 0, p["il"], p["tl"], T, B, C, S, blank,
                                         p["path"], p["score"], p["nll"], p["frame_conf"], p["start"], p["end"],
                                         p["conf"], p["ws"], None)


@pytest.mark.parametrize("which", POINTERS)
def test_null_pointers(lib, which):
    # rejected before anything is dereferenced or launched: the other pointers are non-null but bogus
    assert _call(lib, **{which: True}) == -1


@pytest.mark.parametrize("kw", [dict(T=0), dict(B=0), dict(C=0), dict(S=0), dict(blank=-1), dict(blank=5),
                                dict(S=1024, T=0), dict(S=1024, lp=True)])
def test_bad_sizes_and_blank(lib, kw):
    # (the last two: a bad argument is reported before S is looked at)
    assert _call(lib, **kw) == -1


def test_too_many_labels(lib):
    assert _call(lib, S=1024) == -2                               # dummy pointers: nothing is launched


def test_python_export():
    import ctc_amd
    assert "blank_token_spans" in ctc_amd.__all__ and callable(ctc_amd.blank_token_spans)
    assert ctc_amd.BlankTokenSpans._fields == ("start", "end", "conf", "frame_conf", "path", "score", "nll")


def test_no_cpu_path():
    import torch
    import ctc_amd
    lp = torch.randn(4, 2, 5).log_softmax(2)
    with pytest.raises(ctc_amd.CtcAmdError):
        ctc_amd.blank_token_spans(lp, torch.ones(2, 3, dtype=torch.int64), torch.tensor([4, 4]), torch.tensor([2, 1]))


# ---- the restatement on paths with known answers ---------------------------------------------------

def _one(path, fc, L, Tb=None):
    path = np.asarray([path], dtype=np.int32)
    fc = np.asarray([fc], dtype=np.float32)
    s, e, c = spans_of_path(path, fc, [path.shape[1] if Tb is None else Tb], [L])
    return list(s[0]), list(e[0]), c[0]


def test_two_labels_with_blanks():
    fc = [0.5, 0.25, 0.75, 1.0, 0.5, 0.125, 0.9]
    s, e, c = _one([0, 1, 1, 2, 3, 3, 4], fc, 2)
    assert s == [1, 4] and e == [3, 6]
    assert c[0] == np.float32(0.5) and c[1] == np.float32(0.3125)


def test_no_blank_frame():
    s, e, c = _one([1, 3, 5], [0.5, 0.25, 1.0], 3)
    assert s == [0, 1, 2] and e == [1, 2, 3]
    assert list(c) == [np.float32(0.5), np.float32(0.25), np.float32(1.0)]


def test_ends_on_the_last_label_without_a_closing_blank():
    s, e, c = _one([0, 1, 2, 3, 3], [1, 1, 1, 0.5, 0.25], 2)
    assert s == [1, 3] and e == [2, 5] and c[1] == np.float32(0.375)


def test_no_labels_and_no_alignment():
    s, e, c = _one([0, 0, 0], [1, 1, 1], 0)
    assert s == [-1] and e == [-1] and c[0] == 0
    s, e, c = _one([-1, -1, -1], [0, 0, 0], 2)
    assert s == [-1, -1] and e == [-1, -1] and (c == 0).all()


def test_short_sample_and_padding_columns():
    # T_b = 4 of 6 frames: what lies behind T_b is not looked at; label columns j >= L stay at -1
    path = np.array([[1, 1, 2, 3, -1, -1], [0, 1, 2, -1, -1, -1]], dtype=np.int32)
    path_dirty = path.copy()
    path_dirty[0, 4:] = 3                                          # (garbage behind T_b must not extend the span)
    fc = np.array([[0.5, 0.25, 1, 0.75, 9, 9], [1, 0.5, 1, 9, 9, 9]], dtype=np.float32)
    for p in (path, path_dirty):
        s, e, c = spans_of_path(p, fc, [4, 3], [2, 1])
        assert s.tolist() == [[0, 3], [1, -1]] and e.tolist() == [[2, 4], [2, -1]]
        assert c.tolist() == [[0.375, 0.75], [0.5, 0.0]]
    assert padded(s, 5, -1).tolist() == [[0, 3, -1, -1, -1], [1, -1, -1, -1, -1]]


def test_sum_order_is_sequential_float32():
    # 1 + 2^-24 + 2^-24 in float32: left to right both small terms are lost, pairwise they are not
    tiny = np.float32(2.0 ** -24)
    s, e, c = _one([1, 1, 1], [1.0, tiny, tiny], 1)
    assert c[0] == np.float32(np.float32(1.0) / np.float32(3.0))
    assert c[0] != np.float32((1.0 + 2.0 ** -23) / 3.0)
