"""Blank-CTC best path (forced alignment): the C ABI (declared, exported, bound, argument errors before any HIP call)
and the float32 numpy restatement of its specification on hand-built lattices with known answers (runs without a
GPU).  tests/test_blank_align_gpu.py checks the kernel against the same restatement."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "ctc_amd_blank_best_path"
NINF = np.float32(-np.inf)


def viterbi_blank(lp, targets, in_len, tgt_len, blank=0):
    """float32 restatement of ctc_amd_blank_best_path -> (path [B,T] int32, score [B] float32).

    One select chain (stay, advance, skip; a later candidate only when strictly greater) and one float32 add per
    state and step, in the kernel's order: scores are bit-identical and paths identical, ties included."""
    lp = np.asarray(lp, dtype=np.float32)
    targets = np.asarray(targets)
    T, B, _ = lp.shape
    path = np.full((B, T), -1, dtype=np.int32)
    score = np.full(B, NINF, dtype=np.float32)
    for b in range(B):
        Tb, L = int(in_len[b]), int(tgt_len[b])
        ext = np.full(2 * L + 1, blank, dtype=np.int64)
        ext[1::2] = targets[b, :L]
        n = ext.size
        em = lp[:Tb, b, ext]                                            # [Tb, n]
        skip = np.zeros(n, dtype=bool)
        for s in range(3, n, 2):
            skip[s] = ext[s] != blank and ext[s] != ext[s - 2]
        v = np.full(n, NINF, dtype=np.float32)
        v[0] = em[0, 0]
        if n > 1:
            v[1] = em[0, 1]
        bp = np.zeros((Tb, n), dtype=np.int8)
        for t in range(1, Tb):
            adv = np.concatenate([[NINF], v[:-1]]).astype(np.float32)
            sk = np.concatenate([[NINF, NINF], v[:-2]])[:n].astype(np.float32)
            best = v.copy()
            code = np.zeros(n, dtype=np.int8)
            m1 = adv > best
            best[m1] = adv[m1]
            code[m1] = 1
            m2 = skip & (sk > best)
            best[m2] = sk[m2]
            code[m2] = 2
            v = (best + em[t]).astype(np.float32)
            bp[t] = code
        s = 0 if L == 0 else (2 * L if v[2 * L] > v[2 * L - 1] else 2 * L - 1)
        score[b] = v[s]
        if not v[s] > NINF:
            continue
        for t in range(Tb - 1, -1, -1):
            path[b, t] = s
            s -= int(bp[t, s])
    return path, score


def tokens_of(path, targets, blank):
    """class of every path state (blank for even, the label for odd states), -1 where path is -1"""
    tok = np.full(path.shape, -1, dtype=np.int64)
    for b in range(path.shape[0]):
        for t in range(path.shape[1]):
            s = int(path[b, t])
            if s >= 0:
                tok[b, t] = blank if s % 2 == 0 else int(targets[b, (s - 1) // 2])
    return tok


def _one(rows, labels, blank=0, Tb=None):
    lp = np.asarray(rows, dtype=np.float32)[:, None, :]
    T = lp.shape[0]
    tg = np.asarray([list(labels) + [0]], dtype=np.int64)
    p, s = viterbi_blank(lp, tg, [T if Tb is None else Tb], [len(labels)], blank)
    return p[0], s[0]


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
    assert res is ctypes.c_int and len(args) == 16
    assert lib.ctc_amd_abi_version() == 2


def _call(lib, ptr=16, T=4, B=2, C=5, S=3, blank=0, **null):
    p = {k: (None if null.get(k) else ptr) for k in ("lp", "tgt", "il", "tl", "path", "score", "ws")}
    return lib.ctc_amd_blank_best_path(p["lp"], 0, 0, p["tgt"], 0, p["il"], p["tl"], T, B, C, S, blank,
                                       p["path"], p["score"], p["ws"], None)


@pytest.mark.parametrize("which", ["lp", "tgt", "il", "tl", "path", "score", "ws"])
def test_null_pointers(lib, which):
    # rejected before anything is dereferenced or launched: the other pointers are non-null but bogus
    assert _call(lib, **{which: True}) == -1


@pytest.mark.parametrize("kw", [dict(T=0), dict(B=0), dict(C=0), dict(S=0), dict(T=-3), dict(blank=-1),
                                dict(blank=5), dict(C=5, blank=7)])
def test_bad_sizes_and_blank(lib, kw):
    assert _call(lib, **kw) == -1


@pytest.mark.parametrize("S", [256, 300])
def test_too_many_labels(lib, S):
    assert _call(lib, S=S) == -2


# ---- the restatement on lattices with known answers ------------------------------------------------

def test_single_label_known_path():
    # label 1, blank 0: the best path is blank, 1, 1, blank
    rows = [[-0.5, -2.0], [-3.0, -0.25], [-4.0, -0.5], [-0.125, -3.0]]
    p, s = _one(rows, [1])
    assert list(p) == [0, 1, 1, 2]
    assert s == np.float32(-0.5) + np.float32(-0.25) + np.float32(-0.5) + np.float32(-0.125)


def test_tie_at_a_step_keeps_the_earlier_candidate():
    # step 1 into state 1: stay (v0(1) = -1) and advance (v0(0) = -1) tie -> stay (the earlier candidate)
    rows = [[-1.0, -1.0], [-9.0, -1.0]]
    p, s = _one(rows, [1])
    assert list(p) == [1, 1] and s == np.float32(-2.0)


def test_tie_advance_against_skip():
    # labels 1, 2 (skip allowed into state 3): first the skip alone, then advance and skip tied -- advance comes
    # first and a tie does not replace it
    rows = [[-1.0, -1.0, -9.0], [-9.0, -9.0, -1.0]]
    # v0 = [-1, -1, -inf, -inf, -inf]; t = 1 state 3: stay -inf, advance v0(2) = -inf, skip v0(1) = -1 -> skip
    p, s = _one(rows, [1, 2])
    assert list(p) == [1, 3] and s == np.float32(-2.0)
    # now make advance equal to skip: v(2) = v(1) at t = 1, read at t = 2
    rows = [[-1.0, -1.0, -9.0], [-1.0, -1.0, -9.0], [-9.0, -9.0, -1.0]]
    p, s = _one(rows, [1, 2])
    # t = 1: v(1) = max(stay -1, adv -1) - 1 = -2 (stay), v(2) = max(stay -inf, adv v0(1) = -1) - 1 = -2
    # t = 2 state 3: stay -inf... advance v1(2) = -2 and skip v1(1) = -2 tie -> advance (code 1)
    assert list(p) == [1, 2, 3] and s == np.float32(-3.0)


def test_tie_at_the_end_takes_the_last_label():
    # v(2L) == v(2L-1): the final state is 2L - 1
    rows = [[-1.0, -1.0], [-1.0, -1.0]]
    p, s = _one(rows, [1])
    assert p[-1] == 1 and s == np.float32(-2.0)
    rows = [[-1.0, -1.0], [-0.5, -1.0]]
    p, s = _one(rows, [1])
    assert p[-1] == 2 and list(p) == [1, 2] and s == np.float32(-1.5)


def test_adjacent_repeat_forbids_the_skip():
    # labels 1, 1: state 3 may not come from state 1; three frames are the minimum (1, blank, 1)
    rows = [[-9.0, -0.5], [-0.25, -9.0], [-9.0, -0.5]]
    p, s = _one(rows, [1, 1])
    assert list(p) == [1, 2, 3] and s == np.float32(-1.25)
    # two frames are too short for 1, 1
    p, s = _one(rows[:2], [1, 1])
    assert s == NINF and list(p) == [-1, -1]
    # labels 1, 2 in two frames: the skip is allowed
    p, s = _one([[-9.0, -0.5, -9.0], [-9.0, -9.0, -0.25]], [1, 2])
    assert list(p) == [1, 3] and s == np.float32(-0.75)


def test_no_labels():
    rows = [[-0.5, -1.0], [-0.25, -2.0], [-1.0, -0.1]]
    p, s = _one(rows, [])
    assert list(p) == [0, 0, 0] and s == np.float32(-1.75)


def test_exactly_long_enough_and_one_step_short():
    # labels 1, 1, 2: minimum length L + repeats = 4 frames
    rows = np.full((5, 3), -1.0, dtype=np.float32)
    p, s = _one(rows, [1, 1, 2], Tb=4)
    assert s == np.float32(-4.0) and list(p[:4]) == [1, 2, 3, 5] and p[4] == -1
    p, s = _one(rows, [1, 1, 2], Tb=3)
    assert s == NINF and list(p) == [-1] * 5


def test_blank_is_the_last_class():
    C = 4
    rows = [[-3.0, -3.0, -3.0, -0.25], [-0.5, -3.0, -3.0, -3.0], [-3.0, -3.0, -3.0, -0.125]]
    p, s = _one(rows, [0], blank=C - 1)
    # tokens 3 (blank), 0, 3 -> states 0, 1, 2; label 0 == class 0 is no blank here
    assert list(p) == [0, 1, 2] and s == np.float32(-0.25) + np.float32(-0.5) + np.float32(-0.125)
    tok = tokens_of(p[None, :], np.array([[0]]), C - 1)
    assert list(tok[0]) == [3, 0, 3]


def test_score_is_the_sequential_sum_along_the_path():
    rng = np.random.default_rng(0)
    T, B, C, S = 40, 6, 7, 5
    lp = (rng.standard_normal((T, B, C)) - 2).astype(np.float32)
    tg = rng.integers(1, C, (B, S))
    il = rng.integers(15, T + 1, B)
    tl = rng.integers(0, S + 1, B)
    path, score = viterbi_blank(lp, tg, il, tl, 0)
    tok = tokens_of(path, tg, 0)
    for b in range(B):
        acc = np.float32(0)
        for t in range(int(il[b])):
            acc = np.float32(acc + lp[t, b, tok[b, t]])
        assert acc == score[b] or (score[b] == NINF and (tok[b] == -1).all())
        steps = np.diff(path[b, :il[b]])
        assert ((steps >= 0) & (steps <= 2)).all()
