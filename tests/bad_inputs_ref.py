"""Lengths and labels OUTSIDE their range on every lattice kernel: the cases, the buffers they run in and what the
library must answer -- shared by tests/test_bad_inputs_ref.py (no GPU) and tests/test_bad_inputs_gpu.py (the kernels).

The Python layer hands device-resident lengths to the kernels unchecked (ctc_amd.functional._lengths: a check would cost
a synchronisation) and never looks at labels, so a dataset bug arrives in the kernels as it is.  Every kernel carries a
guard of its own; include/ctc_amd.h states what the guards add up to (Conventions, "Lengths and labels outside their
range").  The cases here put such values into batches of the existing path tables -- the shapes of
tests/lattice_inputs_ref.py (no-blank, binary) and tests/blank_grad_ref.py (blank), unchanged, so that the plan tests
keep proving which kernel each shape reaches.

A case is (family, path, composition).  The tables' batches are small (B = 2 .. 6, and 520 for the persistent form), so
one batch cannot hold bad samples at 0, B-1 and in the middle, an adjacent pair AND good samples: every shape with
B <= 6 runs as TWO compositions, the ends (0, B-1, and 1 where B >= 5) and the middle (B//2 and a neighbour where B >= 4);
tests/test_bad_inputs_ref.py asserts what the two hold together.  r16_ps (B = 520) runs once, bad at 0, 1, 255, 256, 257,
519 and at every b % 13 == 5.

A sample is turned bad through its LENGTHS (one kind of BAD_LENGTHS per sample, cycling; a case's cycle starts where
the family's previous case stopped) or, a good sample only, through LABELS inside L_b: values in [-C, -1] and [C, 2C), and
2^32 + k in an int64 tensor.  The TWIN of a case is the same batch with every bad-length sample replaced by the in-range
pair without an alignment (T_b = 1, L_b = 2; blank: with two different labels): good samples must come out of both
launches with the same bits.

Memory safety never rests on a guard: unguarded_extents() walks the addresses a kernel WITHOUT any guard would touch --
the ABI's index formulas with t < max T_b, l < max L_b and the raw label, label mod C or the label's low word as the
class -- and every one of them lies inside the test's own allocations (layout()): x is the centre of a larger tensor with
finite canary logits around it, every other array is followed by a canary tail.  Values beyond 32 bits alias, in their
low word, to a valid length or class."""
import functools

import numpy as np
import torch

from tests import blank_grad_ref as bg
from tests import lattice_inputs_ref as li
from tests.helpers import np_, synth_blank
from tests.test_blank_align_abi import viterbi_blank
from tests.test_blank_posteriors_abi import class_occupancy, posteriors_blank

T_MARGIN, S_MARGIN = 8, 4               # how far beyond the tensor a bad length reaches; the buffers' margins
LOGIT_CANARY, LOGPROB_CANARY = 40.0, 0.0    # around x: either would dominate (or visibly change) any row that read it
HI = 1 << 32
FAMILIES = ("noblank", "binary", "blank")
SHAPES = {"noblank": li.NOBLANK_SHAPES, "binary": li.BINARY_SHAPES, "blank": bg.SHAPES}

# ---- the kinds of bad lengths: name -> (T, S, tb, l) -> (T_b, L_b), (tb, l) the sample's valid pair -------------------
_COMMON = [
    ("T=0", lambda T, S, tb, l: (0, max(l, 1))),
    ("T=-1", lambda T, S, tb, l: (-1, l)),
    ("T=T+1", lambda T, S, tb, l: (T + 1, l)),
    ("T=T+8", lambda T, S, tb, l: (T + T_MARGIN, l)),
    ("L=-1", lambda T, S, tb, l: (tb, -1)),
    ("L=S+1", lambda T, S, tb, l: (tb, S + 1)),
    ("L=S+4", lambda T, S, tb, l: (tb, S + S_MARGIN)),
    ("both beyond", lambda T, S, tb, l: (T + T_MARGIN, S + S_MARGIN)),
    ("infeasible", lambda T, S, tb, l: (1, 2)),
    # beyond 32 bits, the low word a valid length (a guard that compares after truncating would let them through)
    ("T=2^32+3", lambda T, S, tb, l: (HI + 3, min(l, 3))),
    ("T=-2^32+3", lambda T, S, tb, l: (-HI + 3, min(l, 3))),
    ("T=2^40+T_b", lambda T, S, tb, l: ((1 << 40) + tb, l)),
    ("L=2^32+3", lambda T, S, tb, l: (max(tb, 3), HI + 3)),
    ("L=-2^32+3", lambda T, S, tb, l: (max(tb, 3), -HI + 3)),
    ("L=2^40+L_b", lambda T, S, tb, l: (tb, (1 << 40) + l)),
]
BAD_LENGTHS = {
    # L_b = 0 is out of range without a blank ...
    "noblank": _COMMON + [("L=0", lambda T, S, tb, l: (tb, 0)), ("both below", lambda T, S, tb, l: (-1, 0))],
    # (the binary table holds sixteen bad samples in all, one per kind: both-at-once is "both beyond" there)
    "binary": _COMMON + [("L=0", lambda T, S, tb, l: (tb, 0))],
    # ... and valid with one
    "blank": _COMMON + [("both below", lambda T, S, tb, l: (-1, -1))],
}
INFEASIBLE = (1, 2)                      # the twin's pair: in range, no alignment


def in_range(family, T, S, tb, l):
    """each length inside its tensor (include/ctc_amd.h): 1 <= T_b <= T, 1 <= L_b <= S (blank: 0 <= L_b)"""
    return (0 if family == "blank" else 1) <= l <= S and 1 <= tb <= T


def valid_pair(family, T, S, tb, l):
    """in range, and not too short by the lengths alone"""
    return in_range(family, T, S, tb, l) and tb >= l


def low_word(v):
    """what a 32-bit load of the low half of a little-endian int64 gives (load_label; a truncating guard)"""
    v = np.asarray(v, np.int64)
    return ((v & 0xFFFFFFFF) ^ 0x80000000) - 0x80000000


def effective_classes(family, tg, C):
    """the class every label is read as: its low word, then modulo C (no-blank: Python's modulo, negative ones wrap) or
    clamped to [0, C-1] (blank: a clamp to 0 is a label equal to the blank)"""
    k = low_word(tg)
    return k % C if family == "noblank" else np.clip(k, 0, C - 1)


# ---- which samples are bad ---------------------------------------------------------------------------------------------
def compositions(B):
    """-> the bad-length samples of each composition of a batch of B"""
    if B > 64:
        return [sorted({0, 1, 255, 256, 257, B - 1} | {b for b in range(B) if b % 13 == 5})]
    ends = {0, B - 1} | ({1} if B >= 5 else set())
    middle = {B // 2} | ({B // 2 + 1} if B >= 5 else {B // 2 - 1} if B == 4 else set())
    if B == 2:
        ends, middle = {0}, {1}
    return [sorted(ends), sorted(middle)]


CASES = [(f, p, c) for f in FAMILIES for p in SHAPES[f] for c in range(len(compositions(SHAPES[f][p][1])))]


def case_id(case):
    return "%s-%s-%s" % (case[0], case[1], "ab"[case[2]])


def _bad_label_values(C, n, int64, rot):
    """n values outside [0, C), cycling through both ranges (and beyond 32 bits where the tensor can hold it) from the
    rot-th on"""
    out = []
    for j in range(rot, rot + n):
        ring = [-1, C, -C, 2 * C - 1, -1 - (j % C), C + (j % C)] + ([HI + (j % C)] if int64 else [])
        out.append(ring[j % len(ring)])
    return out


@functools.lru_cache(maxsize=None)
def make_case(family, path, comp):
    """-> dict: T, B, C, S; x [T,B,C] float32 (blank: log-probs); tg -- labels [B,S] (int32 or int64: `lab64`) or rows
    [B,S,C] float32; Tb, L the lengths as the launch gets them and Tb_twin, L_twin the twin's (int64 numpy); valid = the
    pairs before anything was turned bad; bad [B] (lengths), badlab [B] (labels), kind [B] (names of BAD_LENGTHS or None)"""
    T, B, C, S = SHAPES[family][path]
    index = list(SHAPES[family]).index(path)
    bad = np.zeros(B, bool)
    bad[compositions(B)[comp]] = True
    lab64 = B > 64 or (index + comp) % 2 == 0
    if family == "blank":
        lp, tg, Tb, L = synth_blank(T + B + C + S, T, B, C, S, var_T=True)      # unit-scale randn, log_softmax
        bg._force_lengths(tg, Tb, L, T)
        x = lp
        for b in np.nonzero(bad)[0]:                        # the twin's (1, 2) needs two different labels
            if int(tg[b, 1]) == int(tg[b, 0]):
                tg[b, 1] = int(tg[b, 0]) % (C - 1) + 1
        tg = tg.long() if lab64 else tg.int()
    else:
        g = torch.Generator().manual_seed(7 * T + 5 * B + 3 * C + S + (0 if family == "noblank" else 1000))
        Tb, L = li._lengths(T, B, S, g)                     # ragged; sample 0 full, the last one with a choice
        x = torch.randn(T, B, C, generator=g)               # unit scale
        if family == "noblank":
            tg = torch.randint(0, C, (B, S), generator=g, dtype=torch.int32)
            tg[torch.arange(S)[None, :] >= L[:, None]] = -1
            tg = tg.long() if lab64 else tg
        else:
            tg = (torch.rand(B, S, C, generator=g) < 0.2).float()
            tg[torch.arange(S)[None, :] >= L[:, None]] = 0.0
    valid = (np_(Tb).astype(np.int64).copy(), np_(L).astype(np.int64).copy())
    Tb, L = valid[0].copy(), valid[1].copy()
    kinds = BAD_LENGTHS[family]
    kind = [None] * B
    first = sum(len(k) for p in list(SHAPES[family])[:index] for k in compositions(SHAPES[family][p][1])) + \
        sum(len(k) for k in compositions(B)[:comp])          # bad samples of the family's earlier cases: the cycle goes on
    for i, b in enumerate(np.nonzero(bad)[0]):
        name, f = kinds[(first + i) % len(kinds)]
        Tb[b], L[b] = f(T, S, int(valid[0][b]), int(valid[1][b]))
        kind[b] = name
    Tb_twin, L_twin = Tb.copy(), L.copy()
    Tb_twin[bad], L_twin[bad] = INFEASIBLE
    badlab = np.zeros(B, bool)
    if family != "binary":
        tg = tg.clone()
        good = np.nonzero(~bad)[0]
        for r, b in enumerate(good):
            l = int(L[b])
            if (r + comp) % 2 == 1 and l >= 1:
                # (blank: three of them -- a clamped label may repeat its neighbour, and every repeat costs a full-length
                # sample a frame it does not have)
                pos = sorted({0, l // 2, l - 1} if family == "blank" else {0, l - 1} | set(range(1, l, 3)))
                for j, v in zip(pos, _bad_label_values(C, len(pos), lab64, 2 * (index + comp) + r)):
                    tg[b, j] = v
                badlab[b] = True
    for a in (Tb, L, Tb_twin, L_twin, bad, badlab) + valid:
        a.setflags(write=False)
    return {"family": family, "path": path, "comp": comp, "T": T, "B": B, "C": C, "S": S, "x": x, "tg": tg, "lab64": lab64,
            "Tb": Tb, "L": L, "Tb_twin": Tb_twin, "L_twin": L_twin, "valid": valid, "bad": bad, "badlab": badlab,
            "kind": kind}


# ---- the buffers ---------------------------------------------------------------------------------------------------------
def states(family, S):
    """last dimension of gamma"""
    return 2 * S + 1 if family == "blank" else S


def layout(family, T, B, C, S):
    """name -> (elements the ABI takes, elements of the canary tail behind them).  x is different: the ABI's tensor is
    X[:T, :B, C:2C] of X [T + 8, B + 1, 3C] ("X": all of it, no tail)."""
    NS = states(family, S)
    NSX = states(family, S + S_MARGIN)                       # the states of a sample with L_b = S + 4
    out = {
        "X": ((T + T_MARGIN) * (B + 1) * 3 * C, 0),
        "in_len": (B, 8), "tgt_len": (B, 8),
        "nll": (B, 8), "loss": (1, 8), "score": (B, 8),
        "grad": (T * B * C, T_MARGIN * B * C),
        "gamma": (B * T * NS, T_MARGIN * NS + NSX),
        "path": (B * T, T_MARGIN), "frame_conf": (B * T, T_MARGIN),
        "start": (B * S, S_MARGIN), "end": (B * S, S_MARGIN), "conf": (B * S, S_MARGIN),
    }
    if family == "binary":
        out["y"] = (B * S * C, S_MARGIN * C)                 # zeros
    else:
        out["labels"] = (B * S, S_MARGIN)                    # valid classes
    return out


def x_strides(B, C):
    """(offset of x[0,0,0] in X, stride_t, stride_b) in elements"""
    return C, (B + 1) * 3 * C, 3 * C


def label_tail(C):
    return [(3 * j + 1) % C for j in range(S_MARGIN)]


def unguarded_extents(case):
    """name -> (lowest, highest) flat element index a kernel WITHOUT any guard would touch in that buffer: the ABI's index
    formulas with t < max T_b and l < max L_b over the batch (lengths as a 32-bit kernel variable holds them: the low
    word), and for x the class = the raw label, label mod C or the label's low word.  Also -> the problems found on the
    way (a value beyond 32 bits whose low word is not valid)."""
    f, T, B, C, S = (case[k] for k in ("family", "T", "B", "C", "S"))
    problems = []
    tmax, lmax = T, S
    for which in ("", "_twin"):
        for b in range(B):
            tb, l = int(case["Tb" + which][b]), int(case["L" + which][b])
            tw, lw = int(low_word(tb)), int(low_word(l))
            if (tw, lw) != (tb, l) and not valid_pair(f, T, S, tw, lw):
                problems.append("sample %d: (%d, %d) aliases to (%d, %d), not a valid pair" % (b, tb, l, tw, lw))
            tmax, lmax = max(tmax, tw), max(lmax, lw)
    NS, nsmax = states(f, S), states(f, lmax)
    off, st, sb = x_strides(B, C)
    ext = {
        "in_len": (0, B - 1), "tgt_len": (0, B - 1), "nll": (0, B - 1), "loss": (0, 0), "score": (0, B - 1),
        "grad": (0, ((tmax - 1) * B + B - 1) * C + C - 1),
        "gamma": (0, ((B - 1) * T + tmax - 1) * NS + nsmax - 1),
        "path": (0, (B - 1) * T + tmax - 1), "frame_conf": (0, (B - 1) * T + tmax - 1),
        "start": (0, (B - 1) * S + lmax - 1), "end": (0, (B - 1) * S + lmax - 1), "conf": (0, (B - 1) * S + lmax - 1),
    }
    cls_lo, cls_hi = 0, C - 1                                # the rows' own columns (softmax, BCE)
    if f == "binary":
        ext["y"] = (0, ((B - 1) * S + lmax - 1) * C + C - 1)
    else:
        ext["labels"] = (0, (B - 1) * S + lmax - 1)
        every = np.concatenate([np_(case["tg"]).astype(np.int64).reshape(-1), np.asarray(label_tail(C), np.int64)])
        for v in every[: ext["labels"][1] + 1]:
            v, w = int(v), int(low_word(v))
            if v != w:                                       # beyond 32 bits: only its low word is ever read
                if not 0 <= w < C:
                    problems.append("label %d aliases to %d, not a class" % (v, w))
                cands = [w]
            else:
                cands = [v, v % C]
            cls_lo, cls_hi = min([cls_lo] + cands), max([cls_hi] + cands)
    ext["X"] = (off + cls_lo, off + (tmax - 1) * st + (B - 1) * sb + cls_hi)
    return ext, problems


# ---- what the library must answer -------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def expected(family, path, comp):
    """float64 on the TWIN batch (every bad-length sample is (1, 2) there: no alignment) with the labels as the kernels read
    them -> dict(nll [B] (+inf without an alignment), grad [T,B,C] of the batch-mean loss, gamma [B,T,states], path [B,T],
    score [B], fin [B]); blank: path and score from the float32 restatement (bit for bit the kernel's)."""
    c = make_case(family, path, comp)
    T, B, C, S = (c[k] for k in "TBCS")
    Tb, L = c["Tb_twin"], c["L_twin"]
    if family != "blank":
        tg = c["tg"] if family == "binary" else effective_classes(family, np_(c["tg"]), C)
        r = li.lattice_ref(family, c["x"], tg, Tb, L)
        out = {k: r[k] for k in ("nll", "grad", "gamma", "path", "score", "fin")}
    else:
        lp, tg = np_(c["x"]).astype(np.float64), effective_classes(family, np_(c["tg"]), C)
        gamma, nll = posteriors_blank(lp, tg, Tb, L, 0)
        fin = np.isfinite(nll)
        occ = class_occupancy(gamma, tg, Tb, L, C, 0)
        grad = np.zeros((T, B, C))
        for b in np.nonzero(fin)[0]:
            tb = int(Tb[b])
            grad[:tb, b] = (np.exp(lp[:tb, b]) - occ[:tb, b]) / (max(int(L[b]), 1) * B)
        path_, score = viterbi_blank(np_(c["x"]), tg, Tb, L, 0)
        out = {"nll": nll, "grad": grad, "gamma": gamma, "path": path_, "score": score, "fin": fin}
    for v in out.values():
        v.setflags(write=False)
    return out
