"""The answers of every producer entry and scratch query of libctc_amd.so to calls that its checks refuse (no GPU needed).

    CTC_AMD_LIB=/path/to/other/libctc_amd.so python tools/producer_abi_grid.py --out old.txt
    python tools/producer_abi_grid.py --out new.txt
    python tools/producer_abi_grid.py --compare old.txt new.txt [--allow REGEX]...

For comparing the host code of two builds: every pointer is a bogus host address, every call carries at least one thing an entry
refuses (a NULL pointer, a size <= 0 or beyond a documented bound, a pitch below the width, a misaligned operand, a scratch one
byte short, an incomplete pair of statistics, an unknown dtype code), alone and paired with every other variation, over several
valid shapes, both modes and all three feat dtypes.  One line per call: entry, what was varied, the return code.  The process
hides every GPU from the HIP runtime before it loads the library, so a call that did get past the checks fails in the launch
and is reported ("not refused"), never run.  --compare prints the lines that differ; --allow accepts the differing lines that
match REGEX (a deliberate change of an answer) and lists them by entry and answers."""
import argparse
import itertools
import os
import re
import sys

for _v in ("HIP_VISIBLE_DEVICES", "ROCR_VISIBLE_DEVICES"):
    os.environ[_v] = "-1"                                    # no device: nothing this tool calls may launch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

P, BIG = 4096, 1 << 30
ROWS = 1 << 22                                               # the documented bound on T B


def _p(a, k):
    return a.get(k, P)


def head_forward(lib, name, a):
    T, B, K, C = a["T"], a["B"], a["K"], a["C"]
    fsb = a.get("fsb", K)
    rm, rv = (a.get("rm", P), a.get("rv", P)) if a["mode"] == "eval" else (a.get("rm"), a.get("rv"))
    args = [_p(a, "feat"), a.get("fst", B * fsb), fsb, _p(a, "weight"), _p(a, "bias"), _p(a, "bn_weight"), _p(a, "bn_bias"), rm, rv,
            1e-5]
    if "lstm_forward" in name:
        cols = a.get("cols", C)
        args += [_p(a, k) for k in ("h0", "c0", "w_ih", "w_hh", "b_ih", "b_hh")]
        args += [T, B, K, C, _p(a, "out"), B * cols, a.get("out_sb", cols), cols, 0.0, None, None]
    else:
        osb = a.get("out_sb", C)
        args += [None, T, B, K, C, _p(a, "out"), B * osb, osb, P, P, P, P]
        if "wide" in name:
            args += [_p(a, "scratch"), _scratch(lib, "ctc_amd_head_forward_wide_scratch_bytes", a, T, B, K, C)]
    return _call(lib, name, a, args, 0)


def head_backward(lib, name, a):
    T, B, K, C = a["T"], a["B"], a["K"], a["C"]
    fsb, dsb, gsb = a.get("fsb", K), a.get("dout_sb", C), a.get("dfeat_sb", K)
    train = a["mode"] == "train"
    sm, si = (a.get("smean", P), a.get("sinv", P)) if train else (a.get("smean"), a.get("sinv"))
    rm, rv = (a.get("rm"), a.get("rv")) if train else (a.get("rm", P), a.get("rv", P))
    query = "ctc_amd_head_backward%s_scratch_bytes" % ("_wide" if "wide" in name else "")
    args = [_p(a, "d_out"), B * dsb, dsb, _p(a, "feat"), a.get("fst", B * fsb), fsb, _p(a, "weight"), _p(a, "bn_weight"),
            _p(a, "bn_bias"), _p(a, "linear_out"), sm, si, rm, rv, 1e-5, None, T, B, K, C, _p(a, "d_feat"), B * gsb, gsb,
            _p(a, "d_weight"), _p(a, "d_bias"), _p(a, "d_bn_weight"), _p(a, "d_bn_bias"), _p(a, "scratch"),
            _scratch(lib, query, a, T, B, K, C)]
    return _call(lib, name, a, args, 3)


def series(lib, name, a):
    T, B, I, H = a["T"], a["B"], a["I"], a["H"]
    cols = a.get("cols", H)
    args = [_p(a, k) for k in ("x", "h0", "c0", "w_ih", "w_hh", "b_ih", "b_hh")]
    args += [T, B, I, H, _p(a, "series"), B * cols, a.get("series_sb", cols), cols, 0.0, P, P, None, None]
    if "wide" in name:
        args += [_p(a, "scratch"), _scratch(lib, "ctc_amd_lstm_series_wide_scratch_bytes", a, T, B, I, H)]
    return getattr(lib, name)(*args, None)


def series_backward(lib, name, a):
    T, B, H = a["T"], a["B"], a["H"]
    return getattr(lib, name)(_p(a, "d_series"), B * H, H, _p(a, "gates"), _p(a, "cells"), _p(a, "w_hh"), T, B, H, _p(a, "dpre"),
                              _p(a, "dh0"), _p(a, "dc0"), None)


def lstm_backward(lib, name, a):
    T, B, I, H = a["T"], a["B"], a["I"], a["H"]
    dsb, xsb, ssb, gsb = a.get("ds_sb", H), a.get("x_sb", I), a.get("series_sb", H), a.get("dx_sb", I)
    return getattr(lib, name)(_p(a, "d_series"), B * dsb, dsb, _p(a, "gates"), _p(a, "cells"), _p(a, "x"), B * xsb, xsb, _p(a, "h0"),
                              _p(a, "series"), B * ssb, ssb, _p(a, "w_ih"), _p(a, "w_hh"), T, B, I, H, _p(a, "d_x"), B * gsb, gsb,
                              _p(a, "dh0"), _p(a, "dc0"), _p(a, "d_w_ih"), _p(a, "d_w_hh"), _p(a, "d_b_ih"), _p(a, "d_b_hh"),
                              _p(a, "scratch"), _scratch(lib, "ctc_amd_lstm_backward_scratch_bytes", a, T, B, I, H), None)


def cell_step(lib, name, a):
    B, I, H = a["B"], a["I"], a["H"]
    cols = a.get("cols", H)
    return getattr(lib, name)(*[_p(a, k) for k in ("x", "h0", "c0", "w_ih", "w_hh", "b_ih", "b_hh")], B, I, H, _p(a, "h_out"),
                              _p(a, "c_out"), P, _p(a, "series"), a.get("series_sb", cols), cols, 0.0, None)


def bias_grad(lib, name, a):
    return getattr(lib, name)(_p(a, "dpre"), a["T"], a["H"], _p(a, "d_b_ih"), _p(a, "d_b_hh"), None)


def _scratch(lib, query, a, *shape):
    need = getattr(lib, query)(*shape)
    return max(need - 1, 0) if a.get("short") else a.get("scratch_bytes", need)


def _call(lib, name, a, args, at):
    """the head entries: feat_dtype behind the feat pointer of the typed entry, the untyped sibling for dtype None"""
    if a["dtype"] is None:
        return getattr(lib, name)(*args, None)
    return getattr(lib, name + "_typed")(*args[:at + 1], a["dtype"], *args[at + 1:], None)


def _null(*names):
    return [("%s=NULL" % n, {n: None}, True) for n in names]


def _sizes(**values):
    """name=(faults, modifiers): a fault is refused whatever else the call holds, a modifier only rides along"""
    return [("%s=%d" % (n, v), {n: v}, i == 0) for n, pair in values.items() for i, vs in enumerate(pair) for v in vs]


HEAD_ALIGN = [("feat+4", {"feat": P + 4}, True), ("feat+2", {"feat": P + 2}, True), ("feat+8", {"feat": P + 8}, False),
              ("weight+8", {"weight": P + 8}, True), ("weight+4", {"weight": P + 4}, True), ("fsb=K+2", {"fsb": 34}, True),
              ("fst+2", {"fst": 10 * 32 + 2}, True), ("dtype=3", {"dtype": 3}, True), ("dtype=-1", {"dtype": -1}, True)]
HEAD_BASES = [dict(T=2, B=10, K=32, C=8), dict(T=1, B=2, K=16, C=1), dict(T=3, B=37, K=32, C=17)]
WIDE_BASES = HEAD_BASES + [dict(T=2, B=300, K=32, C=8)]
SERIES_BASES = [dict(T=2, B=10, I=33, H=33), dict(T=1, B=1, I=1, H=1), dict(T=3, B=5, I=16, H=64)]
SERIES_WIDE_BASES = SERIES_BASES + [dict(T=2, B=3, I=158, H=158)]
SERIES_PTRS = ("x", "h0", "c0", "w_ih", "w_hh", "b_ih", "b_hh", "series")
MODES = [dict(mode="train"), dict(mode="eval")]
DTYPES = [dict(dtype=d) for d in (None, 0, 1, 2)]
FWD_STATS = [("rm only", {"mode": "train", "rm": P}, True), ("rv only", {"mode": "train", "rv": P}, True)]
BWD_STATS = [("train-smean", {"mode": "train", "smean": None}, True), ("train-sinv", {"mode": "train", "sinv": None}, True),
             ("train+rm", {"mode": "train", "rm": P}, True), ("train+rv", {"mode": "train", "rv": P}, True),
             ("eval-rm", {"mode": "eval", "rm": None}, True), ("eval-rv", {"mode": "eval", "rv": None}, True),
             ("eval+smean", {"mode": "eval", "smean": P}, True), ("no statistics", {"mode": "eval", "rm": None, "rv": None}, True)]
SHORT = [("scratch one byte short", {"short": True}, True)]
# the pitch of an optional pointer is not looked at without the pointer: such a pair is a valid call
MOOT = {("d_feat=NULL", "dfeat pitch=K-1"), ("d_x=NULL", "dx pitch=I-1"), ("no series row", "cols=H-1"),
        ("no series row", "pitch=cols-1")}


def head_variations(name):
    wide, bwd, fused = "wide" in name, "backward" in name, "lstm_forward" in name
    ranged = wide or bwd                                     # the entries with the bound on T B and the task count
    v = _sizes(T=((0, -3) + ((BIG, ROWS // 2 + 1) if ranged or fused else ()), () if ranged or fused else (BIG,)),
               B=((0, -1) + (() if fused else (65537 if wide else 257, BIG)), (BIG,) if fused else ()),
               K=((0, -16, 24, 17), (BIG,)),
               C=((0, -1) + ((41,) if fused else ()) + ((65535 * 16 + 1, BIG) if ranged else ()), () if ranged else (BIG,)))
    v += HEAD_ALIGN
    if fused:
        v += _null("feat", "weight", "bias", "bn_weight", "bn_bias", "out", "h0", "c0", "w_ih", "w_hh", "b_ih", "b_hh")
        v += [("train mode", {"mode": "train"}, True), ("eval-rm", {"rm": None}, True), ("eval-rv", {"rv": None}, True),
              ("cols=0", {"cols": 0}, True), ("series pitch=0", {"out_sb": 0}, True)]
    elif bwd:
        v += _null("d_out", "feat", "weight", "bn_weight", "bn_bias", "linear_out", "d_weight", "d_bias", "d_bn_weight", "d_bn_bias",
                   "scratch") + BWD_STATS + SHORT
        v += [("d_feat=NULL", {"d_feat": None}, False), ("d_feat+1", {"d_feat": P + 1}, False), ("d_feat+2", {"d_feat": P + 2}, False),
              ("B=1 train", {"B": 1, "mode": "train"}, True), ("dout pitch=C-1", {"dout_sb": 0}, True),
              ("dfeat pitch=K-1", {"dfeat_sb": 15}, True)]
    else:
        v += _null("feat", "weight", "bias", "bn_weight", "bn_bias", "out") + FWD_STATS
        v += [("B=1 train", {"B": 1, "mode": "train"}, True), ("out pitch=C-1", {"out_sb": 0}, True)]
        if wide:
            v += _null("scratch") + SHORT
    return v


def series_variations(name):
    wide = "wide" in name
    v = _null(*SERIES_PTRS) + _sizes(T=((0, -1) + ((BIG,) if wide else ()), () if wide else (BIG,)),
                                     B=((0, -1) + ((BIG,) if wide else ()), () if wide else (BIG,)),
                                     I=((0, -1, 161 if wide else 65, BIG), ()), H=((0, -1, 161 if wide else 65, BIG), ()))
    v += [("cols=H-1", {"cols": 0}, True), ("pitch=cols-1", {"series_sb": 0}, True)]
    if wide:
        v += _null("scratch") + SHORT + [("rows past 2^22", {"T": ROWS // 2 + 1, "B": 2}, True)]
    else:
        v += [("I+H=81", {"I": 48, "H": 33}, True)]
    return v


def entries():
    out = []
    for name in ("ctc_amd_head_forward", "ctc_amd_head_forward_wide", "ctc_amd_lstm_forward"):
        modes = MODES[1:] if "lstm" in name else MODES
        out.append((name, head_forward, WIDE_BASES if "wide" in name else HEAD_BASES, modes, DTYPES, head_variations(name)))
    for name in ("ctc_amd_head_backward", "ctc_amd_head_backward_wide"):
        out.append((name, head_backward, WIDE_BASES if "wide" in name else HEAD_BASES, MODES, DTYPES, head_variations(name)))
    for name in ("ctc_amd_lstm_series", "ctc_amd_lstm_series_wide"):
        out.append((name, series, SERIES_WIDE_BASES if "wide" in name else SERIES_BASES, [{}], [{}], series_variations(name)))
    for name in ("ctc_amd_lstm_series_backward", "ctc_amd_lstm_series_backward_wide"):
        wide = "wide" in name
        v = _null("d_series", "gates", "cells", "w_hh", "dpre", "dh0", "dc0")
        v += _sizes(T=((0, -1), (BIG,)), B=((0, -1), (BIG,)), H=((0, -1) + ((161, BIG) if wide else (65,)), ()))
        out.append((name, series_backward, SERIES_WIDE_BASES if wide else SERIES_BASES, [{}], [{}], v))
    v = _null("d_series", "gates", "cells", "x", "h0", "series", "w_ih", "w_hh", "dh0", "dc0", "d_w_ih", "d_w_hh", "d_b_ih", "d_b_hh",
              "scratch") + SHORT
    v += _sizes(T=((0, -1, BIG), ()), B=((0, -1, BIG), ()), I=((0, -1, 65, BIG), ()), H=((0, -1, 65, BIG), ()))
    v += [("I+H=81", {"I": 48, "H": 33}, True), ("rows past 2^22", {"T": ROWS // 2 + 1, "B": 2}, True), ("d_x=NULL", {"d_x": None}, False),
          ("ds pitch=H-1", {"ds_sb": 0}, True), ("series pitch=H-1", {"series_sb": 0}, True), ("x pitch=I-1", {"x_sb": 0}, True),
          ("dx pitch=I-1", {"dx_sb": 0}, True)]
    out.append(("ctc_amd_lstm_backward", lstm_backward, SERIES_BASES, [{}], [{}], v))
    v = _null("x", "h0", "c0", "w_ih", "w_hh", "b_ih", "b_hh", "h_out", "c_out")
    v += _sizes(B=((0, -1), (BIG,)), I=((0, -1, BIG), ()), H=((0, -1, 1100, BIG), ()))
    v += [("cols=H-1", {"cols": 0}, True), ("pitch=cols-1", {"series_sb": 0}, True), ("no series row", {"series": None}, False)]
    out.append(("ctc_amd_lstm_cell_step", cell_step, SERIES_BASES, [{}], [{}], v))
    v = _null("dpre", "d_b_ih", "d_b_hh") + _sizes(T=((0, -1), (BIG,)), H=((0, -1, 161, BIG), ()))
    out.append(("ctc_amd_lstm_bias_grad_wide", bias_grad, SERIES_WIDE_BASES, [{}], [{}], v))
    return out


QUERIES = {"ctc_amd_head_backward_scratch_bytes": ([-1, 0, 1, 2, 10, ROWS // 2 + 1, BIG], [-1, 0, 1, 2, 256, 257, 65536, 65537, BIG],
                                                  [-16, 0, 1, 16, 24, 1024, BIG], [-1, 0, 1, 33, 65535 * 16, 65535 * 16 + 1, BIG]),
           "ctc_amd_lstm_backward_scratch_bytes": ([-1, 0, 1, 10, ROWS // 2 + 1, BIG], [-1, 0, 1, 2, 256, BIG],
                                                  [-1, 0, 1, 33, 47, 48, 64, 65, BIG], [-1, 0, 1, 33, 64, 65, BIG])}
QUERIES["ctc_amd_head_forward_wide_scratch_bytes"] = QUERIES["ctc_amd_head_backward_wide_scratch_bytes"] = \
    QUERIES["ctc_amd_head_backward_scratch_bytes"]
QUERIES["ctc_amd_lstm_series_wide_scratch_bytes"] = ([-1, 0, 1, 10, ROWS // 2 + 1, BIG], [-1, 0, 1, 2, 256, BIG],
                                                     [-1, 0, 1, 33, 160, 161, BIG], [-1, 0, 1, 33, 160, 161, BIG])


def dump(path):
    from ctc_amd import _lib
    lib = _lib.load()
    lines, passed = [], 0
    for name, fn, bases, modes, dtypes, variations in entries():
        for shape, mode, dt in itertools.product(bases, modes, dtypes):
            base = {**shape, **mode, **dt}
            tag = "%s %s" % (name, " ".join("%s=%s" % kv for kv in sorted(base.items())))
            calls = [(v,) for v in variations if v[2] is True]
            calls += [(v, w) for v, w in itertools.combinations(variations, 2)
                      if True in (v[2], w[2]) and not set(v[1]) & set(w[1]) and (v[0], w[0]) not in MOOT and (w[0], v[0]) not in MOOT]
            for vs in calls:
                a = dict(base)
                for _, upd, _f in vs:
                    a.update(upd)
                if a.get("dtype") in (3, -1) and dt.get("dtype", 0) is None:
                    continue                                 # (the untyped entries have no dtype argument)
                rc = fn(lib, name, a)
                if rc not in (_lib.ERR_BAD_ARGUMENT, _lib.ERR_UNSUPPORTED_SHAPE):
                    passed += 1
                    rc = "not refused (%d)" % rc
                lines.append("%s | %s | %s" % (tag, " + ".join(v[0] for v in vs), rc))
    for q, grids in sorted(QUERIES.items()):
        for shape in itertools.product(*grids):
            lines.append("%s | %s | %d" % (q, shape, getattr(lib, q)(*shape)))
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("%s: %d calls of %s, %d not refused" % (path, len(lines), _lib.SO_PATH, passed))


def compare(old, new, allow):
    a, b = open(old).read().splitlines(), open(new).read().splitlines()
    assert len(a) == len(b), (len(a), len(b))
    diff = [(x, y) for x, y in zip(a, b) if x != y]
    allowed = [d for d in diff if any(re.search(s, d[1]) for s in allow) and d[0].rsplit("|", 1)[0] == d[1].rsplit("|", 1)[0]]
    other = [d for d in diff if d not in allowed]
    print("%d calls compared, %d differ: %d allowed, %d not" % (len(a), len(diff), len(allowed), len(other)))
    for x, y in other[:50]:
        print("  OLD %s\n  NEW %s" % (x, y))
    seen = sorted({(x.split("|", 1)[0].split()[0], x.rsplit("|", 1)[1].strip(), y.rsplit("|", 1)[1].strip()) for x, y in allowed})
    for s in seen:
        print("  allowed: %s %s -> %s" % s)
    return 1 if other else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out")
    ap.add_argument("--compare", nargs=2)
    ap.add_argument("--allow", action="append", default=[])
    o = ap.parse_args()
    if o.compare:
        sys.exit(compare(*o.compare, o.allow))
    dump(o.out)
