"""The head for batches beyond 256 samples (ctc_amd_head_forward_wide, ctc_amd_head_backward_wide and their scratch queries):
the C ABI (declared, exported, bound, every argument error reported before any HIP call -- bogus host pointers, no device
needed), the Python surface, and the float64 restatement of the forward (tests/head_forward_ref.py) pinned against torch's
float64 layers on the CPU.  tests/test_head_wide_gpu.py checks the kernels."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests.head_forward_ref import draw_forward_case, head_forward_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FWD, FWD_QUERY = "ctc_amd_head_forward_wide", "ctc_amd_head_forward_wide_scratch_bytes"
BWD, BWD_QUERY = "ctc_amd_head_backward_wide", "ctc_amd_head_backward_wide_scratch_bytes"
FWD_REQUIRED = ["feat", "weight", "bias", "bn_weight", "bn_bias", "out", "scratch"]
FWD_OPTIONAL = ["mask", "linear_out", "save_mean", "save_var", "save_invstd"]
BWD_REQUIRED = ["d_out", "feat", "weight", "bn_weight", "bn_bias", "linear_out", "d_weight", "d_bias", "d_bn_weight", "d_bn_bias",
                "scratch"]
BAD_ARGUMENT, UNSUPPORTED_SHAPE = -1, -2
MAX_BATCH = 65536                                            # the documented bound on B (include/ctc_amd.h)
# K not a multiple of 16; feat off by 4 bytes; strides that are no multiples of 4; weight unaligned; row counts beyond 2^22
# (no int overflow on the way); a batch beyond the bound
UNSUPPORTED = [dict(K=24), dict(feat_ptr=4096 + 4), dict(fsb=1026), dict(fst=300 * 1024 + 2), dict(ptr=4096 + 8, feat_ptr=4096),
               dict(T=1 << 30), dict(T=(1 << 22) // 8 + 1, B=8), dict(T=1, B=MAX_BATCH + 1), dict(T=2, B=1 << 30)]


@pytest.fixture(scope="module")
def lib():
    from ctc_amd import _lib, build
    build.build()
    return _lib.load()


def test_symbols_declared_exported_and_bound(lib):
    from ctc_amd import _lib
    header = open(os.path.join(ROOT, "include", "ctc_amd.h")).read()
    so = ctypes.CDLL(_lib.SO_PATH)
    names = {}
    for name, narrow in ((FWD, "ctc_amd_head_forward"), (BWD, "ctc_amd_head_backward")):
        lists = []
        for n in (name, narrow):
            m = re.search(r"\bint %s\s*\(([^;]*)\);" % n, header)
            assert m, "%s is not declared in include/ctc_amd.h" % n
            lists.append([" ".join(a.split()) for a in m.group(1).split(",") if a.strip()])
        names[name] = lists
        assert hasattr(so, name)
        res, args = _lib.PROTOTYPES[name]
        assert res is ctypes.c_int and len(args) == len(lists[0])
    for q in (FWD_QUERY, BWD_QUERY):
        assert re.search(r"\bsize_t %s\s*\(int T, int B, int K, int C\);" % q, header)
        assert hasattr(so, q)
        res, args = _lib.PROTOTYPES[q]
        assert res is ctypes.c_size_t and len(args) == 4
    # forward: the narrow entry's arguments, then the scratch, then the stream; backward: the narrow entry's list exactly
    wide, narrow = names[FWD]
    assert wide == narrow[:-1] + ["void *scratch", "size_t scratch_bytes", "void *stream"] and len(wide) == 25
    assert names[BWD][0] == names[BWD][1] and len(names[BWD][0]) == 30
    narrow = _lib.PROTOTYPES["ctc_amd_head_forward"][1]
    assert _lib.PROTOTYPES[FWD][1] == narrow[:-1] + [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    assert _lib.PROTOTYPES[BWD][1] == _lib.PROTOTYPES["ctc_amd_head_backward"][1]
    assert lib.ctc_amd_abi_version() == 2 and "#define CTC_AMD_ABI_VERSION 2" in header       # (additions do not bump it)


def _fwd(lib, ptr=4096, T=10, B=300, K=1024, C=33, mode="train", feat_ptr=None, fst=None, fsb=None, out_sb=None,
         scratch_bytes=None, **null):
    """every pointer is a bogus, 16-byte aligned host address: a call that got past the checks would fault, not return.
    null: NAME=True makes a pointer NULL."""
    present = {k: True for k in FWD_REQUIRED + FWD_OPTIONAL}
    present.update(running_mean=mode == "eval", running_var=mode == "eval")
    for k, v in null.items():
        assert k in present
        present[k] = not v
    p = {k: (ptr if present[k] else None) for k in present}
    if feat_ptr is not None:
        p["feat"] = feat_ptr
    fsb = K if fsb is None else fsb
    fst = B * fsb if fst is None else fst
    out_sb = C if out_sb is None else out_sb
    if scratch_bytes is None:
        scratch_bytes = lib.ctc_amd_head_forward_wide_scratch_bytes(T, B, K, C)
    return lib.ctc_amd_head_forward_wide(p["feat"], fst, fsb, p["weight"], p["bias"], p["bn_weight"], p["bn_bias"],
                                         p["running_mean"], p["running_var"], 1e-5, p["mask"], T, B, K, C, p["out"], B * out_sb,
                                         out_sb, p["linear_out"], p["save_mean"], p["save_var"], p["save_invstd"], p["scratch"],
                                         scratch_bytes, None)


def _bwd(lib, ptr=4096, T=10, B=300, K=1024, C=33, mode="train", feat_ptr=None, fst=None, fsb=None, dout_sb=None, dfeat_sb=None,
         scratch_bytes=None, **null):
    present = {k: True for k in BWD_REQUIRED}
    present.update(save_mean=mode == "train", save_invstd=mode == "train", running_mean=mode == "eval",
                   running_var=mode == "eval", mask=True, d_feat=True)
    for k, v in null.items():
        assert k in present
        present[k] = not v
    p = {k: (ptr if present[k] else None) for k in present}
    if feat_ptr is not None:
        p["feat"] = feat_ptr
    fsb = K if fsb is None else fsb
    fst = B * fsb if fst is None else fst
    dout_sb = C if dout_sb is None else dout_sb
    dfeat_sb = K if dfeat_sb is None else dfeat_sb
    if scratch_bytes is None:
        scratch_bytes = lib.ctc_amd_head_backward_wide_scratch_bytes(T, B, K, C)
    return lib.ctc_amd_head_backward_wide(p["d_out"], B * dout_sb, dout_sb, p["feat"], fst, fsb, p["weight"], p["bn_weight"],
                                          p["bn_bias"], p["linear_out"], p["save_mean"], p["save_invstd"], p["running_mean"],
                                          p["running_var"], 1e-5, p["mask"], T, B, K, C, p["d_feat"], B * dfeat_sb, dfeat_sb,
                                          p["d_weight"], p["d_bias"], p["d_bn_weight"], p["d_bn_bias"], p["scratch"],
                                          scratch_bytes, None)


@pytest.mark.parametrize("mode", ["train", "eval"])
@pytest.mark.parametrize("which", FWD_REQUIRED)
def test_forward_null_pointers(lib, which, mode):
    assert _fwd(lib, mode=mode, **{which: True}) == BAD_ARGUMENT
    assert _fwd(lib, mode=mode, mask=True, linear_out=True, save_mean=True, save_var=True, save_invstd=True,
                **{which: True}) == BAD_ARGUMENT
    assert _fwd(lib, mode=mode, K=24, **{which: True}) == BAD_ARGUMENT           # the bad argument wins over the shape


@pytest.mark.parametrize("mode", ["train", "eval"])
@pytest.mark.parametrize("which", BWD_REQUIRED)
def test_backward_null_pointers(lib, which, mode):
    assert _bwd(lib, mode=mode, **{which: True}) == BAD_ARGUMENT
    assert _bwd(lib, mode=mode, K=24, **{which: True}) == BAD_ARGUMENT


@pytest.mark.parametrize("kw", [
    dict(T=0), dict(B=0), dict(K=0), dict(C=0), dict(T=-3), dict(B=-1), dict(K=-16), dict(C=-1),
    dict(mode="eval", running_mean=True), dict(mode="eval", running_var=True),  # one running statistic without the other
    dict(B=1),                                      # train mode needs two rows per frame
    dict(out_sb=32),
    dict(scratch_bytes=0),
    # a bad argument together with an unsupported shape: the bad argument wins
    dict(T=0, K=24), dict(B=1, feat_ptr=4096 + 4), dict(out_sb=32, fsb=1026), dict(scratch=True, T=1 << 30),
    dict(bias=True, B=MAX_BATCH + 1), dict(T=0, B=MAX_BATCH + 1),
])
def test_forward_bad_arguments(lib, kw):
    assert _fwd(lib, **kw) == BAD_ARGUMENT


@pytest.mark.parametrize("kw", [
    dict(T=0), dict(B=0), dict(K=0), dict(C=0), dict(T=-3), dict(C=-1),
    # the statistics are not exactly one complete pair
    dict(save_mean=True), dict(save_invstd=True), dict(save_mean=True, save_invstd=True),
    dict(running_mean=False), dict(running_var=False), dict(running_mean=False, running_var=False),
    dict(mode="eval", running_mean=True), dict(mode="eval", running_var=True), dict(mode="eval", save_mean=False),
    dict(mode="eval", save_invstd=False, save_mean=False),
    dict(B=1),
    dict(dout_sb=32), dict(dfeat_sb=1023),
    dict(scratch_bytes=0),
    dict(T=0, B=MAX_BATCH + 1), dict(d_out=True, K=24), dict(save_mean=True, K=24), dict(B=1, feat_ptr=4096 + 4),
    dict(dout_sb=32, fsb=1026), dict(dfeat_sb=8, K=24), dict(scratch=True, T=1 << 30), dict(d_bias=True, B=MAX_BATCH + 1),
])
def test_backward_bad_arguments(lib, kw):
    assert _bwd(lib, **kw) == BAD_ARGUMENT


def test_the_scratch_bound_is_the_query(lib):
    for (T, B, K, C) in ((10, 300, 1024, 33), (1, 2, 16, 1), (2, 4096, 64, 158), (3, 37, 32, 17)):
        need = lib.ctc_amd_head_forward_wide_scratch_bytes(T, B, K, C)
        assert need > 0
        assert _fwd(lib, T=T, B=B, K=K, C=C, scratch_bytes=need - 1) == BAD_ARGUMENT
        assert _fwd(lib, T=T, B=B, K=K, C=C, scratch_bytes=need - 1, mode="eval", linear_out=True) == BAD_ARGUMENT
        need = lib.ctc_amd_head_backward_wide_scratch_bytes(T, B, K, C)
        assert need > 0
        assert _bwd(lib, T=T, B=B, K=K, C=C, scratch_bytes=need - 1) == BAD_ARGUMENT
        assert _bwd(lib, T=T, B=B, K=K, C=C, scratch_bytes=need - 1, d_feat=True, mode="eval") == BAD_ARGUMENT


@pytest.mark.parametrize("mode", ["train", "eval"])
@pytest.mark.parametrize("kw", UNSUPPORTED, ids=lambda kw: "-".join("%s%d" % kv for kv in kw.items()))
def test_unsupported_shapes(lib, kw, mode):
    assert _fwd(lib, mode=mode, **kw) == UNSUPPORTED_SHAPE
    assert _fwd(lib, mode=mode, mask=True, linear_out=True, save_mean=True, save_var=True, save_invstd=True,
                **kw) == UNSUPPORTED_SHAPE
    assert _bwd(lib, mode=mode, **kw) == UNSUPPORTED_SHAPE
    assert _bwd(lib, mode=mode, d_feat=True, **kw) == UNSUPPORTED_SHAPE


@pytest.mark.parametrize("q", [FWD_QUERY, BWD_QUERY])
def test_scratch_queries(lib, q):
    f = getattr(lib, q)
    for bad in [(0, 300, 1024, 33), (10, 0, 1024, 33), (10, 300, 0, 33), (10, 300, 1024, 0), (-1, 300, 1024, 33),
                (10, -300, 1024, 33), (10, 300, 24, 33), (1 << 30, 300, 1024, 33), (1, MAX_BATCH + 1, 1024, 33),
                ((1 << 22) // 8 + 1, 8, 1024, 33), (1 << 30, 1 << 30, 16, 5)]:
        assert f(*bad) == 0, bad
    sizes = [f(10, B, 1024, 33) for B in (2, 37, 256, 257, 300, 512, 2048, 4096, MAX_BATCH)]
    assert all(s > 0 for s in sizes) and sizes == sorted(set(sizes)), sizes      # non-zero and growing with B
    assert f((1 << 22) // 8, 8, 16, 5) > 0 and f(64, MAX_BATCH, 16, 5) > 0
    if q == FWD_QUERY:      # the Linear output [T B][C] and the column sums of every block of 256 rows [T][NB][C padded to 16]
        assert f(10, 300, 1024, 33) >= 4 * (10 * 300 * 33 + 10 * 2 * 48)
        assert f(2, 2048, 64, 158) >= 4 * (2 * 2048 * 158 + 2 * 8 * 160)
    else:                   # the narrow entry's layout: dlin [T B][C padded], three [T][C padded] partials, the weight partials
        assert f(10, 300, 1024, 33) >= 4 * (3000 * 48 + 3 * 10 * 48 + 24 * 33 * 1024)
        assert f(10, 10, 1024, 33) == lib.ctc_amd_head_backward_scratch_bytes(10, 10, 1024, 33)


def test_the_narrow_entries_still_refuse_b300(lib):
    p, T, B, K, C = 4096, 10, 300, 1024, 33
    assert lib.ctc_amd_head_forward(p, B * K, K, p, p, p, p, None, None, 1e-5, None, T, B, K, C, p, B * C, C,
                                    None, None, None, None, None) == UNSUPPORTED_SHAPE
    assert lib.ctc_amd_head_forward(p, B * K, K, p, p, p, p, p, p, 1e-5, None, T, B, K, C, p, B * C, C,
                                    None, None, None, None, None) == UNSUPPORTED_SHAPE
    assert lib.ctc_amd_head_backward_scratch_bytes(T, B, K, C) == 0
    assert lib.ctc_amd_head_backward(p, B * C, C, p, B * K, K, p, p, p, p, p, p, None, None, 1e-5, None, T, B, K, C,
                                     p, B * K, K, p, p, p, p, p, 1 << 30, None) == UNSUPPORTED_SHAPE


def test_python_export():
    import ctc_amd
    from ctc_amd import producer
    for name in ("head_forward_wide", "head_backward_wide"):
        assert callable(getattr(producer, name)) and getattr(ctc_amd, name) is getattr(producer, name)
        assert name in ctc_amd.__all__
    for gate in ("HEAD_WIDE_MAX_ROWS", "HEAD_WIDE_BACKWARD_MAX_ROWS"):
        assert type(getattr(producer, gate)) is int and getattr(producer, gate) >= 0
    import inspect
    for wide, narrow in ((producer.head_forward_wide, producer.head_forward), (producer.head_backward_wide, producer.head_backward)):
        assert inspect.signature(wide) == inspect.signature(narrow)


def test_no_cpu_path():
    import torch
    import ctc_amd
    z = torch.zeros
    with pytest.raises(ctc_amd.CtcAmdError):
        ctc_amd.head_forward_wide(z(2, 300, 16), z(5, 16), z(5), z(5), z(5))
    with pytest.raises(ctc_amd.CtcAmdError):
        ctc_amd.head_backward_wide(z(2, 300, 5), z(2, 300, 16), z(5, 16), z(5), z(5), z(2, 300, 5), mean=z(2, 5),
                                   invstd=torch.ones(2, 5))


@pytest.mark.parametrize("shape", [(4, 37, 64, 40), (2, 300, 32, 8), (2, 2, 16, 5)])
@pytest.mark.parametrize("train", [True, False])
@pytest.mark.parametrize("with_mask", [True, False])
def test_restatement_equals_torch_float64_layers(shape, train, with_mask):
    """nn.Linear / nn.BatchNorm1d / nn.ReLU applied frame by frame in float64 on the CPU, times the mask, against the
    restatement -- out, the Linear output and (train mode) the statistics BatchNorm normalises with, to 1e-12.  eps is a power
    of two: the restatement rounds it to fp32, as the entry's float argument does."""
    import torch
    T, B, K, C = shape
    eps = 2.0 ** -17
    d = draw_forward_case(shape, train, with_mask, seed=sum(shape) + 2 * int(train) + int(with_mask))
    lin, bn = torch.nn.Linear(K, C).double(), torch.nn.BatchNorm1d(C, eps=eps).double()
    with torch.no_grad():
        lin.weight.copy_(torch.from_numpy(d["weight"]).double()); lin.bias.copy_(torch.from_numpy(d["bias"]).double())
        bn.weight.copy_(torch.from_numpy(d["bn_weight"]).double()); bn.bias.copy_(torch.from_numpy(d["bn_bias"]).double())
        if not train:
            bn.running_mean.copy_(torch.from_numpy(d["running_mean"]).double())
            bn.running_var.copy_(torch.from_numpy(d["running_var"]).double())
    bn.train(train)
    feat = torch.from_numpy(d["feat"]).double()
    with torch.no_grad():
        lins = torch.stack([lin(feat[t]) for t in range(T)])
        want = torch.stack([torch.relu(bn(lins[t])) for t in range(T)])
    if with_mask:
        want = want * torch.from_numpy(d["mask"]).double()
    out, lo, mean, var, inv = head_forward_ref(d["feat"], d["weight"], d["bias"], d["bn_weight"], d["bn_bias"],
                                               d.get("running_mean"), d.get("running_var"), eps, d["mask"])
    assert out.shape == (T, B, C) and lo.shape == (T, B, C)
    assert np.abs(out - want.numpy()).max() <= 1e-12
    assert np.abs(lo - lins.numpy()).max() <= 1e-12
    if train:
        assert mean.shape == var.shape == inv.shape == (T, C)
        assert np.abs(mean - lins.mean(1).numpy()).max() <= 1e-12
        assert np.abs(var - lins.var(1, unbiased=False).numpy()).max() <= 1e-12
        assert np.abs(inv - torch.rsqrt(lins.var(1, unbiased=False) + eps).numpy()).max() <= 1e-12
    else:
        assert mean.shape == var.shape == inv.shape == (C,)
        assert np.abs(inv - 1.0 / np.sqrt(d["running_var"].astype(np.float64) + eps)).max() <= 1e-12


def test_the_offset_case_separates_two_passes_from_one():
    """the common-offset case of tests/test_head_wide_gpu.py, on the CPU: plain fp32 numpy in two passes (the mean, then the
    centred second moment) stays inside that test's bound on var, 1e-4 max(1, max|ref|); one pass (E[x^2] - mean^2) does not"""
    from tests.head_forward_ref import OFFSET, OFFSET_SHAPE, TOL
    d = draw_forward_case(OFFSET_SHAPE, True, False, seed=4242, offset=OFFSET)
    _, lin64, _, var, _ = head_forward_ref(d["feat"], d["weight"], d["bias"], d["bn_weight"], d["bn_bias"])
    assert abs(float(lin64.mean()) - OFFSET) < 1.0
    lin = (d["feat"] @ d["weight"].T + d["bias"]).astype(np.float32)
    B = np.float32(lin.shape[1])
    mean = lin.sum(1, dtype=np.float32) / B
    two = ((lin - mean[:, None, :]) ** 2).sum(1, dtype=np.float32) / B
    one = (lin * lin).sum(1, dtype=np.float32) / B - mean * mean
    bound = TOL * max(1.0, float(np.abs(var).max()))
    print("offset case: two-pass |var - ref| = %.3e, one-pass %.3e, bound %.3e" % (np.abs(two - var).max(), np.abs(one - var).max(), bound))
    assert np.abs(two - var).max() <= bound
    assert np.abs(one - var).max() > bound
