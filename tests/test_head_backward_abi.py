"""The head's backward on the HIP path (ctc_amd_head_backward): the C ABI (declared, exported, bound, every argument error
reported before any HIP call -- bogus host pointers, no device needed), the Python surface, and the float64 restatement
(tests/head_backward_ref.py) pinned against torch's float64 CPU autograd of the layers.
tests/test_head_backward_gpu.py checks the kernels against the restatement."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests.head_backward_ref import bn_output, head_backward_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME, QUERY = "ctc_amd_head_backward", "ctc_amd_head_backward_scratch_bytes"
REQUIRED = ["d_out", "feat", "weight", "bn_weight", "bn_bias", "linear_out", "d_weight", "d_bias", "d_bn_weight", "d_bn_bias",
            "scratch"]
BAD_ARGUMENT, UNSUPPORTED_SHAPE = -1, -2


@pytest.fixture(scope="module")
def lib():
    from ctc_amd import _lib, build
    build.build()
    return _lib.load()


def test_symbols_declared_exported_and_bound(lib):
    from ctc_amd import _lib
    header = open(os.path.join(ROOT, "include", "ctc_amd.h")).read()
    m = re.search(r"\bint %s\s*\(([^;]*)\);" % NAME, header)
    assert m, "not declared in include/ctc_amd.h"
    declared = [a for a in m.group(1).split(",") if a.strip()]
    assert re.search(r"\bsize_t %s\s*\(int T, int B, int K, int C\);" % QUERY, header)
    so = ctypes.CDLL(_lib.SO_PATH)
    assert hasattr(so, NAME) and hasattr(so, QUERY)
    res, args = _lib.PROTOTYPES[NAME]
    assert res is ctypes.c_int and len(args) == len(declared) == 30
    res, args = _lib.PROTOTYPES[QUERY]
    assert res is ctypes.c_size_t and len(args) == 4
    assert lib.ctc_amd_abi_version() == 2 and _lib.ABI_VERSION == 2
    assert "#define CTC_AMD_ABI_VERSION 2" in header


def _call(lib, ptr=4096, T=10, B=10, K=1024, C=33, mode="train", feat_ptr=None, fst=None, fsb=None, dout_sb=None, dfeat_sb=None,
          scratch_bytes=None, **null):
    """every pointer is a bogus, 16-byte aligned host address: a call that got past the checks would fault, not return.
    null: NAME=True makes a pointer NULL, NAME=False makes an optional pointer present."""
    present = {k: True for k in REQUIRED}
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
        scratch_bytes = lib.ctc_amd_head_backward_scratch_bytes(T, B, K, C)
    return lib.ctc_amd_head_backward(p["d_out"], B * dout_sb, dout_sb, p["feat"], fst, fsb, p["weight"], p["bn_weight"],
                                     p["bn_bias"], p["linear_out"], p["save_mean"], p["save_invstd"], p["running_mean"],
                                     p["running_var"], 1e-5, p["mask"], T, B, K, C, p["d_feat"], B * dfeat_sb, dfeat_sb,
                                     p["d_weight"], p["d_bias"], p["d_bn_weight"], p["d_bn_bias"], p["scratch"], scratch_bytes,
                                     None)


@pytest.mark.parametrize("mode", ["train", "eval"])
@pytest.mark.parametrize("which", REQUIRED)
def test_null_pointers(lib, which, mode):
    assert _call(lib, mode=mode, **{which: True}) == BAD_ARGUMENT


@pytest.mark.parametrize("kw", [
    dict(T=0), dict(B=0), dict(K=0), dict(C=0), dict(T=-3), dict(C=-1),
    # the statistics are not exactly one complete pair
    dict(save_mean=True), dict(save_invstd=True), dict(save_mean=True, save_invstd=True),
    dict(running_mean=False), dict(running_var=False), dict(running_mean=False, running_var=False),
    dict(mode="eval", running_mean=True), dict(mode="eval", running_var=True), dict(mode="eval", save_mean=False),
    dict(mode="eval", save_invstd=False, save_mean=False),
    dict(B=1),                                      # train mode needs two rows per frame
    dict(dout_sb=32), dict(dfeat_sb=1023),
    dict(scratch_bytes=0), dict(scratch_bytes=25343),       # (one byte below the query at (10, 10, 1024, 33))
    # a bad argument together with an unsupported shape: the bad argument wins
    dict(T=0, B=300), dict(d_out=True, K=24), dict(save_mean=True, K=24), dict(B=1, feat_ptr=4096 + 4),
    dict(dout_sb=32, fsb=1026), dict(dfeat_sb=8, K=24), dict(scratch=True, T=1 << 30), dict(d_bias=True, B=300),
])
def test_bad_arguments(lib, kw):
    assert _call(lib, **kw) == BAD_ARGUMENT


def test_the_scratch_bound_is_the_query(lib):
    need = lib.ctc_amd_head_backward_scratch_bytes(10, 10, 1024, 33)
    assert need == 25344
    assert _call(lib, scratch_bytes=need - 1) == BAD_ARGUMENT
    assert _call(lib, scratch_bytes=need - 1, d_feat=True) == BAD_ARGUMENT


@pytest.mark.parametrize("mode", ["train", "eval"])
@pytest.mark.parametrize("kw", [dict(B=300),                     # more rows than one workgroup holds
                                dict(K=24),                      # not a multiple of 16
                                dict(feat_ptr=4096 + 4),         # feat off by 4 bytes
                                dict(fsb=1026), dict(fst=10 * 1024 + 2),        # strides that are no multiples of 4
                                dict(ptr=4096 + 8, feat_ptr=4096),              # (weight unaligned)
                                dict(T=1 << 30),                 # (no int overflow on the way to that answer)
                                dict(T=(1 << 22) // 8 + 1, B=8)])               # one frame beyond 2^22 rows
def test_unsupported_shapes(lib, kw, mode):
    assert _call(lib, mode=mode, **kw) == UNSUPPORTED_SHAPE
    assert _call(lib, mode=mode, d_feat=True, **kw) == UNSUPPORTED_SHAPE


def test_scratch_query(lib):
    q = lib.ctc_amd_head_backward_scratch_bytes
    for bad in [(0, 10, 1024, 33), (10, 0, 1024, 33), (10, 10, 0, 33), (10, 10, 1024, 0), (-1, 10, 1024, 33),
                (10, 300, 1024, 33), (10, 10, 24, 33), (1 << 30, 10, 1024, 33)]:
        assert q(*bad) == 0, bad
    assert q(10, 10, 1024, 33) > 0
    # dlin [T B][C padded to 16] and three [T][C padded] partials at the least; the partial weight gradients beyond 128 rows
    assert q(10, 10, 1024, 33) >= 4 * (100 * 48 + 3 * 10 * 48)
    assert q(150, 256, 64, 33) >= 4 * (38400 * 48 + 3 * 150 * 48 + 64 * 33 * 64)
    assert q((1 << 22) // 8, 8, 16, 5) > 0


def test_python_export():
    import ctc_amd
    from ctc_amd import producer
    assert callable(producer.head_backward) and ctc_amd.head_backward is producer.head_backward
    assert "head_backward" in ctc_amd.__all__
    assert type(producer.HEAD_BACKWARD_MAX_ROWS) is int and producer.HEAD_BACKWARD_MAX_ROWS >= 0
    assert callable(producer._head_backward_torch)


def test_no_cpu_path():
    import torch
    import ctc_amd
    z = torch.zeros
    with pytest.raises(ctc_amd.CtcAmdError):
        ctc_amd.head_backward(z(2, 2, 5), z(2, 2, 16), z(5, 16), z(5), z(5), z(2, 2, 5), mean=z(2, 5), invstd=torch.ones(2, 5))


@pytest.mark.parametrize("shape", [(4, 37, 64, 40), (2, 2, 16, 5)])
@pytest.mark.parametrize("train", [True, False])
def test_restatement_equals_torch_float64_autograd(shape, train):
    """nn.Linear / nn.BatchNorm1d / nn.ReLU applied frame by frame in float64 on the CPU, times the mask; its autograd
    gradients against the restatement fed with the Linear output and the statistics of that very forward"""
    import torch
    T, B, K, C = shape
    g = torch.Generator().manual_seed(sum(shape) + int(train))
    rnd = lambda *s: (torch.rand(*s, generator=g, dtype=torch.float64) * 2 - 1)          # noqa: E731
    lin, bn = torch.nn.Linear(K, C).double(), torch.nn.BatchNorm1d(C).double()
    with torch.no_grad():
        bn.weight.copy_(rnd(C) * 0.5 + 1.0); bn.bias.copy_(rnd(C) * 0.2)
        bn.running_mean.copy_(rnd(C) * 0.3); bn.running_var.copy_(rnd(C) * 0.4 + 1.0)
    bn.train(train)
    rm, rv = bn.running_mean.clone().numpy(), bn.running_var.clone().numpy()
    mask = (rnd(T, B, C) > -0.4).double() / 0.7
    up = rnd(T, B, C)
    feat = rnd(T, B, K).requires_grad_(True)
    lins = [lin(feat[t]) for t in range(T)]
    out = torch.stack([torch.relu(bn(x)) for x in lins]) * mask
    (out * up).sum().backward()
    lo = torch.stack(lins).detach().numpy()
    kw = dict(mask=mask.numpy())
    if train:
        mean = lo.mean(1)
        inv = 1.0 / np.sqrt(lo.var(1) + bn.eps)
        kw.update(mean=mean, invstd=inv)
    else:
        mean, inv = rm, 1.0 / np.sqrt(rv + bn.eps)
        kw.update(running_mean=rm, running_var=rv, eps=bn.eps)
    # (the comparison is only meaningful away from the ReLU's corner)
    assert np.abs(bn_output(lo, bn.weight.detach().numpy(), bn.bias.detach().numpy(), mean, inv)).min() > 1e-9
    d_feat, d_w, d_b, d_g, d_be, _ = head_backward_ref(up.numpy(), feat.detach().numpy(), lin.weight.detach().numpy(),
                                                        bn.weight.detach().numpy(), bn.bias.detach().numpy(), lo, **kw)
    for got, want, what in ((d_feat, feat.grad, "d_feat"), (d_w, lin.weight.grad, "d_weight"), (d_b, lin.bias.grad, "d_bias"),
                            (d_g, bn.weight.grad, "d_bn_weight"), (d_be, bn.bias.grad, "d_bn_bias")):
        assert np.abs(got - want.numpy()).max() <= 1e-10, (what, shape, train)
