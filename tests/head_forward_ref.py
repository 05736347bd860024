"""The head's forward (ctc_amd_head_forward / ctc_amd_head_forward_wide, include/ctc_amd.h) restated in float64 numpy -- the
oracle of tests/test_head_wide_gpu.py, itself pinned against torch's float64 layers in tests/test_head_wide_abi.py.
A helper, no test."""
import numpy as np

TOL = 1e-4                                       # bound on |got - ref| / max(1, max|ref|) for out and the statistics
OFFSET_SHAPE, OFFSET = (2, 300, 32, 8), 1000.0   # the common-offset case: lin ~ 1000 + noise of variance ~0.2


def head_forward_ref(feat, weight, bias, bn_weight, bn_bias, running_mean=None, running_var=None, eps=1e-5, mask=None):
    """the entry's own inputs (fp32 arrays, widened here) -> (out [T,B,C], lin [T,B,C], mean, var, invstd).  Train mode
    (running_mean is None): the statistics of each frame's B rows, [T,C], two passes, biased variance; eval mode: the running
    statistics, [C], invstd computed from them."""
    w = lambda a: np.asarray(a, np.float64)          # noqa: E731
    feat, weight, bias, g, be = (w(a) for a in (feat, weight, bias, bn_weight, bn_bias))
    e = np.float64(np.float32(eps))
    lin = feat @ weight.T + bias                                         # [T,B,C]
    if running_mean is None:
        assert running_var is None
        mean = lin.mean(1)                                               # [T,C]
        var = ((lin - mean[:, None, :]) ** 2).mean(1)                    # the centred second moment, biased
        inv = 1.0 / np.sqrt(var + e)
        y = (lin - mean[:, None, :]) * inv[:, None, :] * g + be
    else:
        mean, var = w(running_mean), w(running_var)
        inv = 1.0 / np.sqrt(var + e)
        y = (lin - mean) * inv * g + be
    out = np.maximum(y, 0.0)
    if mask is not None:
        out = out * w(mask)
    return out, lin, mean, var, inv


def draw_forward_case(shape, train, with_mask, seed, offset=0.0):
    """fp32 inputs of the entry for (T, B, K, C), drawn with a fixed seed.  ``offset``: added to the Linear bias, so that every
    column of lin carries that common offset (lin ~ offset + noise): what a one-pass variance does not survive."""
    T, B, K, C = shape
    rng = np.random.default_rng(seed)
    u = lambda *s: rng.uniform(-1.0, 1.0, s).astype(np.float32)          # noqa: E731
    d = dict(feat=u(T, B, K), weight=(u(C, K) * 0.25).astype(np.float32),
             bias=(u(C) * 0.1 + np.float32(offset)).astype(np.float32),
             bn_weight=(u(C) * 0.5 + 1.0).astype(np.float32), bn_bias=(u(C) * 0.2).astype(np.float32), eps=1e-5)
    if not train:
        d["running_mean"] = (u(C) * 0.3 + np.float32(offset)).astype(np.float32)
        d["running_var"] = (u(C) * 0.4 + 1.0).astype(np.float32)
    d["mask"] = ((u(T, B, C) > -0.4).astype(np.float32) / np.float32(0.7)) if with_mask else None
    return d
