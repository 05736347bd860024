"""The head's backward (ctc_amd_head_backward, include/ctc_amd.h) restated in float64 numpy -- the oracle of
tests/test_head_backward_gpu.py, itself pinned against torch's float64 autograd in tests/test_head_backward_abi.py.
A helper, no test."""
import numpy as np

MARGIN = 1e-4          # no BatchNorm output of a drawn case lies this close to the ReLU's corner


def bn_output(lin, bn_weight, bn_bias, mean, inv):
    """y, the value the forward's ReLU tests; mean / inv: [T,C] (train) or [C] (eval), float64"""
    lin = np.asarray(lin, np.float64)
    mean, inv = (np.asarray(a, np.float64).reshape(-1, 1, lin.shape[2]) for a in (mean, inv))
    return (lin - mean) * inv * np.asarray(bn_weight, np.float64) + np.asarray(bn_bias, np.float64)


def head_backward_ref(d_out, feat, weight, bn_weight, bn_bias, lin, mean=None, invstd=None, running_mean=None,
                      running_var=None, eps=1e-5, mask=None):
    """the entry's own inputs (fp32 arrays, widened here) -> (d_feat, d_weight, d_bias, d_bn_weight, d_bn_bias, dlin)"""
    w = lambda a: np.asarray(a, np.float64)          # noqa: E731
    d_out, feat, weight, g, be, lin = (w(a) for a in (d_out, feat, weight, bn_weight, bn_bias, lin))
    T, B, C = lin.shape
    train = mean is not None
    if train:
        assert invstd is not None and running_mean is None and running_var is None
        mu, inv = w(mean).reshape(T, 1, C), w(invstd).reshape(T, 1, C)
    else:
        assert invstd is None and running_mean is not None and running_var is not None
        mu = w(running_mean).reshape(1, 1, C)
        inv = (1.0 / np.sqrt(w(running_var) + np.float64(np.float32(eps)))).reshape(1, 1, C)
    xhat = (lin - mu) * inv
    y = xhat * g + be
    dy = d_out * (1.0 if mask is None else w(mask)) * (y > 0)
    dbeta_t = dy.sum(1, keepdims=True)
    dgamma_t = (dy * xhat).sum(1, keepdims=True)
    if train:
        dlin = inv * g * (dy - dbeta_t / B - xhat * dgamma_t / B)
    else:
        dlin = dy * g * inv
    flat = dlin.reshape(T * B, C)
    d_weight = flat.T @ feat.reshape(T * B, -1)
    d_feat = (flat @ weight).reshape(feat.shape)
    return d_feat, d_weight, flat.sum(0), dgamma_t.sum((0, 1)), dbeta_t.sum((0, 1)), dlin


def draw_case(shape, train, with_mask, seed):
    """fp32 inputs of the entry for (T, B, K, C), drawn with a fixed seed.  linear_out is an input of its own (the formulas
    do not need mean / inv to be its statistics); every element whose float64 BatchNorm output lies within MARGIN of 0 is
    redrawn until none is left, so no ReLU decision hangs on a rounding."""
    T, B, K, C = shape
    rng = np.random.default_rng(seed)
    u = lambda *s: rng.uniform(-1.0, 1.0, s).astype(np.float32)          # noqa: E731
    d = dict(d_out=u(T, B, C), feat=u(T, B, K), weight=(u(C, K) * 0.25).astype(np.float32),
             bn_weight=(u(C) * 0.5 + 1.0).astype(np.float32), bn_bias=(u(C) * 0.2).astype(np.float32),
             lin=(u(T, B, C) * 2.0).astype(np.float32), eps=1e-5)
    if train:
        d["mean"], d["invstd"] = (u(T, C) * 0.3).astype(np.float32), (u(T, C) * 0.4 + 1.0).astype(np.float32)
        mean, inv = d["mean"], d["invstd"]
    else:
        d["running_mean"], d["running_var"] = (u(C) * 0.3).astype(np.float32), (u(C) * 0.4 + 1.0).astype(np.float32)
        mean = d["running_mean"]
        inv = 1.0 / np.sqrt(d["running_var"].astype(np.float64) + np.float64(np.float32(1e-5)))
    d["mask"] = ((u(T, B, C) > -0.4).astype(np.float32) / np.float32(0.7)) if with_mask else None
    for _ in range(100):
        close = np.abs(bn_output(d["lin"], d["bn_weight"], d["bn_bias"], mean, inv)) < MARGIN
        if not close.any():
            break
        d["lin"][close] = (u(int(close.sum())) * 2.0).astype(np.float32)
    assert not (np.abs(bn_output(d["lin"], d["bn_weight"], d["bn_bias"], mean, inv)) < MARGIN).any()
    return d
