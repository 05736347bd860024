"""Seeded synthetic inputs shared by tests, smoke and bench (SURVEY 8d generator)."""
import numpy as np
import torch


def synth_noblank(seed, T, B, C, S, var_T=False, int64=False):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(T, B, C, generator=g)
    L = torch.randint(1, S + 1, (B,), generator=g)
    lab = torch.randint(0, C, (B, S), generator=g, dtype=torch.int32)
    lab[torch.arange(S)[None, :] >= L[:, None]] = -1
    if var_T:
        Tb = torch.maximum(torch.randint(min(S, T), T + 1, (B,), generator=g), L)
    else:
        Tb = torch.full((B,), T, dtype=torch.int64)
    return x, (lab.long() if int64 else lab), Tb.long(), L.long()


def synth_binary(seed, T, B, C, S, var_T=False, density=0.05):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(T, B, C, generator=g)
    L = torch.randint(1, S + 1, (B,), generator=g)
    y = (torch.rand(B, S, C, generator=g) < density).float()
    y[(torch.arange(S)[None, :] >= L[:, None])] = 0.0
    if var_T:
        Tb = torch.maximum(torch.randint(min(S, T), T + 1, (B,), generator=g), L)
    else:
        Tb = torch.full((B,), T, dtype=torch.int64)
    return x, y, Tb.long(), L.long()


def synth_blank(seed, T, B, C, S, var_T=False):
    g = torch.Generator().manual_seed(seed)
    lp = torch.randn(T, B, C, generator=g).log_softmax(2)
    tgt = torch.randint(1, C, (B, S), generator=g)
    L = torch.randint(1, S + 1, (B,), generator=g)
    if var_T:
        Tb = torch.randint(min(2 * S + 1, T), T + 1, (B,), generator=g)
    else:
        Tb = torch.full((B,), T, dtype=torch.int64)
    return lp, tgt, Tb.long(), L.long()


def np_(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


NOBLANK_PLAN_FIELDS = ("family", "n4", "n2", "nt", "ps", "ch", "dual", "K", "glb", "grid", "lds", "next_round", "koff")
NOBLANK_PLAN_FAMILIES = ("unsupported", "r16", "km", "xr", "pipelined", "fused")


def noblank_plan_entry():
    """`ctc_amd_debug_noblank_plan` of the diagnostics build (built on first use; no GPU needed), bound once for the tests
    that ask which kernel a no-blank call gets -> call(T, B, C, S, dtype, st, sb, x_low, grad_low, want_grad, want_gamma,
    smooth, cus, sw) -> {field: value} of NOBLANK_PLAN_FIELDS"""
    import ctypes
    from ctc_amd import build
    fn = ctypes.CDLL(build.build_diag()).ctc_amd_debug_noblank_plan
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_int] * 5 + [ctypes.c_int64] * 2 + [ctypes.c_uint] * 2 + [ctypes.c_int] * 5 + \
        [ctypes.POINTER(ctypes.c_int64)]
    out = (ctypes.c_int64 * len(NOBLANK_PLAN_FIELDS))()

    def call(T, B, C, S, dtype, st, sb, x_low, grad_low, want_grad, want_gamma, smooth, cus, sw):
        rc = fn(T, B, C, S, dtype, st, sb, x_low, grad_low, int(want_grad), int(want_gamma), int(smooth), cus, sw, out)
        assert rc == 0, (T, B, C, S, dtype, st, sb, x_low, grad_low, want_grad, want_gamma, smooth, cus, sw)
        return dict(zip(NOBLANK_PLAN_FIELDS, out))
    return call


BINARY_PLAN_FIELDS = ("family", "K", "SP", "ch", "wt", "Tpad", "pd", "grid", "lds")
BINARY_PLAN_FAMILIES = ("unsupported", "flow", "pipe", "mfma", "fused")


def binary_plan_entry():
    """`ctc_amd_debug_binary_plan` of the diagnostics build (built on first use; no GPU needed), bound once for the tests
    that ask which kernel a binary call gets -> call(T, B, C, S, dtype, want_gamma, sw) -> {field: value} of
    BINARY_PLAN_FIELDS"""
    import ctypes
    from ctc_amd import build
    fn = ctypes.CDLL(build.build_diag()).ctc_amd_debug_binary_plan
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_int] * 7 + [ctypes.POINTER(ctypes.c_int64)]
    out = (ctypes.c_int64 * len(BINARY_PLAN_FIELDS))()

    def call(T, B, C, S, dtype, want_gamma, sw):
        rc = fn(T, B, C, S, dtype, int(want_gamma), sw, out)
        assert rc == 0, (T, B, C, S, dtype, want_gamma, sw)
        return dict(zip(BINARY_PLAN_FIELDS, out))
    return call
