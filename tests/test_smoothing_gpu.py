"""The label-smoothed no-blank loss, noblank_ctc_loss(..., label_smoothing=lam), on the MI355X: every form of the
four-rows-per-wave kernel (the only one that carries the smoothed emission) on a trained model's peaks (`aligned`), peaks
on the wrong class (`wrongpeak`), masked logits (`masked`), exact ties (`ties`) and a softmax-invariant common offset of
3.0e4 (`offset`), at lam = 0.9, 0.5, 1 / (C + 1) (a = 0) and 0 (a = -1 / C < 0) -- `masked` at 0.9 and 0.5 only: lam = 0
together with -inf asks for -inf + inf and is left undefined -- through the public Python API alone.  The cases and the
float64 reference are those of tests/smoothing_ref.py; tests/test_smoothing_ref.py checks them without a GPU.

The contract: a live row with a -inf logit gives every state of that row e = -inf; a sample whose nll
reaches 1e12 -- through such a row, or through finite pad logits whose b sum_n lp[n] alone carries it there -- has no
alignment: nll >= 1e12, never NaN, every gradient row exactly 0.  Everywhere else float64 decides.

Per case (path x regime x lam): nll >= 1e12 exactly on the reference's infeasible samples and within 1e-5 relative
elsewhere; the gradient finite, exactly 0 beyond T_b, on every row of an infeasible sample and at every infinite logit;
its error over the feasible samples within max(plain, 2 err32) (plain = the bound of test_noblank_vs_oracle_shapes at
that B, err32 = the error of the float32 port of oracle/ctc_numpy with label_smoothing on the same inputs); live rows of
B * grad sum to 0 within 1e-5; float(loss) = the float32 mean of the returned nll within 1e-6 wherever all samples are
feasible; a forward-only call gives the same nll (bits on r16_ps, 2e-6 relative elsewhere); two calls give equal bits.
Then: finite pad logits alone (the chains keep their mass); lam = 1 is the plain call bit for bit; two-byte logits keep
the contract of tests/test_lowp_gpu.py; the in-launch batch loss sum against the float64 mean; a retained graph's second
backward; one captured step.

Measured on an MI355X (gfx950), the library as this file's commit leaves it (nll_rel against max(1, |nll|); the
forward-only call and the second call as asserted above, r16_ps bit for bit on all 520 samples).  Samples without an
alignment report nll = 1e13 (no mass in the chains) or +inf (a -inf logit in a live row: the row constant).

    path-regime-lam                  err        err32      bound      nll_rel
    r16-aligned-lam0.9               3.6e-08    8.6e-07    1.0e-04    2.74e-07
    r16-aligned-lam0.5               3.6e-08    1.7e-06    1.0e-04    8.34e-08
    r16-aligned-lam1/(C+1)           4.0e-08    4.5e-08    1.0e-04    1.68e-07
    r16-aligned-lam0                 3.8e-08    3.5e-07    1.0e-04    9.19e-08
    r16-wrongpeak-lam0.9             1.4e-07    3.3e-05    1.0e-04    5.08e-08
    r16-wrongpeak-lam0.5             5.7e-08    1.7e-05    1.0e-04    4.36e-08
    r16-wrongpeak-lam1/(C+1)         3.9e-08    4.0e-08    1.0e-04    1.29e-07
    r16-wrongpeak-lam0               3.2e-08    2.5e-06    1.0e-04    5.34e-08
    r16-masked-lam0.9                1.9e-08    2.2e-05    1.0e-04    7.49e-08
    r16-masked-lam0.5                1.0e-08    2.2e-05    1.0e-04    7.72e-08
    r16-ties-lam0.9                  1.7e-08    1.5e-06    1.0e-04    9.78e-08
    r16-ties-lam0.5                  1.1e-08    3.9e-07    1.0e-04    1.64e-07
    r16-ties-lam1/(C+1)              1.9e-09    3.0e-09    1.0e-04    1.40e-07
    r16-ties-lam0                    1.8e-09    4.8e-08    1.0e-04    5.94e-08
    r16-offset-lam0.9                3.8e-08    5.7e-07    1.0e-04    2.86e-07
    r16-offset-lam0.5                5.1e-08    1.4e-06    1.0e-04    1.39e-07
    r16-offset-lam1/(C+1)            4.3e-08    4.7e-08    1.0e-04    1.33e-07
    r16-offset-lam0                  3.3e-08    3.6e-07    1.0e-04    9.13e-08
    r16_n4-aligned-lam0.9            4.5e-08    1.0e-06    1.0e-04    2.90e-07
    r16_n4-aligned-lam0.5            4.7e-08    1.2e-06    1.0e-04    1.64e-07
    r16_n4-aligned-lam1/(C+1)        4.5e-08    7.5e-08    1.0e-04    1.16e-07
    r16_n4-aligned-lam0              4.3e-08    1.1e-07    1.0e-04    1.39e-07
    r16_n4-wrongpeak-lam0.9          3.4e-08    4.4e-05    1.0e-04    9.22e-08
    r16_n4-wrongpeak-lam0.5          2.7e-08    1.7e-05    1.0e-04    3.99e-08
    r16_n4-wrongpeak-lam1/(C+1)      2.8e-08    3.1e-08    1.0e-04    5.24e-08
    r16_n4-wrongpeak-lam0            3.0e-08    5.7e-07    1.0e-04    7.13e-08
    r16_n4-masked-lam0.9             2.2e-08    4.4e-05    1.0e-04    2.80e-08
    r16_n4-masked-lam0.5             1.3e-08    1.2e-05    1.0e-04    4.36e-08
    r16_n4-ties-lam0.9               9.2e-09    2.5e-06    1.0e-04    1.77e-07
    r16_n4-ties-lam0.5               8.9e-09    1.4e-06    1.0e-04    5.52e-08
    r16_n4-ties-lam1/(C+1)           1.4e-18    1.4e-18    1.0e-04    7.81e-08
    r16_n4-ties-lam0                 1.7e-10    2.2e-08    1.0e-04    6.83e-08
    r16_n4-offset-lam0.9             5.3e-08    7.3e-07    1.0e-04    2.55e-07
    r16_n4-offset-lam0.5             6.3e-08    1.8e-06    1.0e-04    1.57e-07
    r16_n4-offset-lam1/(C+1)         5.1e-08    3.7e-08    1.0e-04    1.61e-07
    r16_n4-offset-lam0               4.9e-08    6.6e-08    1.0e-04    8.16e-08
    r16_n2-aligned-lam0.9            5.0e-08    5.1e-07    1.0e-04    2.47e-07
    r16_n2-aligned-lam0.5            4.1e-08    1.4e-06    1.0e-04    6.30e-08
    r16_n2-aligned-lam1/(C+1)        4.3e-08    5.4e-08    1.0e-04    1.05e-07
    r16_n2-aligned-lam0              3.7e-08    1.2e-07    1.0e-04    1.00e-07
    r16_n2-wrongpeak-lam0.9          6.9e-08    2.2e-05    1.0e-04    7.45e-08
    r16_n2-wrongpeak-lam0.5          2.8e-08    1.3e-05    1.0e-04    1.01e-07
    r16_n2-wrongpeak-lam1/(C+1)      2.7e-08    3.8e-08    1.0e-04    1.02e-07
    r16_n2-wrongpeak-lam0            3.2e-08    1.3e-06    1.0e-04    5.55e-08
    r16_n2-masked-lam0.9             1.4e-08    4.7e-05    1.0e-04    1.47e-09
    r16_n2-masked-lam0.5             9.3e-09    1.3e-05    1.0e-04    2.55e-08
    r16_n2-ties-lam0.9               1.3e-08    1.3e-06    1.0e-04    2.60e-07
    r16_n2-ties-lam0.5               9.6e-09    5.3e-07    1.0e-04    1.54e-07
    r16_n2-ties-lam1/(C+1)           6.9e-19    6.9e-19    1.0e-04    1.76e-07
    r16_n2-ties-lam0                 5.6e-10    5.1e-08    1.0e-04    9.77e-08
    r16_n2-offset-lam0.9             5.7e-08    5.5e-07    1.0e-04    3.45e-07
    r16_n2-offset-lam0.5             5.6e-08    1.5e-06    1.0e-04    1.15e-07
    r16_n2-offset-lam1/(C+1)         5.1e-08    5.0e-08    1.0e-04    3.71e-08
    r16_n2-offset-lam0               5.9e-08    1.4e-07    1.0e-04    1.07e-07
    r16_c158-aligned-lam0.9          5.7e-08    1.4e-06    1.0e-04    3.09e-07
    r16_c158-aligned-lam0.5          5.6e-08    4.4e-06    1.0e-04    3.55e-08
    r16_c158-aligned-lam1/(C+1)      5.1e-08    7.4e-08    1.0e-04    7.49e-08
    r16_c158-aligned-lam0            5.9e-08    6.6e-08    1.0e-04    6.65e-08
    r16_c158-wrongpeak-lam0.9        1.4e-07    8.8e-05    1.8e-04    6.40e-08
    r16_c158-wrongpeak-lam0.5        1.0e-07    3.6e-05    1.0e-04    7.97e-08
    r16_c158-wrongpeak-lam1/(C+1)    5.2e-08    3.6e-08    1.0e-04    6.53e-08
    r16_c158-wrongpeak-lam0          5.1e-08    3.2e-07    1.0e-04    1.52e-07
    r16_c158-masked-lam0.9           3.3e-08    2.9e-05    1.0e-04    1.16e-08
    r16_c158-masked-lam0.5           1.3e-08    2.4e-05    1.0e-04    9.38e-08
    r16_c158-ties-lam0.9             1.2e-08    4.7e-06    1.0e-04    9.83e-08
    r16_c158-ties-lam0.5             6.1e-09    2.0e-06    1.0e-04    1.11e-07
    r16_c158-ties-lam1/(C+1)         1.2e-10    1.9e-10    1.0e-04    7.07e-08
    r16_c158-ties-lam0               1.3e-10    3.0e-08    1.0e-04    1.03e-07
    r16_c158-offset-lam0.9           4.9e-08    1.3e-06    1.0e-04    3.80e-07
    r16_c158-offset-lam0.5           5.6e-08    3.1e-06    1.0e-04    6.67e-08
    r16_c158-offset-lam1/(C+1)       5.4e-08    7.1e-08    1.0e-04    6.13e-08
    r16_c158-offset-lam0             5.2e-08    8.8e-08    1.0e-04    1.11e-07
    r16_s31-aligned-lam0.9           6.1e-08    1.4e-06    1.0e-04    3.66e-07
    r16_s31-aligned-lam0.5           4.6e-08    2.3e-06    1.0e-04    1.17e-07
    r16_s31-aligned-lam1/(C+1)       3.9e-08    4.9e-08    1.0e-04    1.41e-07
    r16_s31-aligned-lam0             4.6e-08    8.0e-07    1.0e-04    9.37e-08
    r16_s31-wrongpeak-lam0.9         2.0e-07    4.4e-05    1.0e-04    7.70e-08
    r16_s31-wrongpeak-lam0.5         4.7e-08    2.4e-05    1.0e-04    9.76e-08
    r16_s31-wrongpeak-lam1/(C+1)     3.3e-08    3.0e-08    1.0e-04    8.82e-08
    r16_s31-wrongpeak-lam0           3.2e-08    8.1e-06    1.0e-04    8.49e-08
    r16_s31-masked-lam0.9            2.7e-08    4.6e-05    1.0e-04    1.40e-07
    r16_s31-masked-lam0.5            1.0e-08    5.8e-05    1.2e-04    2.09e-08
    r16_s31-ties-lam0.9              2.2e-08    1.7e-06    1.0e-04    5.50e-08
    r16_s31-ties-lam0.5              1.2e-08    2.1e-06    1.0e-04    1.21e-07
    r16_s31-ties-lam1/(C+1)          1.9e-09    0.0e+00    1.0e-04    7.91e-08
    r16_s31-ties-lam0                2.8e-09    1.3e-07    1.0e-04    1.03e-07
    r16_s31-offset-lam0.9            5.6e-08    1.0e-06    1.0e-04    3.23e-07
    r16_s31-offset-lam0.5            3.7e-08    2.8e-06    1.0e-04    1.03e-07
    r16_s31-offset-lam1/(C+1)        4.4e-08    5.8e-08    1.0e-04    8.48e-08
    r16_s31-offset-lam0              4.1e-08    5.5e-07    1.0e-04    7.99e-08
    r16_t168-aligned-lam0.9          6.2e-08    4.1e-06    1.0e-04    3.30e-07
    r16_t168-aligned-lam0.5          4.6e-08    3.1e-05    1.0e-04    6.95e-08
    r16_t168-aligned-lam1/(C+1)      3.9e-08    4.9e-08    1.0e-04    8.39e-08
    r16_t168-aligned-lam0            4.2e-08    1.1e-05    1.0e-04    1.30e-07
    r16_t168-wrongpeak-lam0.9        3.6e-07    1.5e-04    3.0e-04    9.82e-08
    r16_t168-wrongpeak-lam0.5        5.1e-08    5.2e-05    1.1e-04    1.16e-07
    r16_t168-wrongpeak-lam1/(C+1)    3.2e-08    4.8e-08    1.0e-04    9.56e-08
    r16_t168-wrongpeak-lam0          3.9e-08    3.5e-05    1.0e-04    1.48e-07
    r16_t168-masked-lam0.9           3.7e-08    7.1e-04    1.4e-03    2.19e-07
    r16_t168-masked-lam0.5           1.7e-08    7.8e-04    1.6e-03    3.35e-08
    r16_t168-ties-lam0.9             2.1e-08    3.0e-05    1.0e-04    1.70e-07
    r16_t168-ties-lam0.5             1.2e-08    1.4e-05    1.0e-04    1.28e-07
    r16_t168-ties-lam1/(C+1)         3.7e-09    5.6e-18    1.0e-04    1.34e-07
    r16_t168-ties-lam0               6.5e-09    1.2e-06    1.0e-04    1.39e-07
    r16_t168-offset-lam0.9           5.5e-08    8.1e-06    1.0e-04    2.97e-07
    r16_t168-offset-lam0.5           4.3e-08    1.3e-05    1.0e-04    5.30e-08
    r16_t168-offset-lam1/(C+1)       4.1e-08    5.1e-08    1.0e-04    8.75e-08
    r16_t168-offset-lam0             3.4e-08    1.2e-05    1.0e-04    5.93e-08
    r16_ps-aligned-lam0.9            6.4e-10    9.9e-09    2.0e-06    5.17e-07
    r16_ps-aligned-lam0.5            5.1e-10    2.8e-08    2.0e-06    1.81e-07
    r16_ps-aligned-lam1/(C+1)        5.2e-10    6.1e-10    2.0e-06    2.08e-07
    r16_ps-aligned-lam0              5.5e-10    1.1e-08    2.0e-06    1.97e-07
    r16_ps-wrongpeak-lam0.9          6.3e-09    5.1e-07    2.0e-06    1.34e-07
    r16_ps-wrongpeak-lam0.5          2.0e-09    3.2e-07    2.0e-06    1.63e-07
    r16_ps-wrongpeak-lam1/(C+1)      3.8e-10    5.0e-10    2.0e-06    2.30e-07
    r16_ps-wrongpeak-lam0            3.6e-10    6.9e-08    2.0e-06    1.72e-07
    r16_ps-masked-lam0.9             4.4e-10    8.7e-07    2.0e-06    2.25e-07
    r16_ps-masked-lam0.5             2.2e-10    9.9e-07    2.0e-06    1.64e-07
    r16_ps-ties-lam0.9               2.4e-10    1.7e-08    2.0e-06    1.77e-07
    r16_ps-ties-lam0.5               1.8e-10    1.3e-08    2.0e-06    1.64e-07
    r16_ps-ties-lam1/(C+1)           1.5e-11    2.9e-11    2.0e-06    1.96e-07
    r16_ps-ties-lam0                 3.5e-11    7.5e-10    2.0e-06    1.76e-07
    r16_ps-offset-lam0.9             6.2e-10    1.0e-08    2.0e-06    5.22e-07
    r16_ps-offset-lam0.5             5.3e-10    2.6e-08    2.0e-06    1.47e-07
    r16_ps-offset-lam1/(C+1)         5.1e-10    6.7e-10    2.0e-06    2.24e-07
    r16_ps-offset-lam0               4.5e-10    1.2e-08    2.0e-06    1.62e-07
    r16-aligned-lam1                 4.2e-08    5.7e-08    1.0e-04    1.87e-06
    r16_n4-aligned-lam1              4.4e-08    1.1e-07    1.0e-04    8.32e-07
    r16_n2-aligned-lam1              5.2e-08    1.0e-07    1.0e-04    3.86e-07
    r16_c158-aligned-lam1            4.9e-08    3.1e-07    1.0e-04    4.10e-07
    r16_s31-aligned-lam1             5.1e-08    1.2e-07    1.0e-04    1.66e-06
    r16_t168-aligned-lam1            4.6e-08    5.4e-07    1.0e-04    5.54e-06
    r16_ps-aligned-lam1              5.6e-10    1.7e-09    2.0e-06    2.75e-06

    two-byte logits, lam = 0.9     bf16 / f16 / f16 with +-65504: nll, loss and gradient bits equal those of the fp32 call
    aligned, ties                  equal on all seven paths, every sample feasible
    masked                         equal on all seven paths; samples without an alignment: 4 of 5 (416 of 520 on r16_ps)
    batch loss sum, lam = 0.9      |loss - float64 mean| / mean: B = 1 6.6e-08, B = 3 4.8e-08, B = 257 5.7e-08, B = 520 5.4e-08

Before the fixes of this commit (the library as its parent left it) 63 of the 211 cases failed here:
  * `masked`, all 14 loss cases and all 21 two-byte cases: the samples with a -inf logit in a live row whose chains keep
    mass (kinds a and b of tests/lattice_inputs_ref.make_case) reported nll = +inf -- the row constant b sum_n lp[n] --
    with gradient rows of (1 - b) softmax - a occupancy - b, and -b / B at the -inf logit itself ("sample N has no
    alignment", "gradient at an infinite logit");
  * `offset`, all 28 cases: nll off by 1.5e-5 ... 1.1e-3 of max(1, |nll|) (r16_ps at lam = 0.9: 1.09e-3; the gradient was
    right, 6e-8).  Summing x - max in place of x alone did not cure it (r16 at lam = 0.9: 3.0e-4 after, 3.5e-4 before):
    most of the error is the rounding of -max log2e in front of the row's exponentials, which the row's log-sum-exp
    carried (noblank_r16.hpp, P1b).  5.2e-7 at most now.
  * a <= 0 (lam = 1 / (C + 1) and 0) passed as it was on `aligned`, `wrongpeak` and `ties`: the chains take emissions with
    positive exponents.  The clamp from above that this commit adds only guards the int exponent against a masked label
    class at a <= 0, which stays outside the contract.  lam = 1 gave the plain call's bits before and after.
The fixes: DESIGN.md 3.1 "Label-smoothed emission", 4 "Masked logits".  What the assertions hold in place, each seen on the
MI355X with a library built from a scratch copy (wrong numbers only):
  * the -b constant of the smoothed gradient dropped: test_loss_and_gradient fails on 126 of its 133 cases, at the
    gradient bound (125) or at the row sums (1, off by 0.1) -- all but the seven lam = 1 cases, where b = 0;
  * a = lam in place of lam - b: the same 126 at the nll tolerance, and test_batch_loss_sum at all four B;
  * without the rule for a -inf row (the workers' look at the row constants): exactly the 35 `masked` cases above, loss
    and two-byte, and nothing else.
"""
import numpy as np
import pytest
import torch

from tests.helpers import np_
from tests.lattice_inputs_ref import NLL_RTOL, NO_ALIGNMENT, plain_bound
from tests.smoothing_ref import CASES, PATHS, REGIMES, batch_case, case_id, inputs, port, reference, smoothed_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    import ctc_amd  # noqa: F401  (raises if libctc_amd.so is missing)
    return torch.device("cuda:0")


def run_loss(dev, args, lam, grad=True, smoothed=True):
    """one call -> nll, loss, grad as numpy"""
    import ctc_amd
    x, lab, Tb, L = (a.to(dev) for a in args)
    x.requires_grad_(grad)
    kw = {"label_smoothing": lam} if smoothed else {}
    loss, nll = ctc_amd.noblank_ctc_loss(x, lab, Tb, L, **kw)
    if grad:
        loss.backward()
    torch.cuda.synchronize()
    return {"nll": np_(nll), "loss": np_(loss.detach()), "grad": np_(x.grad) if grad else None}


def check_nll(nll, ref, what):
    """>= 1e12 exactly on the samples without an alignment, never NaN, within 1e-5 relative on the others"""
    fin = ref["fin"]
    nll = nll.astype(np.float64)
    assert not np.isnan(nll).any(), what
    assert np.array_equal(nll >= NO_ALIGNMENT, ~fin), "%s: nll %r, feasible %r" % (what, nll[:10], fin[:10])
    nerr = float((np.abs(nll[fin] - ref["nll"][fin]) / np.maximum(1.0, np.abs(ref["nll"][fin]))).max())
    if not fin.all():
        print("smoothing %s: nll without an alignment %s" % (what, sorted(set("%.3g" % v for v in nll[~fin]))))
    assert nerr <= NLL_RTOL, "%s: nll off by %.3e relative" % (what, nerr)
    return nerr


def bits(a):
    return a.view(np.int32)


# ---- 1. loss and gradient: every form, regime and lam -----------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_loss_and_gradient(dev, case):
    path, regime, lam = case
    ref = reference(*case)
    x, _, Tb, _ = ref["inputs"]
    T, B, C = x.shape
    fin, xn = ref["fin"], np_(x)
    r = run_loss(dev, ref["inputs"], lam)
    g32 = r["grad"]
    g = g32.astype(np.float64)
    err = float(np.abs(g[:, fin] - ref["grad"][:, fin]).max())
    nll64 = r["nll"].astype(np.float64)
    nrel = float((np.abs(nll64[fin] - ref["nll"][fin]) / np.maximum(1.0, np.abs(ref["nll"][fin]))).max())
    print("smoothing %s: err %.3e err32 %.3e bound %.3e nll_rel %.2e" % (case_id(case), err, ref["err32"], ref["bound"], nrel))
    check_nll(r["nll"], ref, case_id(case))
    # the exact parts of the gradient
    assert np.isfinite(g32).all()
    for b in range(B):
        assert np.abs(g32[int(Tb[b]):, b]).max(initial=0.0) == 0.0, "sample %d beyond T_b" % b
        if not fin[b]:
            assert np.abs(g32[:, b]).max() == 0.0, "sample %d has no alignment" % b
    assert (g32[np.isinf(xn)] == 0.0).all(), "gradient at an infinite logit"
    # accuracy: neither term of the bound comes from the kernel
    assert err <= ref["bound"], (err, ref["bound"])
    rows = np.abs(g.sum(2) * B)                               # (1 - b) softmax - a occupancy - b sums to 0
    assert rows[:, fin].max() <= 1e-5
    if fin.all():
        mean32 = float(r["nll"].mean(dtype=np.float32))
        assert abs(float(r["loss"]) - mean32) <= 1e-6 * max(1.0, abs(mean32)), (float(r["loss"]), mean32)
    # a forward-only call
    f = run_loss(dev, ref["inputs"], lam, grad=False)
    check_nll(f["nll"], ref, case_id(case) + " forward only")
    if path == "r16_ps":
        assert np.array_equal(bits(f["nll"]), bits(r["nll"])), "forward-only nll bits"
    else:
        assert (np.abs(f["nll"][fin] - r["nll"][fin]) <= 2e-6 * np.maximum(1.0, np.abs(r["nll"][fin]))).all()
    # two calls, equal bits
    again = run_loss(dev, ref["inputs"], lam)
    assert np.array_equal(bits(again["nll"]), bits(r["nll"]))
    assert np.array_equal(bits(again["loss"]), bits(r["loss"]))
    assert np.array_equal(bits(again["grad"]), bits(g32))


@pytest.mark.parametrize("path", ["r16", "r16_ps"])
def test_finite_pad_logits_alone_leave_no_alignment(dev, path):
    """a pad column (-1e30, finite) on every other sample, outside every transcript: the chains keep their mass, and
    b sum_n lp[n] alone carries nll past 1e12 -- no alignment, zero gradient rows; the samples in between are untouched"""
    x, lab, Tb, L = inputs(path, "aligned")[:4]
    C = x.shape[2]
    x, lab = x.clone(), torch.where(lab >= 0, lab % (C - 1), lab)
    x[:, 0::2, C - 1] = -1.0e30
    ref = smoothed_ref(x, lab, Tb, L, 0.9)
    padded = np.arange(x.shape[1]) % 2 == 0
    assert np.array_equal(ref["fin"], ~padded) and np.isfinite(np_(x)).all()
    r = run_loss(dev, (x, lab, Tb, L), 0.9)
    check_nll(r["nll"], ref, path + " pad column")
    assert np.isfinite(r["nll"]).all()
    assert np.abs(r["grad"][:, padded]).max() == 0.0
    p32 = port(x, lab, Tb, L, 0.9, np.float32)["grad"]
    bound = max(plain_bound("noblank", x.shape[1]), 2.0 * float(np.abs(p32[:, ~padded] - ref["grad"][:, ~padded]).max()))
    assert np.abs(r["grad"][:, ~padded] - ref["grad"][:, ~padded]).max() <= bound


# ---- 2. lam = 1 is the plain loss -------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
def test_lam_one_is_the_plain_call_bit_for_bit(dev, path):
    for regime in REGIMES:
        args = inputs(path, regime)[:4]
        for grad in (True, False):
            s = run_loss(dev, args, 1.0, grad=grad)
            p = run_loss(dev, args, None, grad=grad, smoothed=False)
            what = "%s-%s grad=%s" % (path, regime, grad)
            assert np.array_equal(bits(s["nll"]), bits(p["nll"])), what
            assert np.array_equal(bits(s["loss"]), bits(p["loss"])), what
            if grad:
                assert np.array_equal(bits(s["grad"]), bits(p["grad"])), what


# ---- 3. two-byte logits -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["bf16", "f16", "f16-65504"])
@pytest.mark.parametrize("regime", ["aligned", "masked", "ties"])
@pytest.mark.parametrize("path", PATHS)
def test_two_byte_logits(dev, path, regime, form):
    """the contract of tests/test_lowp_gpu.py and test_two_byte_masked_logits at lam = 0.9: nll is bitwise that of the
    fp32 call on x.float(), the gradient bitwise that call's gradient rounded once to the dtype (fp16 turns PAD_LOGIT into
    -inf; +-65504 is its range)"""
    import ctc_amd
    dtype = torch.bfloat16 if form == "bf16" else torch.float16
    x, lab, Tb, L = inputs(path, regime)[:4]
    x = x.clone()
    if form == "f16-65504":
        g = torch.Generator().manual_seed(5)
        hit = (torch.rand(x.shape, generator=g) < 0.05) & torch.isfinite(x) & (x > -1e3)
        x[hit] = torch.where(torch.rand(x.shape, generator=g) < 0.5, 65504.0, -65504.0)[hit]
    lab, Tb, L = lab.to(dev), Tb.to(dev), L.to(dev)
    xl = x.to(dev, dtype).requires_grad_(True)
    xf = xl.detach().float().requires_grad_(True)
    out = []
    for leaf in (xl, xf):
        loss, nll = ctc_amd.noblank_ctc_loss(leaf, lab, Tb, L, label_smoothing=0.9)
        loss.backward()
        torch.cuda.synchronize()
        out.append((nll.detach(), loss.detach(), leaf.grad))
    (nll, loss, g), (nll32, loss32, g32) = out
    assert g.dtype == dtype and nll.dtype == torch.float32
    assert not bool(torch.isnan(nll).any())
    assert torch.equal(nll.view(torch.int32), nll32.view(torch.int32)), "nll"
    assert torch.equal(loss.view(torch.int32), loss32.view(torch.int32)), "loss"
    assert torch.equal(g.view(torch.int16), g32.to(dtype).view(torch.int16)), "grad"
    assert bool(torch.isfinite(g).all()) and bool((g[torch.isinf(xl.detach())] == 0).all())
    dead = nll >= NO_ALIGNMENT
    assert bool((g[:, dead] == 0).all()), "a sample without an alignment"
    if regime == "masked":
        assert bool(dead.any()) and not bool(dead.all())
    print("smoothing two-byte %s-%s-%s: nll, loss and gradient bits equal, %d of %d samples without an alignment"
          % (path, regime, form, int(dead.sum()), nll.numel()))


# ---- 4. the in-launch batch loss sum ----------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3, 257, 520])
def test_batch_loss_sum(dev, B):
    """(24, B, 10, 6) at lam = 0.9 (B = 520: the persistent form): the loss against the float64 mean of the float64 nll,
    within the nll's own tolerance, and against the float32 mean of the returned nll within 1e-6; with and without a
    gradient"""
    args = batch_case(B)
    ref = smoothed_ref(*args, 0.9)
    assert ref["fin"].all()
    mean64 = float(ref["nll"].mean())
    for grad in (True, False):
        r = run_loss(dev, args, 0.9, grad=grad)
        nrel = float((np.abs(r["nll"] - ref["nll"]) / np.maximum(1.0, np.abs(ref["nll"]))).max())
        print("smoothing batch sum B=%d grad=%s: loss %.9g float64 mean %.9g nll_rel %.2e" % (B, grad, float(r["loss"]), mean64, nrel))
        assert nrel <= NLL_RTOL
        assert abs(float(r["loss"]) - mean64) <= NLL_RTOL * max(1.0, abs(mean64))
        mean32 = float(r["nll"].mean(dtype=np.float32))
        assert abs(float(r["loss"]) - mean32) <= 1e-6 * max(1.0, abs(mean32))


# ---- 5. a retained graph: the second backward recomputes with the stored lam -------------------------------------------
@pytest.mark.parametrize("path", ["r16", "r16_ps"])
def test_retained_graph_recomputes_the_smoothed_gradient(dev, path):
    import ctc_amd
    x, lab, Tb, L = (a.to(dev) for a in inputs(path, "aligned")[:4])
    x.requires_grad_(True)
    loss, _ = ctc_amd.noblank_ctc_loss(x, lab, Tb, L, label_smoothing=0.5)
    y = 2.5 * loss
    y.backward(retain_graph=True)
    first = x.grad.clone()
    x.grad = None
    y.backward()                                              # recomputed by a second launch (_scaled_grad)
    torch.cuda.synchronize()
    assert torch.equal(x.grad.view(torch.int32), first.view(torch.int32)), "second backward"
    fresh = run_loss(dev, inputs(path, "aligned")[:4], 0.5)
    assert np.array_equal(bits(np_(first)), bits(fresh["grad"] * np.float32(2.5))), "2.5 x the gradient"
    plain = run_loss(dev, inputs(path, "aligned")[:4], None, smoothed=False)
    assert np.abs(np_(first) - plain["grad"] * np.float32(2.5)).max() > 1e-4 / x.shape[1]      # not the plain loss's


# ---- 6. graph capture -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["r16", "r16_ps"])
def test_graph_capture(dev, path):
    """one smoothed step (forward + backward) captured and replayed on new data: the eager bits"""
    import ctc_amd
    x, lab, Tb, L = (a.to(dev) for a in inputs(path, "aligned")[:4])
    xs = x.clone().requires_grad_(True)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                                # warm-up on a side stream (workspace, grads)
        for _ in range(2):
            xs.grad = None
            loss, nll = ctc_amd.noblank_ctc_loss(xs, lab, Tb, L, label_smoothing=0.9)
            loss.backward()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    xs.grad = None
    with torch.cuda.graph(g):
        loss, nll = ctc_amd.noblank_ctc_loss(xs, lab, Tb, L, label_smoothing=0.9)
        loss.backward()
    with torch.no_grad():
        xs.copy_(inputs(path, "wrongpeak")[0].to(dev))
    g.replay()
    torch.cuda.synchronize()
    got = (loss.detach().clone(), nll.clone(), xs.grad.clone())
    e = run_loss(dev, inputs(path, "wrongpeak")[:4], 0.9)
    assert np.array_equal(bits(np_(got[0])), bits(e["loss"])), "replayed loss"
    assert np.array_equal(bits(np_(got[1])), bits(e["nll"])), "replayed nll"
    assert np.array_equal(bits(np_(got[2])), bits(e["grad"])), "replayed grad"
