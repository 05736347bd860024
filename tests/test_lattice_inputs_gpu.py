"""The no-blank and the binary lattice on the MI355X on the inputs a real caller produces and `randn` at unit scale never
does -- a trained model's peaks (`aligned`), peaks on the wrong class (`wrongpeak`), masked logits (`masked`: -inf,
PAD_LOGIT = -1e30, -1e4 and samples that lose every alignment through their emissions alone; binary: +-inf, PAD_LOGIT,
+-100) and exact ties (`ties`) -- on every kernel the default dispatch can launch, through the public Python API alone.
The cases and the float64 reference that is defined at -inf are those of tests/lattice_inputs_ref.py;
tests/test_lattice_inputs_ref.py checks them without a GPU.

Per case of the loss (family x kernel x regime): nll is >= 1e12 exactly on the samples the reference calls infeasible and
within 1e-5 relative otherwise; the gradient is finite, exactly 0 beyond T_b, on every row of an infeasible sample and at
every infinite logit; over the feasible samples its error against float64 stays within max(plain, 2 err32), plain = the
bound of test_noblank_vs_oracle_shapes / test_binary_vs_oracle_shapes at that B, err32 = the error of the float32 port of
the reference (oracle/ctc_numpy) on the same inputs; live no-blank rows of B * grad sum to 0 within 1e-5; a forward-only
call gives the same nll (bit for bit on the streamed binary kernel, 2e-6 relative elsewhere); two calls give equal bits.
The read-outs: best path exactly the reference's on ties (ties stay), elsewhere the score within the existing bound and
the returned path attaining the float64 optimum; posteriors within max(2e-4, 2 err32_gamma), rows summing to 1, exactly 0
on masked cells and infeasible samples; token spans with the best path's bits, nll, frame_conf and the partition of
[0, T_b).  Two-byte logits on the r16 shapes keep the contract of tests/test_lowp_gpu.py on masked inputs.

Measured on an MI355X (gfx950), the library as this file's commit leaves it.  Loss and gradient (nll_rel against
max(1, |nll|); a forward-only call and a second call as asserted above, the persistent form r16_ps bit for bit on all 520
samples); then the read-outs (score bound = the relative bound x max(1, max |score|)) and the two-byte cases.  Samples
without an alignment report nll = 1e13 on r16, xr and the workspace lattice, multiples of 1e13 or 1e30 on the fused and
pipelined kernels, +inf from the token spans.

    family-path-regime             err        err32      err/err32  bound      max|grad_ref|  nll_rel
    noblank-r16-aligned            4.2e-08    5.7e-08    0.739      1.0e-04    1.3e-02        1.87e-06
    noblank-r16-wrongpeak          1.5e-07    7.3e-05    0.002      1.5e-04    2.0e-01        7.23e-08
    noblank-r16-masked             2.5e-08    2.4e-05    0.001      1.0e-04    2.0e-01        3.35e-08
    noblank-r16-ties               2.5e-08    8.1e-07    0.031      1.0e-04    1.8e-01        1.33e-07
    noblank-r16_n4-aligned         4.4e-08    1.1e-07    0.389      1.0e-04    4.6e-02        8.32e-07
    noblank-r16_n4-wrongpeak       3.0e-08    4.9e-05    0.001      1.0e-04    2.0e-01        5.26e-08
    noblank-r16_n4-masked          4.3e-08    5.5e-05    0.001      1.1e-04    2.0e-01        1.16e-07
    noblank-r16_n4-ties            1.1e-08    1.7e-06    0.006      1.0e-04    2.0e-01        6.24e-08
    noblank-r16_n2-aligned         5.2e-08    1.0e-07    0.508      1.0e-04    2.2e-02        3.86e-07
    noblank-r16_n2-wrongpeak       3.7e-08    2.4e-05    0.002      1.0e-04    2.0e-01        9.23e-08
    noblank-r16_n2-masked          3.3e-08    2.6e-05    0.001      1.0e-04    2.0e-01        6.69e-08
    noblank-r16_n2-ties            1.2e-08    1.4e-06    0.008      1.0e-04    1.9e-01        1.70e-07
    noblank-r16_c158-aligned       4.9e-08    3.1e-07    0.159      1.0e-04    1.0e-01        4.10e-07
    noblank-r16_c158-wrongpeak     5.6e-08    9.8e-05    0.001      2.0e-04    2.0e-01        7.78e-08
    noblank-r16_c158-masked        3.4e-08    5.3e-05    0.001      1.1e-04    2.0e-01        1.04e-07
    noblank-r16_c158-ties          1.3e-08    5.2e-06    0.002      1.0e-04    2.0e-01        1.28e-07
    noblank-r16_s31-aligned        5.1e-08    1.2e-07    0.439      1.0e-04    1.8e-02        1.66e-06
    noblank-r16_s31-wrongpeak      1.5e-07    7.3e-05    0.002      1.5e-04    2.0e-01        4.47e-08
    noblank-r16_s31-masked         3.0e-08    4.9e-05    0.001      1.0e-04    2.0e-01        1.39e-07
    noblank-r16_s31-ties           1.9e-08    4.6e-06    0.004      1.0e-04    1.8e-01        4.40e-08
    noblank-r16_t168-aligned       4.6e-08    5.4e-07    0.085      1.0e-04    8.5e-03        5.54e-06
    noblank-r16_t168-wrongpeak     3.4e-07    9.8e-05    0.003      2.0e-04    2.0e-01        6.77e-08
    noblank-r16_t168-masked        4.7e-08    9.7e-05    0.000      1.9e-04    2.0e-01        1.03e-07
    noblank-r16_t168-ties          2.3e-08    3.0e-05    0.001      1.0e-04    1.7e-01        5.18e-08
    noblank-r16_ps-aligned         5.6e-10    1.7e-09    0.327      2.0e-06    4.1e-04        2.75e-06
    noblank-r16_ps-wrongpeak       5.4e-09    5.3e-07    0.010      2.0e-06    1.9e-03        1.30e-07
    noblank-r16_ps-masked          4.0e-10    9.4e-07    0.000      2.0e-06    1.9e-03        1.52e-07
    noblank-r16_ps-ties            2.9e-10    1.4e-08    0.021      2.0e-06    1.7e-03        1.61e-07
    noblank-xr_oddc-aligned        4.8e-08    6.7e-08    0.714      1.0e-04    1.3e-02        1.81e-07
    noblank-xr_oddc-wrongpeak      7.9e-08    4.9e-05    0.002      1.0e-04    2.0e-01        7.49e-08
    noblank-xr_oddc-masked         3.1e-08    1.9e-05    0.002      1.0e-04    2.0e-01        8.61e-08
    noblank-xr_oddc-ties           2.3e-08    7.9e-07    0.030      1.0e-04    1.8e-01        7.13e-08
    noblank-xr_s40-aligned         4.5e-08    1.5e-07    0.299      1.0e-04    1.6e-02        3.07e-06
    noblank-xr_s40-wrongpeak       1.3e-07    4.1e-05    0.003      1.0e-04    2.0e-01        2.01e-08
    noblank-xr_s40-masked          6.9e-08    4.9e-05    0.001      1.0e-04    2.0e-01        5.36e-08
    noblank-xr_s40-ties            2.5e-08    3.4e-06    0.008      1.0e-04    1.8e-01        1.34e-07
    noblank-pipelined-aligned      4.6e-08    2.0e-07    0.228      1.0e-04    1.6e-02        1.65e-06
    noblank-pipelined-wrongpeak    5.6e-06    6.0e-05    0.093      1.2e-04    2.0e-01        1.89e-07
    noblank-pipelined-masked       2.0e-05    1.2e-04    0.163      2.4e-04    2.0e-01        4.07e-07
    noblank-pipelined-ties         1.9e-06    9.3e-06    0.206      1.0e-04    1.8e-01        8.05e-07
    noblank-fused_t-aligned        4.1e-08    2.1e-07    0.198      1.0e-04    2.4e-02        1.16e-06
    noblank-fused_t-wrongpeak      7.6e-06    1.1e-04    0.069      2.2e-04    2.0e-01        4.81e-07
    noblank-fused_t-masked         9.0e-06    5.7e-05    0.157      1.2e-04    2.0e-01        3.31e-07
    noblank-fused_t-ties           5.7e-06    8.3e-05    0.069      1.7e-04    1.8e-01        1.59e-06
    noblank-fused_c-aligned        5.0e-08    2.1e-07    0.237      1.0e-04    1.2e-01        2.41e-07
    noblank-fused_c-wrongpeak      2.8e-06    4.9e-05    0.057      1.0e-04    2.0e-01        1.31e-07
    noblank-fused_c-masked         5.8e-06    2.5e-05    0.235      1.0e-04    2.0e-01        9.96e-08
    noblank-fused_c-ties           8.2e-07    2.2e-06    0.376      1.0e-04    2.0e-01        3.70e-07
    noblank-fused_k2-aligned       4.8e-08    1.5e-07    0.323      1.0e-04    2.6e-02        7.30e-07
    noblank-fused_k2-wrongpeak     2.0e-05    9.8e-05    0.202      2.0e-04    2.0e-01        1.38e-07
    noblank-fused_k2-masked        8.2e-06    7.9e-05    0.105      1.6e-04    2.0e-01        1.67e-07
    noblank-fused_k2-ties          1.6e-06    8.5e-06    0.185      1.0e-04    1.8e-01        6.63e-07
    noblank-fused_k4-aligned       3.5e-08    8.5e-08    0.412      1.0e-04    1.5e-02        3.64e-07
    noblank-fused_k4-wrongpeak     4.6e-07    2.0e-04    0.002      3.9e-04    2.0e-01        1.74e-07
    noblank-fused_k4-masked        1.9e-08    9.8e-05    0.000      2.0e-04    2.0e-01        2.76e-07
    noblank-fused_k4-ties          3.3e-07    3.4e-05    0.010      1.0e-04    1.7e-01        6.59e-07
    noblank-glb-aligned            5.0e-08    2.7e-06    0.019      1.0e-04    9.2e-03        3.83e-07
    noblank-glb-wrongpeak          6.4e-06    9.1e-05    0.070      1.8e-04    2.0e-01        6.37e-07
    noblank-glb-masked             1.2e-05    7.6e-05    0.157      1.5e-04    2.0e-01        3.54e-07
    noblank-glb-ties               2.4e-06    2.7e-05    0.090      1.0e-04    1.7e-01        1.29e-06
    binary-flow-aligned            1.9e-08    1.8e-08    1.021      2.6e-05    4.4e-03        1.18e-06
    binary-flow-wrongpeak          1.5e-07    1.7e-07    0.916      2.6e-05    1.7e-02        4.07e-06
    binary-flow-masked             8.1e-08    9.2e-07    0.088      2.6e-05    1.6e-02        1.29e-07
    binary-flow-ties               4.6e-09    3.4e-08    0.135      2.6e-05    8.3e-03        3.61e-08
    binary-flow_c158-aligned       1.8e-09    1.3e-09    1.405      2.6e-05    6.6e-04        1.68e-06
    binary-flow_c158-wrongpeak     4.2e-09    1.5e-08    0.277      2.6e-05    3.2e-03        2.81e-07
    binary-flow_c158-masked        7.9e-09    5.3e-08    0.149      2.6e-05    3.1e-03        2.13e-07
    binary-flow_c158-ties          3.5e-09    2.9e-09    1.215      2.6e-05    1.6e-03        9.33e-07
    binary-pipe_c-aligned          6.4e-10    8.0e-10    0.801      2.6e-05    3.5e-04        4.35e-07
    binary-pipe_c-wrongpeak        9.5e-08    1.2e-07    0.784      2.6e-05    2.5e-03        5.90e-06
    binary-pipe_c-masked           9.0e-09    2.2e-08    0.414      2.6e-05    2.4e-03        1.32e-07
    binary-pipe_c-ties             1.3e-09    1.9e-09    0.670      2.6e-05    1.3e-03        6.25e-08
    binary-pipe_t-aligned          2.4e-08    2.8e-08    0.860      2.6e-05    1.2e-02        4.70e-07
    binary-pipe_t-wrongpeak        4.1e-07    1.2e-06    0.331      2.6e-05    4.2e-02        1.11e-07
    binary-pipe_t-masked           1.0e-06    5.0e-06    0.210      2.6e-05    4.1e-02        3.96e-07
    binary-pipe_t-ties             2.7e-07    2.3e-06    0.116      2.6e-05    2.1e-02        1.53e-06
    binary-mfma_k2-aligned         4.8e-08    1.5e-07    0.309      2.6e-05    2.8e-02        4.82e-07
    binary-mfma_k2-wrongpeak       6.3e-08    2.3e-07    0.276      2.6e-05    4.2e-02        1.73e-07
    binary-mfma_k2-masked          6.5e-07    4.5e-06    0.145      2.6e-05    4.0e-02        2.72e-07
    binary-mfma_k2-ties            5.9e-08    1.3e-07    0.470      2.6e-05    2.1e-02        2.89e-07
    binary-mfma_k4-aligned         2.3e-07    2.4e-07    0.946      2.6e-05    2.3e-02        2.85e-07
    binary-mfma_k4-wrongpeak       3.3e-08    9.5e-07    0.035      2.6e-05    4.2e-02        2.73e-07
    binary-mfma_k4-masked          4.9e-07    5.8e-06    0.084      2.6e-05    4.0e-02        2.36e-07
    binary-mfma_k4-ties            6.3e-09    1.3e-06    0.005      2.6e-05    2.1e-02        5.48e-07
    binary-valu_c-aligned          4.0e-10    5.2e-10    0.775      2.6e-05    2.8e-04        2.51e-07
    binary-valu_c-wrongpeak        1.9e-09    4.9e-09    0.395      2.6e-05    1.9e-03        3.66e-08
    binary-valu_c-masked           5.1e-09    2.9e-08    0.178      2.6e-05    1.9e-03        1.07e-07
    binary-valu_c-ties             9.3e-10    3.7e-09    0.251      2.6e-05    9.7e-04        3.47e-07
    binary-valu_t-aligned          9.7e-09    1.2e-08    0.806      2.6e-05    2.9e-03        5.46e-07
    binary-valu_t-wrongpeak        1.1e-05    1.1e-05    0.999      2.6e-05    1.3e-02        2.37e-06
    binary-valu_t-masked           3.4e-07    1.4e-06    0.241      2.6e-05    1.2e-02        5.04e-07
    binary-valu_t-ties             6.6e-08    7.2e-07    0.091      2.6e-05    6.3e-03        1.52e-06

    best path / token spans        score err  bound      path == ref  frame_conf err  bound
    noblank-r16-aligned            6.0e-07    1.0e-05    1.0000       7.9e-08         2.0e-04
    noblank-r16-wrongpeak          1.7e-04    9.4e-03    1.0000       4.0e-06         7.3e-04
    noblank-r16-masked             2.7e-05    1.0e-02    1.0000       2.7e-05         2.4e-04
    noblank-r16-ties               8.4e-06    5.5e-04    1.0000       1.2e-06         2.0e-04
    noblank-fused_k2-aligned       2.8e-07    1.1e-05    1.0000       8.3e-08         2.0e-04
    noblank-fused_k2-wrongpeak     2.4e-04    3.4e-02    1.0000       9.8e-05         9.8e-04
    noblank-fused_k2-masked        3.3e-04    1.2e-02    1.0000       4.1e-05         7.9e-04
    noblank-fused_k2-ties          1.4e-04    2.2e-03    1.0000       7.9e-06         2.0e-04
    noblank-spans_k4-aligned       6.7e-07    1.0e-05    1.0000       1.5e-07         2.0e-04
    noblank-spans_k4-wrongpeak     2.2e-04    1.4e-02    1.0000       2.5e-05         9.8e-04
    noblank-spans_k4-masked        4.5e-04    1.2e-02    1.0000       4.2e-05         3.5e-04
    noblank-spans_k4-ties          7.2e-05    1.8e-03    1.0000       2.2e-06         2.1e-04
    binary-flow-aligned            8.0e-07    2.0e-05    1.0000       1.1e-06         2.0e-04
    binary-flow-wrongpeak          2.3e-04    1.2e-03    1.0000       6.4e-06         2.0e-04
    binary-flow-masked             1.7e-05    3.2e-03    1.0000       4.7e-06         2.0e-04
    binary-flow-ties               1.3e-05    5.5e-04    1.0000       4.2e-07         2.0e-04
    binary-mfma_k2-aligned         1.1e-06    2.0e-05    1.0000       3.6e-06         2.0e-04
    binary-mfma_k2-wrongpeak       1.6e-05    1.6e-03    1.0000       1.6e-06         2.0e-04
    binary-mfma_k2-masked          8.4e-05    6.7e-03    1.0000       1.6e-05         2.4e-04
    binary-mfma_k2-ties            4.5e-05    1.2e-03    1.0000       1.4e-06         2.0e-04
    binary-mfma_k4-aligned         4.9e-07    2.0e-05    1.0000       5.5e-06         2.0e-04
    binary-mfma_k4-wrongpeak       9.6e-06    1.6e-03    1.0000       5.9e-07         2.0e-04
    binary-mfma_k4-masked          7.0e-05    7.1e-03    1.0000       9.1e-06         3.1e-04
    binary-mfma_k4-ties            3.0e-05    1.1e-03    1.0000       7.4e-08         2.0e-04

    posteriors                     gamma err  err32      bound
    noblank-r16-aligned            1.1e-07    2.7e-07    2.0e-04
    noblank-r16-wrongpeak          7.5e-07    3.7e-04    7.3e-04
    noblank-r16-masked             1.4e-07    1.2e-04    2.4e-04
    noblank-r16-ties               5.4e-08    4.0e-06    2.0e-04
    noblank-fused_k2-aligned       8.3e-08    7.2e-07    2.0e-04
    noblank-fused_k2-wrongpeak     9.9e-05    4.9e-04    9.8e-04
    noblank-fused_k2-masked        4.1e-05    3.9e-04    7.9e-04
    noblank-fused_k2-ties          7.9e-06    3.3e-05    2.0e-04
    binary-flow-aligned            1.1e-06    1.5e-06    2.0e-04
    binary-flow-wrongpeak          7.4e-06    8.4e-06    2.0e-04
    binary-flow-masked             4.9e-06    6.1e-05    2.0e-04
    binary-flow-ties               1.8e-07    1.6e-06    2.0e-04
    binary-pipe_t-aligned          5.5e-07    1.6e-06    2.0e-04
    binary-pipe_t-wrongpeak        8.0e-06    3.1e-05    2.0e-04
    binary-pipe_t-masked           2.5e-05    1.3e-04    2.7e-04
    binary-pipe_t-ties             6.4e-06    4.6e-05    2.0e-04

    two-byte logits, masked        bf16 / f16 / f16 with +-65504: nll and gradient bits equal those of the fp32 path
    r16                            equal, equal, equal (samples without an alignment: 2 of 5, 2 of 5, 2 of 5)
    r16_n4                         equal, equal, equal (samples without an alignment: 2 of 5, 2 of 5, 2 of 5)
    r16_n2                         equal, equal, equal (samples without an alignment: 2 of 5, 2 of 5, 2 of 5)
    r16_c158                       equal, equal, equal (samples without an alignment: 2 of 5, 2 of 5, 2 of 5)
    r16_s31                        equal, equal, equal (samples without an alignment: 2 of 5, 2 of 5, 2 of 5)
    r16_t168                       equal, equal, equal (samples without an alignment: 2 of 5, 2 of 5, 2 of 5)
    r16_ps                         equal, equal, equal (samples without an alignment: 208 of 520, 208 of 520, 208 of 520)

Before the fixes of this commit (the library as its parent left it) these cases failed here:
  * every no-blank loss kernel on `masked`: r16 / xr reported nll = 1.45e6 (the 2^-2^21 emission clamp) for the samples
    without an alignment and gave them gradient rows of softmax / B; pipelined, fused (1, 2, 4 states per lane) and the
    workspace lattice returned NaN nll and NaN gradients (LSE of (-inf, -inf) in the chains);
  * noblank_posteriors (r16: 0 * 0 / 0 on a masked cell; fused: NaN) and noblank_token_spans (frame_conf and conf NaN
    through alpha + beta' - e = -inf - (-inf)) on `masked`, at one, two and four states per lane;
  * the streamed, pipelined and MFMA binary kernels and binary_posteriors on `masked`: NaN nll from +-inf logits
    (t - rint(t) in the careful form of the logs); the VALU kernel passed;
  * all 21 two-byte cases (the r16 defects above, through the bf16 / fp16 entry);
  * binary-pipe_t-aligned, loss and posteriors: nll of the pipelined binary kernel at (165,2,12,6) off by 1.29e-5 of
    max(1, |nll|) (2.2e-5 absolute on nll = -1.708) where the float32 port is off by 3.6e-7.  The cheap rows formed
    log(1 - p) as -log(1 + exp(-x)) - x, which cancels for x < 0 (7e-7 per element against emissions of -3e-3 per frame);
    as -max(x, 0) - log(1 + exp(-|x|)) it does not: 4.7e-7 now.  The streamed and the MFMA kernel had the same form.
The fixes: DESIGN.md 4, "Masked logits".  What the assertions hold in place, each seen on the MI355X with a library built
from a scratch copy: with the floor alone (kMasked) and without cell_posterior_log, test_loss_and_gradient
[noblank-fused_*-masked] fails at "gradient at an infinite logit" and test_token_spans[noblank-*-masked] at the frame_conf
bound (error 1.0); with the tie rule of viterbi_wave reverted (adv >= a in place of adv > a), test_best_path and
test_token_spans fail at "ties stay" on all twelve `ties` cases and pass on the other 36 (every batch holds a sample with
L_b < T_b for this: tests/lattice_inputs_ref._lengths).
"""
import numpy as np
import pytest
import torch

from tests.helpers import np_
from tests.lattice_inputs_ref import (BINARY_KERNEL, LOSS_PATHS, NLL_RTOL, NO_ALIGNMENT, PATH_SHAPES, POSTERIOR_SHAPES, R16,
                                      REGIMES, reference)
from tests.test_token_spans_abi import padded, spans_of_path

pytestmark = pytest.mark.gpu

LOSS_CASES = [(f, p, r) for f in LOSS_PATHS for p in LOSS_PATHS[f] for r in REGIMES]
PATH_CASES = [(f, p, r) for f in PATH_SHAPES for p in PATH_SHAPES[f] for r in REGIMES]
POSTERIOR_CASES = [(f, p, r) for f in POSTERIOR_SHAPES for p in POSTERIOR_SHAPES[f] for r in REGIMES]
SCORE_RTOL = {"noblank": 1e-5, "binary": 2e-5}        # test_noblank_best_path / test_binary_best_path
ids = "-".join


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    import ctc_amd  # noqa: F401  (raises if libctc_amd.so is missing)
    return torch.device("cuda:0")


def _api(family):
    import ctc_amd
    return {name: getattr(ctc_amd, "%s_%s" % (family, name))
            for name in ("ctc_loss", "best_path", "posteriors", "token_spans")}


def _on(dev, ref):
    x, tg, Tb, L = ref["inputs"]
    return x.to(dev), tg.to(dev), Tb.to(dev), L.to(dev)


def run_loss(dev, family, ref, grad=True):
    x, tg, Tb, L = _on(dev, ref)
    x.requires_grad_(grad)
    loss, nll = _api(family)["ctc_loss"](x, tg, Tb, L)
    if grad:
        loss.backward()
    torch.cuda.synchronize()
    return {"nll": np_(nll), "grad": np_(x.grad) if grad else None}


def check_nll(nll, ref, what, infinite=False):
    """>= 1e12 (the loss: the reference's sentinel magnitude; `infinite`: +inf, the read-outs) exactly on the samples
    without an alignment, within 1e-5 relative on the others"""
    fin = ref["fin"]
    nll = nll.astype(np.float64)
    assert not np.isnan(nll).any(), what
    assert np.array_equal(nll >= NO_ALIGNMENT, ~fin), "%s: nll %r, feasible %r" % (what, nll[:10], fin[:10])
    if infinite:
        assert np.isinf(nll[~fin]).all(), what
    nerr = float((np.abs(nll[fin] - ref["nll"][fin]) / np.maximum(1.0, np.abs(ref["nll"][fin]))).max())
    if not fin.all():
        print("lattice inputs %s: nll without an alignment %s" % (what, sorted(set("%.3g" % v for v in nll[~fin]))))
    assert nerr <= NLL_RTOL, "%s: nll off by %.3e relative" % (what, nerr)
    return nerr


# ---- 1. loss and gradient on every kernel ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", LOSS_CASES, ids=ids)
def test_loss_and_gradient(dev, case):
    family, path, regime = case
    ref = reference(*case)
    x, _, Tb, _ = ref["inputs"]
    T, B, C = x.shape
    fin, xn = ref["fin"], np_(x)
    r = run_loss(dev, family, ref)
    g32 = r["grad"]
    g = g32.astype(np.float64)
    err = float(np.abs(g[:, fin] - ref["grad"][:, fin]).max())
    print("lattice inputs %s: err %.3e err32 %.3e err/err32 %.3f bound %.3e max|grad_ref| %.3e"
          % (ids(case), err, ref["err32"], err / max(ref["err32"], 1e-300), ref["bound"], ref["gmax"]))
    nerr = check_nll(r["nll"], ref, ids(case))
    print("lattice inputs %s: nll_rel %.2e" % (ids(case), nerr))
    # the exact parts of the gradient
    assert np.isfinite(g32).all()
    for b in range(B):
        assert np.abs(g32[int(Tb[b]):, b]).max(initial=0.0) == 0.0, "sample %d beyond T_b" % b
        if not fin[b]:
            assert np.abs(g32[:, b]).max() == 0.0, "sample %d has no alignment" % b
    assert (g32[np.isinf(xn)] == 0.0).all(), "gradient at an infinite logit"
    # accuracy: neither term of the bound comes from the kernels
    assert err <= ref["bound"]
    if family == "noblank":                                   # softmax minus a distribution
        rows = np.abs(g.sum(2) * B)
        assert rows[:, fin].max() <= 1e-5
    # a forward-only call: the streamed binary kernel (test_binary_forward_only_launch_gives_the_same_loss) and the
    # persistent no-blank form (test_noblank_more_samples_than_cus_persistent) promise the bits, on every sample
    f = run_loss(dev, family, ref, grad=False)
    check_nll(f["nll"], ref, ids(case) + " forward only")
    if (family == "binary" and BINARY_KERNEL[path] == "flow") or (family, path) == ("noblank", "r16_ps"):
        assert np.array_equal(f["nll"].view(np.int32), r["nll"].view(np.int32)), "forward-only nll bits"
    else:
        assert (np.abs(f["nll"][fin] - r["nll"][fin]) <= 2e-6 * np.maximum(1.0, np.abs(r["nll"][fin]))).all()
    # two calls, equal bits
    again = run_loss(dev, family, ref)
    assert np.array_equal(again["nll"].view(np.int32), r["nll"].view(np.int32))
    assert np.array_equal(again["grad"].view(np.int32), g32.view(np.int32))


# ---- 2. the read-outs -------------------------------------------------------------------------------------------------
def _best_path(dev, family, ref):
    path, score = _api(family)["best_path"](*_on(dev, ref))
    torch.cuda.synchronize()
    return path, score


def check_path(path, score, ref, case):
    family, _, regime = case
    _, _, Tb, L = ref["inputs"]
    fin, e = ref["fin"], ref["e"]
    score = score.astype(np.float64)
    assert (path[~fin] == -1).all() and np.isneginf(score[~fin]).all(), "a sample without an alignment"
    assert np.isfinite(score[fin]).all()
    if regime == "ties":
        assert np.array_equal(path, ref["path"]), "ties stay"
    serr = float(np.abs(score[fin] - ref["score"][fin]).max())
    print("lattice inputs %s: score err %.3e (bound %.1e x %.3e), path agreement %.4f"
          % (ids(case), serr, SCORE_RTOL[family], np.abs(ref["score"][fin]).max(), (path == ref["path"]).mean()))
    assert serr <= SCORE_RTOL[family] * max(1.0, np.abs(ref["score"][fin]).max())
    for b in np.nonzero(fin)[0]:
        tb, l = int(Tb[b]), int(L[b])
        p = path[b]
        assert (p[tb:] == -1).all() and p[0] == 0 and p[tb - 1] == l - 1
        d = np.diff(p[:tb])
        assert ((d == 0) | (d == 1)).all()
        got = e[np.arange(tb), b, p[:tb]].sum()                 # the returned alignment attains the float64 optimum
        assert abs(got - ref["score"][b]) <= 1e-4 * max(1.0, abs(ref["score"][b])), (b, got, ref["score"][b])


@pytest.mark.parametrize("case", PATH_CASES, ids=ids)
def test_best_path(dev, case):
    ref = reference(*case)
    path, score = _best_path(dev, case[0], ref)
    check_path(np_(path), np_(score), ref, case)
    again = _best_path(dev, case[0], ref)
    assert torch.equal(again[0], path) and torch.equal(again[1].view(torch.int32), score.view(torch.int32))


def check_gamma(gamma, ref, case, what="gamma"):
    """gamma [B,T,S] against float64: finite, within max(2e-4, 2 err32_gamma), 0 on masked cells, beyond T_b / L_b and on
    samples without an alignment; live rows sum to 1 within 1e-5"""
    _, _, Tb, L = ref["inputs"]
    fin = ref["fin"]
    assert np.isfinite(gamma).all(), what
    g = gamma.astype(np.float64)
    err = float(np.abs(g[fin] - ref["gamma"][fin]).max())
    print("lattice inputs %s: %s err %.3e err32 %.3e bound %.3e" % (ids(case), what, err, ref["err32_gamma"], ref["gamma_bound"]))
    assert err <= ref["gamma_bound"], what
    assert (gamma[~fin] == 0).all(), "%s of a sample without an alignment" % what
    masked = np.isneginf(ref["e"]).transpose(1, 0, 2)
    for b in np.nonzero(fin)[0]:
        tb, l = int(Tb[b]), int(L[b])
        assert np.abs(g[b, :tb].sum(1) - 1.0).max() <= 1e-5, (what, b)
        assert (gamma[b, tb:] == 0).all() and (gamma[b, :, l:] == 0).all(), (what, b)
        assert (gamma[b, :tb, :l][masked[b, :tb, :l]] == 0).all(), "%s on a masked cell, sample %d" % (what, b)


@pytest.mark.parametrize("case", POSTERIOR_CASES, ids=ids)
def test_posteriors(dev, case):
    ref = reference(*case)
    gamma, nll = _api(case[0])["posteriors"](*_on(dev, ref))
    torch.cuda.synchronize()
    check_nll(np_(nll), ref, ids(case) + " posteriors")
    check_gamma(np_(gamma), ref, case)


@pytest.mark.parametrize("case", PATH_CASES, ids=ids)
def test_token_spans(dev, case):
    family = case[0]
    ref = reference(*case)
    _, tg, Tb, L = ref["inputs"]
    S, fin = tg.shape[1], ref["fin"]
    out = _api(family)["token_spans"](*_on(dev, ref))
    torch.cuda.synchronize()
    path, score = _best_path(dev, family, ref)
    assert torch.equal(out.path, path), "path"
    assert torch.equal(out.score.view(torch.int32), score.view(torch.int32)), "score"
    path, fc = np_(out.path), np_(out.frame_conf)
    check_path(path, np_(out.score), ref, case)
    check_nll(np_(out.nll), ref, ids(case) + " token spans", infinite=True)
    # frame_conf = gamma at the returned path
    assert np.isfinite(fc).all() and np.isfinite(np_(out.conf)).all()
    want = np.take_along_axis(ref["gamma"], np.maximum(path, 0)[:, :, None].astype(np.int64), 2)[:, :, 0]
    want[path < 0] = 0.0
    dfc = float(np.abs(fc - want).max())
    print("lattice inputs %s: frame_conf err %.3e bound %.3e" % (ids(case), dfc, ref["gamma_bound"]))
    assert dfc <= ref["gamma_bound"]
    # the spans: the restatement on the returned path and confidences, bit for bit; the partition of [0, T_b)
    s, e, c = spans_of_path(path, fc, np_(Tb), np_(L))
    start, end, conf = np_(out.start), np_(out.end), np_(out.conf)
    assert np.array_equal(start, padded(s, S, -1)), "start"
    assert np.array_equal(end, padded(e, S, -1)), "end"
    assert np.array_equal(conf.view(np.int32), padded(c, S, 0).view(np.int32)), "conf"
    for b in range(len(fin)):
        tb, l = int(Tb[b]), int(L[b])
        if not fin[b]:
            assert (fc[b] == 0).all() and (start[b] == -1).all() and (end[b] == -1).all() and (conf[b] == 0).all()
            continue
        assert (fc[b, tb:] == 0).all() and (fc[b, :tb] >= 0).all() and (fc[b, :tb] <= 1.0 + 1e-6).all()
        assert start[b, 0] == 0 and end[b, l - 1] == tb
        assert (end[b, :l - 1] == start[b, 1:l]).all() and (start[b, :l] < end[b, :l]).all()
        assert (start[b, l:] == -1).all() and (end[b, l:] == -1).all() and (conf[b, l:] == 0).all()


# ---- 3. two-byte logits on the r16 shapes -------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["bf16", "f16", "f16-65504"])
@pytest.mark.parametrize("path", R16)
def test_two_byte_masked_logits(dev, path, form):
    """the contract of tests/test_lowp_gpu.py on masked logits: nll is bitwise that of the fp32 path on x.float(), the
    gradient bitwise that path's gradient rounded to the dtype (fp16 turns PAD_LOGIT into -inf; +-65504 is its range)"""
    import ctc_amd
    dtype = torch.bfloat16 if form == "bf16" else torch.float16
    x, lab, Tb, L = reference("noblank", path, "masked")["inputs"]
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
        loss, nll = ctc_amd.noblank_ctc_loss(leaf, lab, Tb, L)
        loss.backward()
        torch.cuda.synchronize()
        out.append((nll.detach(), leaf.grad))
    (nll, g), (nll32, g32) = out
    assert g.dtype == dtype and nll.dtype == torch.float32
    assert torch.equal(nll.view(torch.int32), nll32.view(torch.int32)), "nll"
    assert torch.equal(g.view(torch.int16), g32.to(dtype).view(torch.int16)), "grad"
    assert bool(torch.isfinite(g).all()) and bool((g[torch.isinf(xl.detach())] == 0).all())
    print("lattice inputs two-byte %s-%s: nll and gradient bits equal, %d of %d samples without an alignment"
          % (path, form, int((nll >= 1e12).sum()), nll.numel()))
