"""The producer's kernels (ctc_amd/csrc/producer.hip, head_wide.hpp, lstm_wide.hpp, the typed and the backward entries) on the
inputs a real caller produces and a uniform draw at unit scale never does: saturated and overflowing gates, a cell state that
grows for 150 frames, zero-padded frames, repeated samples, dead Linear rows and BatchNorm channels, running_var == 0, and
fp16's +-65504 / subnormals / +-0 -- every regime of tests/producer_inputs_ref.py on every launch the public Python entries
of ctc_amd can make, at the smallest shape that reaches the launch (the shapes and their reasons: tests/test_lstm_wide_gpu.py,
tests/test_lstm_backward_gpu.py, tests/test_head_backward_gpu.py, tests/test_head_wide_gpu.py, tests/test_lstm_forward_gpu.py).

Exact assertions (no tolerance; README / DESIGN 3.6 contracts): every output finite; i, f, o in [0, 1], g and h in [-1, 1],
exactly 1 / 0 where the float64 pre-activation lies beyond +-90; pad columns == PAD_LOGIT; series / gates / cells of
lstm_series, lstm_series_wide and lstm_forward bit for bit those of T lstm_cell_step calls; lstm_forward bit for bit
head_forward + lstm_series; the wide head's lin and all of its eval mode bit for bit the narrow launch's; a typed call bit for
bit the fp32 call on feat.float(), d_feat that call's rounded once; d_b_ih == d_b_hh in two buffers; two calls the same bits;
duplicates: lin[t, b] has the bits of lin[t, 0]; dead: on bn_weight == 0 columns out == relu(bn_bias) x mask, d_bias and the
d_weight row exactly 0 (dlin itself is not visible through the Python entries: these two are its sums); where the output is 0
on every row of a column, d_bn_weight and d_bn_bias are exactly 0.

Accuracy against float64 (each case prints err, err32, err / err32, the bound and max |ref| before it asserts):
  non-constant columns   err <= max(plain, 2 err32), plain = 2e-5 absolute (recurrence forward), 2e-5 max(1, max |ref|)
                         (its gradients), 1e-4 max(1, max |ref|) (the head, the module): neither term comes from the kernels
  constant columns       |out - ref| <= |bn_weight| 316.3 B 2^-24 max |lin_column| (x the mask's factor), saved var <=
                         (B 2^-24 max |lin_column|)^2
  the backward           train mode: the float64 reference AND the float32 restatement behind err32 run on the kernel's own
                         saved lin, mean and invstd (what the entry's contract says it computes; on a constant column a
                         yardstick on another state measures numpy's sum order), err <= max(1e-4, 2 err32) of max(1, max
                         |ref|); without constant columns the end-to-end float64 reference is held to the same form as well.
                         Eval mode: the end-to-end reference.  The accuracy of train-mode d_bias is not asserted (identically
                         0 under batch statistics, a cancelling sum, rounding alone: the existing files skip it there too).
Cases made milder, each where the float32 restatement showed the same loss (written down in tests/producer_inputs_ref.py):
the cell behind lstm_forward has w_ih scaled to a fixed drive; range16 puts each +-65504 at a feature of its own; alternating
draws a Linear row again when it maps the two rows so close that invstd passes 10.

Measured on an MI355X (this file's own output; the tree of the change that added this file, on top of commit 21ee5cd, no kernel
source changed by it): see MEASURED below.

What failed before any fix: nothing.  No kernel needed a change: sigmoid_f's 1 / (1 + inf) is the exact 0, every gate beyond
exp's range is exactly 0 / 1 in all five forward kernels, the backward's derivative forms are exactly 0 there, both head
launches stay inside the derived bound on constant columns, and head_feat4's widening is exact at +-65504, at the subnormals
and at -0.

What the assertions hold in place (mutations of a scratch copy of the library, none of it committed): see MUTATIONS below."""
import types

import numpy as np
import pytest
import torch

from tests import producer_inputs_ref as R
from tests.head_backward_ref import head_backward_ref

pytestmark = pytest.mark.gpu

MEASURED = """
On an MI355X, on the tree this file was added in (parent commit 21ee5cd, no kernel changed): 331 passed.  One line per entry x shape
family x regime -- and per gradient for the train-mode backward of the head -- showing the row with the largest err / bound (rows: how
many it stands for; fp32, bf16 and fp16 features together, the typed entries give the fp32 bits; d_feat in the 2-byte types, whose one
rounding is 2^-8 / 2^-11 of max |ref|, has lines of its own).  err and bound of the gradients and of the head are in units of
max(1, max |ref|); "own state": reference and err32 on the kernel's saved lin, mean, invstd.  duplicates d_weight is a sum that
cancels to 1e-6: all of it is rounding, the kernel's as large as the restatement's on the same state (err / err32 1.1).  On the 126
train-mode cases with constant columns |out - ref| stayed inside |bn_weight| 316.3 B 2^-24 max |lin_column| on every element, and
the saved var was at most 1.5e-2 of (B 2^-24 max |lin_column|)^2.  Train-mode d_bias (not asserted): 1e-4 to 4e-3 of max(1, max |ref|)
on the constant-column cases, err32 on the same state 2e-5 to 2e-4.

entry                         family                                   regime             rows  worst row (err / bound)           err    err32 err/e32    bound max|ref|
cell_step=series=series_wide  T<=20                                    saturated             4  5x17x120x81                   6.7e-06  6.7e-06    1.00  2.0e-05  1.0e+00
cell_step=series=series_wide  T<=20                                    forget_open           4  7x9x158x158                   3.3e-06  2.7e-06    1.22  2.0e-05  1.0e+00
cell_step=series=series_wide  T<=20                                    padded_tail           4  5x17x120x81                   4.1e-06  4.2e-06    0.98  2.0e-05  9.9e-01
cell_step=series=series_wide  T<=20                                    extreme               4  20x7x38x38                    1.1e-05  1.0e-05    1.10  2.1e-05  1.0e+00
cell_step=series=series_wide  T=150                                    saturated             2  150x4x158x158                 6.6e-06  6.7e-06    0.97  2.0e-05  1.0e+00
cell_step=series=series_wide  T=150                                    forget_open           2  150x4x158x158                 3.7e-06  5.1e-06    0.74  2.0e-05  1.0e+00
cell_step=series=series_wide  T=150                                    padded_tail           2  150x4x158x158                 6.4e-06  6.4e-06    1.00  2.0e-05  1.0e+00
cell_step=series=series_wide  T=150                                    extreme               2  150x4x33x33                   1.3e-05  1.1e-05    1.12  2.3e-05  1.0e+00
lstm_forward                  T<=7                                     dead+saturated        6  7x9x64x40 fp32                2.7e-06  1.5e-06    1.89  2.0e-05  1.0e+00
lstm_forward                  T<=7                                     dead+extreme          6  7x9x64x40 fp32                8.2e-06  8.0e-06    1.02  2.0e-05  1.0e+00
lstm_forward                  T<=7                                     backbone+saturated    6  7x9x64x40 bf16                4.8e-06  2.6e-06    1.82  2.0e-05  1.0e+00
lstm_forward                  T<=7                                     backbone+extreme      6  7x9x64x40 bf16                1.4e-05  7.6e-06    1.82  2.0e-05  1.0e+00
lstm_series_backward          T<=20                                    saturated            14  20x7x38x38 d_x                5.8e-07  1.0e-06    0.57  2.0e-05  1.3e+00
lstm_backward = _SeriesFn     T<=20                                    saturated            14  20x7x38x38 d_x                7.3e-07  1.0e-06    0.73  2.0e-05  1.3e+00
lstm_series_backward          T<=20                                    forget_open          14  20x7x38x38 d_w_hh             5.2e-07  6.4e-07    0.81  2.0e-05  4.1e+00
lstm_backward = _SeriesFn     T<=20                                    forget_open          14  20x7x38x38 d_w_hh             5.1e-07  6.4e-07    0.79  2.0e-05  4.1e+00
lstm_series_backward          T<=20                                    padded_tail          14  20x7x38x38 d_w_ih             1.3e-06  8.0e-07    1.62  2.0e-05  8.3e+00
lstm_backward = _SeriesFn     T<=20                                    padded_tail          14  20x7x38x38 d_w_ih             1.3e-06  8.0e-07    1.65  2.0e-05  8.3e+00
lstm_series_backward          T<=20                                    extreme              14  20x7x38x38 d_w_hh             1.4e-05  1.0e-05    1.41  2.0e-05  7.7e-01
lstm_backward = _SeriesFn     T<=20                                    extreme              14  20x7x38x38 d_w_hh             1.4e-05  1.0e-05    1.41  2.0e-05  7.7e-01
lstm_series_backward          T=150                                    saturated             7  150x4x33x33 d_x               5.9e-07  8.0e-07    0.74  2.0e-05  1.8e+00
lstm_backward = _SeriesFn     T=150                                    saturated             7  150x4x33x33 d_w_hh            6.1e-07  5.3e-07    1.15  2.0e-05  4.2e+00
lstm_series_backward          T=150                                    forget_open           7  150x4x33x33 d_w_hh            2.0e-06  2.8e-06    0.73  2.0e-05  3.0e+01
lstm_backward = _SeriesFn     T=150                                    forget_open           7  150x4x33x33 d_w_hh            2.1e-06  2.8e-06    0.74  2.0e-05  3.0e+01
lstm_series_backward          T=150                                    padded_tail           7  150x4x33x33 d_w_ih            1.0e-06  1.4e-06    0.73  2.0e-05  1.3e+01
lstm_backward = _SeriesFn     T=150                                    padded_tail           7  150x4x33x33 d_w_ih            1.0e-06  1.4e-06    0.75  2.0e-05  1.3e+01
lstm_series_backward          T=150                                    extreme               7  150x4x33x33 d_x               9.5e-06  9.0e-06    1.05  2.0e-05  4.0e+00
lstm_backward = _SeriesFn     T=150                                    extreme               7  150x4x33x33 d_x               9.5e-06  9.0e-06    1.05  2.0e-05  4.0e+00
series_backward_wide + bias   T<=20                                    saturated            21  7x9x158x158 d_w_ih            4.4e-06  4.2e-06    1.05  2.0e-05  9.6e+00
_SeriesFn wide                T<=20                                    saturated            21  7x9x158x158 d_w_ih            4.4e-06  4.2e-06    1.05  2.0e-05  9.6e+00
series_backward_wide + bias   T<=20                                    forget_open          21  7x9x158x158 d_x               1.1e-06  1.0e-06    1.08  2.0e-05  9.3e-01
_SeriesFn wide                T<=20                                    forget_open          21  7x9x158x158 d_x               1.1e-06  1.0e-06    1.09  2.0e-05  9.3e-01
series_backward_wide + bias   T<=20                                    padded_tail          21  7x9x158x158 d_w_ih            3.4e-06  3.2e-06    1.05  2.0e-05  7.3e+00
_SeriesFn wide                T<=20                                    padded_tail          21  7x9x158x158 d_w_ih            3.3e-06  3.2e-06    1.04  2.0e-05  7.3e+00
series_backward_wide + bias   T<=20                                    extreme              21  20x7x38x38 d_w_hh             1.4e-05  1.0e-05    1.41  2.0e-05  7.7e-01
_SeriesFn wide                T<=20                                    extreme              21  20x7x38x38 d_w_hh             1.4e-05  1.0e-05    1.41  2.0e-05  7.7e-01
series_backward_wide + bias   T=150                                    saturated            14  150x4x158x158 d_b_ih          4.0e-06  4.0e-06    1.00  2.0e-05  4.0e+00
_SeriesFn wide                T=150                                    saturated            14  150x4x158x158 d_b_ih          4.0e-06  4.0e-06    1.00  2.0e-05  4.0e+00
series_backward_wide + bias   T=150                                    forget_open          14  150x4x158x158 d_b_ih          8.7e-06  1.9e-06    4.51  2.0e-05  1.1e+01
_SeriesFn wide                T=150                                    forget_open          14  150x4x158x158 d_b_ih          8.7e-06  1.9e-06    4.51  2.0e-05  1.1e+01
series_backward_wide + bias   T=150                                    padded_tail          14  150x4x158x158 d_w_ih          4.1e-06  4.1e-06    1.00  2.0e-05  2.3e+01
_SeriesFn wide                T=150                                    padded_tail          14  150x4x158x158 d_w_ih          4.1e-06  4.1e-06    1.01  2.0e-05  2.3e+01
series_backward_wide + bias   T=150                                    extreme              14  150x4x158x158 d_x             4.7e-05  4.7e-05    1.00  9.5e-05  4.4e+00
_SeriesFn wide                T=150                                    extreme              14  150x4x158x158 d_x             4.7e-05  4.7e-05    1.00  9.5e-05  4.4e+00
head narrow                   train, forward                           backbone            120  5x10x1024x33 out fp32         9.2e-07  6.2e-07    1.48  1.0e-04  4.6e+00
head narrow                   train, backward, own state d_feat        backbone              8  4x37x64x40 d_feat fp32        5.8e-08  5.6e-08    1.03  1.0e-04  2.4e-01
head narrow                   train, backward, own state d_weight      backbone             24  8x16x64x33 d_weight fp32      3.2e-07  3.2e-07    1.00  1.0e-04  1.8e+01
head narrow                   train, backward, own state d_bn_weight   backbone             24  9x16x64x33 d_bn_weight bf16   1.6e-07  1.1e-07    1.50  1.0e-04  1.4e+01
head narrow                   train, backward, own state d_bn_bias     backbone             24  4x37x64x40 d_bn_bias bf16     1.2e-07  8.0e-08    1.56  1.0e-04  1.0e+01
head narrow                   train, backward d_feat                   backbone              8  9x16x64x33 d_feat fp32        6.1e-08  5.2e-08    1.17  1.0e-04  2.0e-01
head narrow                   train, backward d_weight                 backbone             24  5x10x1024x33 d_weight fp16    6.1e-07  3.0e-07    2.01  1.0e-04  4.6e+00
head narrow                   train, backward d_bn_weight              backbone             24  5x10x1024x33 d_bn_weight bf16  6.1e-07  3.8e-07    1.61  1.0e-04  8.0e+00
head narrow                   train, backward d_bn_bias                backbone             24  4x37x64x40 d_bn_bias bf16     1.2e-07  8.0e-08    1.56  1.0e-04  1.0e+01
head narrow                   eval, forward                            backbone             48  5x10x1024x33 lin bf16         1.0e-06  3.2e-07    3.27  1.0e-04  1.1e+02
head narrow                   eval, backward                           backbone            104  5x10x1024x33 d_bn_weight bf16  6.1e-07  2.5e-07    2.43  1.0e-04  9.0e+00
head narrow                   train, forward                           padded              120  5x10x1024x33 var fp32         1.4e-06  5.2e-07    2.68  1.0e-04  1.2e+01
head narrow                   train, backward, own state d_feat        padded                8  5x10x1024x33 d_feat fp32      1.9e-07  1.7e-07    1.12  1.0e-04  4.5e+02
head narrow                   train, backward, own state d_weight      padded               24  8x16x64x33 d_weight bf16      4.4e-07  5.1e-07    0.86  1.0e-04  1.3e+01
head narrow                   train, backward, own state d_bn_weight   padded               24  8x16x64x33 d_bn_weight fp16   1.4e-07  1.4e-07    1.00  1.0e-04  1.2e+01
head narrow                   train, backward, own state d_bn_bias     padded               24  9x16x64x33 d_bn_bias fp16     1.6e-07  1.0e-07    1.53  1.0e-04  9.2e+00
head narrow                   eval, forward                            padded               48  5x10x1024x33 out fp32         1.0e-06  4.7e-07    2.20  1.0e-04  1.2e+01
head narrow                   eval, backward                           padded              104  5x10x1024x33 d_bn_weight fp32  8.4e-07  3.7e-07    2.30  1.0e-04  1.5e+01
head narrow                   train, forward                           duplicates          120  5x10x1024x33 lin bf16         1.3e-06  0.0e+00     inf  1.0e-04  8.1e+00
head narrow                   train, backward, own state d_feat        duplicates            8  5x10x1024x33 d_feat fp32      2.2e-07  1.9e-07    1.19  1.0e-04  4.8e+02
head narrow                   train, backward, own state d_weight      duplicates           24  4x37x64x40 d_weight fp16      9.8e-04  8.7e-04    1.12  1.7e-03  7.5e-07
head narrow                   train, backward, own state d_bn_weight   duplicates           24  5x10x1024x33 d_bn_weight fp32  6.3e-11  6.3e-11    1.00  1.0e-04  6.5e-04
head narrow                   train, backward, own state d_bn_bias     duplicates           24  9x16x64x33 d_bn_bias bf16     1.8e-07  1.8e-07    1.00  1.0e-04  2.3e+01
head narrow                   eval, forward                            duplicates           48  5x10x1024x33 out bf16         1.2e-06  4.3e-07    2.86  1.0e-04  8.7e+00
head narrow                   eval, backward                           duplicates          104  5x10x1024x33 d_bn_weight fp16  1.2e-06  1.9e-07    6.68  1.0e-04  3.1e+01
head narrow                   train, forward                           alternating         120  5x10x1024x33 invstd fp32      1.7e-05  6.7e-06    2.47  1.0e-04  9.8e+00
head narrow                   train, backward, own state d_feat        alternating           8  5x10x1024x33 d_feat fp32      3.0e-07  3.3e-07    0.91  1.0e-04  6.1e+00
head narrow                   train, backward, own state d_weight      alternating          24  4x37x64x40 d_weight fp32      4.9e-05  1.3e-05    3.70  1.0e-04  3.3e-02
head narrow                   train, backward, own state d_bn_weight   alternating          24  9x16x64x33 d_bn_weight fp32   1.4e-07  1.7e-07    0.82  1.0e-04  1.2e+01
head narrow                   train, backward, own state d_bn_bias     alternating          24  9x16x64x33 d_bn_bias fp32     1.6e-07  1.6e-07    1.00  1.0e-04  1.2e+01
head narrow                   train, backward d_feat                   alternating           8  5x10x1024x33 d_feat fp32      6.0e-06  5.0e-06    1.21  1.0e-04  6.1e+00
head narrow                   train, backward d_weight                 alternating          24  4x37x64x40 d_weight fp32      4.8e-05  8.8e-05    0.54  1.8e-04  3.3e-02
head narrow                   train, backward d_bn_weight              alternating          24  5x10x1024x33 d_bn_weight fp32  3.5e-07  3.2e-07    1.09  1.0e-04  6.9e+00
head narrow                   train, backward d_bn_bias                alternating          24  9x16x64x33 d_bn_bias fp32     1.6e-07  1.6e-07    1.00  1.0e-04  1.2e+01
head narrow                   eval, forward                            alternating          48  5x10x1024x33 out fp16         1.2e-06  5.1e-07    2.26  1.0e-04  1.2e+01
head narrow                   eval, backward                           alternating         104  5x10x1024x33 d_bn_weight bf16  1.5e-06  1.3e-06    1.21  1.0e-04  2.2e+01
head narrow                   train, forward                           dead                120  5x10x1024x33 var fp32         1.6e-06  3.5e-07    4.51  1.0e-04  1.8e+01
head narrow                   train, backward, own state d_feat        dead                  8  8x16x64x33 d_feat fp32        2.6e-07  2.0e-07    1.33  1.0e-04  1.8e+00
head narrow                   train, backward, own state d_weight      dead                 24  8x16x64x33 d_weight fp32      4.0e-07  4.0e-07    1.00  1.0e-04  5.6e+03
head narrow                   train, backward, own state d_bn_weight   dead                 24  4x37x64x40 d_bn_weight fp32   1.4e-07  1.8e-07    0.79  1.0e-04  9.5e+00
head narrow                   train, backward, own state d_bn_bias     dead                 24  4x37x64x40 d_bn_bias fp16     1.5e-07  4.8e-08    3.10  1.0e-04  2.5e+01
head narrow                   eval, forward                            dead                 48  5x10x1024x33 out fp32         1.3e-06  4.9e-07    2.62  1.0e-04  2.2e+03
head narrow                   eval, backward                           dead                104  5x10x1024x33 d_bn_weight fp16  1.6e-06  3.0e-07    5.42  1.0e-04  3.0e+03
head wide                     train, forward                           backbone             90  2x300x32x8 out fp16           3.8e-07  3.4e-07    1.12  1.0e-04  4.6e+00
head wide                     train, backward, own state d_feat        backbone              6  4x37x64x40 d_feat fp32        5.8e-08  5.1e-08    1.15  1.0e-04  2.4e-01
head wide                     train, backward, own state d_weight      backbone             18  2x300x32x8 d_weight fp16      2.9e-07  5.3e-07    0.55  1.0e-04  5.4e+01
head wide                     train, backward, own state d_bn_weight   backbone             18  2x300x32x8 d_bn_weight bf16   2.5e-07  3.6e-07    0.69  1.0e-04  1.5e+01
head wide                     train, backward, own state d_bn_bias     backbone             18  2x257x16x5 d_bn_bias fp16     3.2e-07  2.6e-07    1.21  1.0e-04  6.3e+00
head wide                     train, backward d_feat                   backbone              6  4x37x64x40 d_feat fp32        5.9e-08  5.0e-08    1.17  1.0e-04  2.4e-01
head wide                     train, backward d_weight                 backbone             18  2x257x16x5 d_weight fp32      3.4e-07  4.3e-07    0.79  1.0e-04  4.5e+01
head wide                     train, backward d_bn_weight              backbone             18  2x300x32x8 d_bn_weight bf16   2.8e-07  2.6e-07    1.06  1.0e-04  1.2e+01
head wide                     train, backward d_bn_bias                backbone             18  2x257x16x5 d_bn_bias fp16     3.2e-07  2.6e-07    1.21  1.0e-04  6.3e+00
head wide                     eval, forward                            backbone             36  4x37x64x40 out fp32           2.5e-07  2.4e-07    1.02  1.0e-04  5.9e+00
head wide                     eval, backward                           backbone             78  2x257x16x5 d_weight fp16      3.2e-07  1.6e-07    1.99  1.0e-04  5.7e+01
head wide                     train, forward                           padded               90  4x37x64x40 lin bf16           2.9e-07  2.9e-07    1.00  1.0e-04  2.5e+00
head wide                     train, backward, own state d_feat        padded                6  4x37x64x40 d_feat fp32        1.6e-07  1.3e-07    1.23  1.0e-04  5.7e+02
head wide                     train, backward, own state d_weight      padded               18  2x257x16x5 d_weight fp32      3.4e-07  4.2e-07    0.82  1.0e-04  3.3e+01
head wide                     train, backward, own state d_bn_weight   padded               18  2x257x16x5 d_bn_weight fp32   1.5e-07  2.4e-07    0.64  1.0e-04  1.0e+01
head wide                     train, backward, own state d_bn_bias     padded               18  2x257x16x5 d_bn_bias fp32     3.6e-07  1.5e-06    0.24  1.0e-04  3.7e+00
head wide                     eval, forward                            padded               36  4x37x64x40 out fp32           3.9e-07  2.2e-07    1.76  1.0e-04  4.2e+00
head wide                     eval, backward                           padded               78  2x257x16x5 d_bn_bias bf16     3.7e-07  5.9e-07    0.62  1.0e-04  6.5e+00
head wide                     train, forward                           duplicates           90  4x37x64x40 lin fp32           3.4e-07  0.0e+00     inf  1.0e-04  2.0e+00
head wide                     train, backward, own state d_feat        duplicates            6  4x37x64x40 d_feat fp32        1.6e-07  1.4e-07    1.13  1.0e-04  6.4e+02
head wide                     train, backward, own state d_weight      duplicates           18  2x257x16x5 d_weight bf16      4.2e-03  3.7e-03    1.15  7.4e-03  5.3e-06
head wide                     train, backward, own state d_bn_weight   duplicates           18  2x300x32x8 d_bn_weight fp16   5.9e-11  2.0e-11    3.01  1.0e-04  3.2e-04
head wide                     train, backward, own state d_bn_bias     duplicates           18  2x257x16x5 d_bn_bias bf16     1.0e-06  4.1e-06    0.26  1.0e-04  1.3e+00
head wide                     eval, forward                            duplicates           36  4x37x64x40 out fp32           2.4e-07  2.4e-07    1.00  1.0e-04  2.7e+00
head wide                     eval, backward                           duplicates           78  2x257x16x5 d_bn_bias fp16     1.1e-06  5.8e-07    1.89  1.0e-04  5.2e-01
head wide                     train, forward                           alternating          90  4x37x64x40 invstd bf16        1.8e-06  1.3e-06    1.42  1.0e-04  9.1e+00
head wide                     train, backward, own state d_feat        alternating           6  4x37x64x40 d_feat fp32        2.6e-07  2.7e-07    0.96  1.0e-04  7.0e+00
head wide                     train, backward, own state d_weight      alternating          18  2x257x16x5 d_weight bf16      7.5e-05  5.5e-05    1.35  1.1e-04  5.2e-02
head wide                     train, backward, own state d_bn_weight   alternating          18  2x257x16x5 d_bn_weight bf16   2.8e-07  2.5e-07    1.12  1.0e-04  6.8e+00
head wide                     train, backward, own state d_bn_bias     alternating          18  2x257x16x5 d_bn_bias bf16     2.9e-07  2.1e-07    1.41  1.0e-04  6.7e+00
head wide                     train, backward d_feat                   alternating           6  4x37x64x40 d_feat fp32        8.4e-07  8.2e-07    1.02  1.0e-04  9.2e+00
head wide                     train, backward d_weight                 alternating          18  2x257x16x5 d_weight bf16      7.8e-05  8.9e-05    0.87  1.8e-04  3.2e-02
head wide                     train, backward d_bn_weight              alternating          18  2x300x32x8 d_bn_weight fp16   4.0e-07  4.2e-06    0.09  1.0e-04  1.8e+01
head wide                     train, backward d_bn_bias                alternating          18  2x257x16x5 d_bn_bias bf16     2.9e-07  2.1e-07    1.41  1.0e-04  6.7e+00
head wide                     eval, forward                            alternating          36  4x37x64x40 out fp32           3.7e-07  5.6e-07    0.67  1.0e-04  2.6e+00
head wide                     eval, backward                           alternating          78  2x257x16x5 d_bn_weight fp16   4.1e-07  3.9e-07    1.03  1.0e-04  2.4e+00
head wide                     train, forward                           dead                 90  4x37x64x40 out fp32           3.4e-07  2.5e-07    1.36  1.0e-04  5.2e+00
head wide                     train, backward, own state d_feat        dead                  6  4x37x64x40 d_feat fp32        1.9e-07  1.9e-07    0.96  1.0e-04  2.6e+00
head wide                     train, backward, own state d_weight      dead                 18  2x300x32x8 d_weight fp16      3.6e-07  1.2e-06    0.30  1.0e-04  9.0e+03
head wide                     train, backward, own state d_bn_weight   dead                 18  2x257x16x5 d_bn_weight fp32   2.5e-07  5.1e-07    0.49  1.0e-04  2.8e+00
head wide                     train, backward, own state d_bn_bias     dead                 18  2x300x32x8 d_bn_bias fp16     2.4e-07  7.4e-07    0.33  1.0e-04  1.2e+01
head wide                     eval, forward                            dead                 36  4x37x64x40 lin bf16           3.3e-07  3.3e-07    1.00  1.0e-04  2.4e+00
head wide                     eval, backward                           dead                 78  2x300x32x8 d_bn_weight fp32   8.8e-07  1.2e-06    0.73  1.0e-04  1.9e+02
head typed d_feat             bf16, own state                          all                  84  4x37x64x40 d_feat bf16        3.7e-03  1.6e-07 22750.50  4.0e-03  5.1e+02
head typed d_feat             bf16                                     all                 126  2x257x16x5 d_feat bf16        3.4e-03  1.3e-07 25243.61  4.0e-03  1.3e+02
head typed d_feat             fp16, own state                          all                  84  5x10x1024x33 d_feat fp16      4.7e-04  1.6e-07 3014.67  5.9e-04  5.2e+02
head typed d_feat             fp16                                     all                 126  8x16x64x33 d_feat fp16        4.7e-04  1.4e-07 3330.94  5.9e-04  2.6e+02
head narrow                   train, forward                           range16              80  5x10x1024x33 lin fp16         1.7e-06  1.2e-06    1.40  1.0e-04  1.6e+01
head narrow                   train, backward, own state d_weight      range16              16  8x16x64x33 d_weight fp16      3.9e-07  3.9e-07    1.00  1.0e-04  4.9e+04
head narrow                   train, backward, own state d_bn_weight   range16              16  8x16x64x33 d_bn_weight bf16   1.8e-07  1.8e-07    1.00  1.0e-04  1.1e+01
head narrow                   train, backward, own state d_bn_bias     range16              16  8x16x64x33 d_bn_bias bf16     1.9e-07  1.6e-07    1.19  1.0e-04  1.0e+01
head narrow                   train, backward d_weight                 range16              16  5x10x1024x33 d_weight fp16    8.9e-07  6.1e-07    1.46  1.0e-04  2.9e+04
head narrow                   train, backward d_bn_weight              range16              16  5x10x1024x33 d_bn_weight fp16  5.5e-07  7.4e-07    0.74  1.0e-04  8.3e+00
head narrow                   train, backward d_bn_bias                range16              16  8x16x64x33 d_bn_bias bf16     1.9e-07  1.6e-07    1.19  1.0e-04  1.0e+01
head narrow                   eval, forward                            range16              32  5x10x1024x33 lin fp16         1.9e-06  1.1e-06    1.64  1.0e-04  1.6e+01
head narrow                   eval, backward                           range16              64  5x10x1024x33 d_bn_weight bf16  5.4e-07  5.4e-07    1.00  1.0e-04  9.0e+00
head wide                     train, forward                           range16              60  4x37x64x40 lin fp16           4.5e-07  4.5e-07    0.99  1.0e-04  1.6e+01
head wide                     train, backward, own state d_weight      range16              12  2x257x16x5 d_weight fp16      5.6e-07  9.1e-07    0.62  1.0e-04  5.7e+04
head wide                     train, backward, own state d_bn_weight   range16              12  2x257x16x5 d_bn_weight fp16   4.5e-07  4.9e-07    0.92  1.0e-04  1.2e+01
head wide                     train, backward, own state d_bn_bias     range16              12  4x37x64x40 d_bn_bias fp16     1.6e-07  1.6e-07    1.00  1.0e-04  1.2e+01
head wide                     train, backward d_weight                 range16              12  2x257x16x5 d_weight fp16      5.9e-07  1.1e-06    0.55  1.0e-04  5.7e+04
head wide                     train, backward d_bn_weight              range16              12  2x300x32x8 d_bn_weight fp16   3.9e-07  4.7e-07    0.82  1.0e-04  1.1e+01
head wide                     train, backward d_bn_bias                range16              12  4x37x64x40 d_bn_bias fp16     1.6e-07  1.6e-07    1.00  1.0e-04  1.2e+01
head wide                     eval, forward                            range16              24  4x37x64x40 lin fp16           4.7e-07  4.7e-07    1.00  1.0e-04  1.6e+01
head wide                     eval, backward                           range16              48  2x300x32x8 d_weight fp16      3.4e-07  3.7e-07    0.90  1.0e-04  3.8e+05
LSTM_cell                     5x10x1024x33                             padded+saturated     11  running_var                   1.6e-06  5.1e-07    3.13  1.0e-05  3.5e+00
LSTM_cell                     4x6x64x158                               padded+saturated     11  d_w_hh                        4.6e-06  1.8e-06    2.48  1.0e-04  1.7e+00
LSTM_cell                     2x300x64x33                              padded+saturated     11  d_bn_weight                   4.3e-06  6.5e-06    0.66  1.0e-04  7.1e+00
"""
MUTATIONS = """
Three mutations of a scratch copy of the library (wrong numbers, no faults), each run once against this file:
  sigmoid_f as e / (1 + e), e = __expf(v)        32 failed, 299 passed.  test_recurrence_forward: extreme on all six shapes,
      saturated at both H = 158 shapes and padded_tail at (150,4,158,158) (their pre-activations pass 88.7 too) -- "not finite"
      names lstm_cell_step, lstm_series, lstm_series_wide, with and without saved state; test_lstm_forward: all twelve extreme
      cases, "not finite" names lstm_forward, head_forward + lstm_series and lstm_cell_step; test_recurrence_backward: the
      eleven cases that run on those states.  The saturated cell behind lstm_forward alone (|pre| <= 60) does not see it: that
      is why test_lstm_forward has the extreme cell too.
  the narrow head's variance as E[x^2] - mean^2   43 failed, 288 passed: every train-mode case of test_head and test_head_typed
      through the narrow entry in padded, duplicates and dead (36, on a negative saved var) and seven of the twelve in
      alternating, whose columns are not constant (on the accuracy of d_weight / invstd).  backbone and range16 pass: with the
      issue's draw a column's offset (22 at K = 1024) is smaller than its spread (40), and a positive-mean weight cannot bring
      offset / spread of relu(u - 0.2) x 30 features beyond 0.65 sqrt(K) = 21, where the one-pass form loses 1e-7 x 21^2 of
      the variance, below 1e-4; the common offset that does break it is OFFSET of tests/head_forward_ref.py (1000 against 0.5).
  1 - gg * gg as 1 - gg in lstm_series_bwd_kernel   14 failed, 317 passed: the twelve narrow cases of
      test_recurrence_backward and the two shapes of test_module_train_step whose recurrence backward is that kernel; every
      wide case and (4,6,64,158) pass.
"""

IDS = lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else str(s)          # noqa: E731
OPEN = 1 << 30
REC_SHAPES = [(9, 5, 17, 40), (20, 7, 38, 38), (5, 17, 120, 81), (7, 9, 158, 158), (150, 4, 33, 33), (150, 4, 158, 158)]
REC_BWD_SHAPES = [(9, 5, 17, 40), (20, 7, 38, 38), (7, 9, 158, 158), (150, 4, 33, 33), (150, 4, 158, 158)]
REC_BWD_CASES = [(p, s) for p in ("narrow", "wide") for s in REC_BWD_SHAPES if p == "wide" or s[2] + s[3] <= 80]   # narrow: I + H <= 80
FUSED_SHAPES = [(3, 6, 48, 17), (7, 9, 64, 40)]
HEAD_SHAPES = {"narrow": [(4, 37, 64, 40), (5, 10, 1024, 33), (8, 16, 64, 33), (9, 16, 64, 33)],
               "wide": [(2, 257, 16, 5), (2, 300, 32, 8), (4, 37, 64, 40)]}
HEAD_CASES = [(e, s) for e in ("narrow", "wide") for s in HEAD_SHAPES[e]]
MODULE_SHAPES = [(5, 10, 1024, 33), (4, 6, 64, 158), (2, 300, 64, 33)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    import ctc_amd  # noqa: F401
    return torch.device("cuda:0")


def np_(t):
    return t.detach().cpu().numpy().astype(np.float64)


def tt(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _finite(*ts):
    return all(t is None or bool(torch.isfinite(t).all()) for t in ts)


def _same(a, b):
    """two results, tensor by tensor, the same bits (NaN-free by the finiteness assertions)"""
    return len(a) == len(b) and all((x is None and y is None) or torch.equal(x, y) for x, y in zip(a, b))


def _report(rows):
    """rows: (what, err, err32, bound, max |ref|); print every figure, then assert"""
    for what, err, e32, bound, scale in rows:
        print("%-60s err %.3e  err32 %.3e  err/err32 %8.2f  bound %.3e  max|ref| %.3e"
              % (what, err, e32, err / e32 if e32 > 0 else float("inf") if err > 0 else 0.0, bound, scale))
    for what, err, e32, bound, scale in rows:
        assert err <= bound, (what, err, e32, bound)


def _counting(monkeypatch, name):
    from ctc_amd import _lib
    lib = _lib.load()
    real = getattr(lib, name)
    calls = []

    def wrapped(*a):
        calls.append(1)
        return real(*a)
    monkeypatch.setattr(lib, name, wrapped)
    return calls


# ---- the recurrence ---------------------------------------------------------------------------------------------------

def _rec_args(d, dev):
    return [tt(d[k], dev) for k in R.REC_KEYS]


_STEPS = {}


def _steps(key, d, cols, dev, v_all=None):
    """T calls of lstm_cell_step (once per case and width): series with its pad columns, gates, cells"""
    if (key, cols) not in _STEPS:
        import ctc_amd
        args = _rec_args(d, dev)
        if v_all is not None:
            args[0] = v_all
        T, B = args[0].shape[:2]
        series = torch.empty((T, B, cols), dtype=torch.float32, device=dev)
        h, c, gates, cells = args[1], args[2], [], [args[2]]
        for t in range(T):
            h, c, gt = ctc_amd.lstm_cell_step(args[0][t], h, c, *args[3:], series[t], want_gates=True)
            gates.append(gt)
            cells.append(c)
        torch.cuda.synchronize()
        _STEPS[(key, cols)] = (series, torch.stack(gates), torch.stack(cells))
    return _STEPS[(key, cols)]


def _gates_in_range(series, gates, H, pre64=None):
    from ctc_amd.producer import PAD_LOGIT
    assert _finite(series[:, :, :H], gates)
    sig = torch.cat([gates[:, :, :2 * H], gates[:, :, 3 * H:]], 2)
    assert float(sig.min()) >= 0.0 and float(sig.max()) <= 1.0
    assert float(gates[:, :, 2 * H:3 * H].abs().max()) <= 1.0 and float(series[:, :, :H].abs().max()) <= 1.0
    if series.shape[2] > H:
        assert bool((series[:, :, H:] == PAD_LOGIT).all())
    if pre64 is not None:                                    # beyond exp's range (with room for the fp32 rounding of the sum)
        p = torch.from_numpy(pre64).to(gates.device)
        s = torch.ones(4 * H, dtype=torch.bool, device=gates.device)
        s[2 * H:3 * H] = False
        assert bool((gates[(p > 90) & s] == 1).all()) and bool((gates[(p < -90) & s] == 0).all())
        assert bool((gates[(p > 90) & ~s] == 1).all()) and bool((gates[(p < -90) & ~s] == -1).all())


@pytest.mark.parametrize("regime", R.REC_REGIMES)
@pytest.mark.parametrize("shape", REC_SHAPES, ids=IDS)
def test_recurrence_forward(dev, shape, regime):
    """lstm_cell_step, lstm_series (I + H <= 80), lstm_series_wide"""
    import ctc_amd
    T, B, I, H = shape
    c = R.rec_case(regime, shape)
    args = _rec_args(c.d, dev)
    pre = R.rec_state(c.d)[2] if regime == "extreme" else None
    entries = [("lstm_series_wide", ctc_amd.lstm_series_wide)] + ([("lstm_series", ctc_amd.lstm_series)] if I + H <= 80 else [])
    for cols in (H, H + 1 + H % 2):
        steps = _steps((regime, shape), c.d, cols, dev)
        res = {"lstm_cell_step": steps}
        for name, fn in entries:
            res[name] = fn(*args, cols, want_backward_state=True)
            res[name + ", no state"] = fn(*args, cols, want_backward_state=False)
            assert res[name] is not None, (name, shape)
        torch.cuda.synchronize()
        bad = [name for name, r in res.items() if not _finite(r[0][:, :, :H], r[1], r[2])]          # (each kernel named)
        assert not bad, ("not finite", bad, shape, regime, cols)
        _gates_in_range(steps[0], steps[1], H, pre)
        assert torch.equal(steps[2][0], args[2])
        for name, fn in entries:
            assert _same(res[name], steps), (name, shape, cols)
            again = res[name + ", no state"]
            assert torch.equal(again[0], steps[0]) and again[1] is None and again[2] is None
    got = np_(steps[0])[:, :, :H]
    err = float(np.abs(got - c.series).max())
    e32 = c.err32["series"]
    _report([("forward steps=series=wide %s %s" % (IDS(shape), regime), err, e32, max(R.PLAIN_FWD, 2 * e32),
              float(np.abs(c.series).max()))])


@pytest.mark.parametrize("cell", ["saturated", "extreme"])
@pytest.mark.parametrize("lowp", [None, "bf16", "fp16"], ids=["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("regime", ["dead", "backbone"])
@pytest.mark.parametrize("shape", FUSED_SHAPES, ids=IDS)
def test_lstm_forward(dev, shape, regime, lowp, cell):
    """lstm_forward (an eval-mode head in front of a saturated cell, one launch) == head_forward + lstm_series == the steps;
    in front of an extreme cell as well, so that the one launch too sees pre-activations beyond exp's range"""
    import ctc_amd
    T, B, K, C = shape
    c = R.fused_case(regime, shape, lowp, cell)
    hd = c.head.d
    feat = tt(hd["feat"], dev)
    if lowp:
        feat = feat.to(R.LOWP[lowp])
    head = [tt(hd[k], dev) for k in ("weight", "bias", "bn_weight", "bn_bias", "running_mean", "running_var")]
    cellw = _rec_args(c.d, dev)[1:]
    v_all = ctc_amd.head_forward(feat, *head, hd["eps"])[0]
    assert _finite(v_all)
    for cols in (C, C + 1 + C % 2):
        two = ctc_amd.lstm_series(v_all, *cellw, cols)[0]
        one = ctc_amd.lstm_forward(feat, *head, hd["eps"], *cellw, cols)
        again = ctc_amd.lstm_forward(feat, *head, hd["eps"], *cellw, cols)
        torch.cuda.synchronize()
        assert one is not None
        steps = _steps(("fused", regime, shape, lowp, cell), c.d, cols, dev, v_all)
        bad = [n for n, r in (("lstm_forward", one), ("head_forward + lstm_series", two), ("lstm_cell_step", steps[0]))
               if not _finite(r[:, :, :C])]
        assert not bad, ("not finite", bad, shape, regime, cell, cols)
        _gates_in_range(one, steps[1], C)
        assert torch.equal(one, two) and torch.equal(one, steps[0]) and torch.equal(one, again)
        if lowp:
            assert torch.equal(one, ctc_amd.lstm_forward(feat.float(), *head, hd["eps"], *cellw, cols))
    err = float(np.abs(np_(one)[:, :, :C] - c.series).max())
    _report([("lstm_forward %s %s %s %s" % (IDS(shape), regime, cell, lowp or "fp32"), err, c.err32, max(R.PLAIN_FWD, 2 * c.err32),
              float(np.abs(c.series).max()))])


def _from_dpre(dpre, dh0, dc0, c, series):
    """the seven gradients from a recurrence launch's dpre, the products in float64"""
    d = c.d
    T, B, G = dpre.shape
    H = G // 4
    p = np_(dpre).reshape(T * B, G)
    hs = np.concatenate([np.asarray(d["h0"], np.float64)[None], np_(series)[:-1, :, :H]]).reshape(T * B, H)
    db = p.sum(0)
    return [(p @ np.asarray(d["w_ih"], np.float64)).reshape(T, B, -1), np_(dh0), np_(dc0),
            p.T @ np.asarray(d["v"], np.float64).reshape(T * B, -1), p.T @ hs, db, db]


def _seriesfn(c, dev, cols):
    from ctc_amd import producer
    leaves = [t.clone().requires_grad_(True) for t in _rec_args(c.d, dev)]
    series = producer._SeriesFn.apply(*leaves, cols, producer.PAD_LOGIT)
    fn = series.grad_fn
    (series * tt(c.d["d_series"], dev)).sum().backward()
    torch.cuda.synchronize()
    return series.detach(), fn, [t.grad for t in leaves]


@pytest.mark.parametrize("regime", R.REC_REGIMES)
@pytest.mark.parametrize("path,shape", REC_BWD_CASES, ids=IDS)
def test_recurrence_backward(dev, monkeypatch, shape, regime, path):
    """narrow (I + H <= 80): lstm_series_backward, lstm_backward, _SeriesFn through them; wide: lstm_series_backward_wide +
    lstm_bias_grad_wide, _SeriesFn through them -- both gates open"""
    import ctc_amd
    from ctc_amd import producer
    T, B, I, H = shape
    c = R.rec_case(regime, shape)
    d = c.d
    cols = H + 1 + H % 2
    series, gates, cells = _steps((regime, shape), d, cols, dev)
    v, h0, c0, w_ih, w_hh, b_ih, b_hh = _rec_args(d, dev)
    up = tt(d["d_series"], dev)
    monkeypatch.setattr(producer, "SERIES_WIDE_MAX_ROWS", OPEN)
    monkeypatch.setattr(producer, "SERIES_BACKWARD_MAX_ROWS", OPEN)
    results = {}
    if path == "narrow":
        rec = producer.lstm_series_backward(up, gates, cells, w_hh)
        whole = ctc_amd.lstm_backward(up, gates, cells, v, h0, series, w_ih, w_hh)
        again = ctc_amd.lstm_backward(up, gates, cells, v, h0, series, w_ih, w_hh)
        nodx = ctc_amd.lstm_backward(up, gates, cells, v, h0, series, w_ih, w_hh, need_dx=False)
        torch.cuda.synchronize()
        assert whole is not None and _finite(*rec, *whole)
        assert torch.equal(whole[1], rec[1]) and torch.equal(whole[2], rec[2])
        assert whole[5].data_ptr() != whole[6].data_ptr() and torch.equal(whole[5], whole[6])
        assert _same(whole, again) and nodx[0] is None and _same(whole[1:], nodx[1:])
        calls = _counting(monkeypatch, "ctc_amd_lstm_backward")
        out, fn, grads = _seriesfn(c, dev, cols)
        assert fn.one_launch and fn.in_place and len(calls) == 1
        assert torch.equal(out, series) and _same(grads, whole)
        results = {"lstm_series_backward": _from_dpre(*rec, c, series), "lstm_backward = _SeriesFn": [np_(t) for t in whole]}
    else:
        rec = ctc_amd.lstm_series_backward_wide(up, gates, cells, w_hh)
        again = ctc_amd.lstm_series_backward_wide(up, gates, cells, w_hh)
        torch.cuda.synchronize()
        assert rec is not None and _finite(*rec) and _same(rec, again)
        db = ctc_amd.lstm_bias_grad_wide(rec[0])
        assert db[0].data_ptr() != db[1].data_ptr() and torch.equal(db[0], db[1]) and _same(db, ctc_amd.lstm_bias_grad_wide(rec[0]))
        if I + H <= 80:                                      # (only with the narrow launch out of the way does _SeriesFn reach the wide one)
            monkeypatch.setattr(producer, "lstm_series", lambda *a, **k: None)
        calls = [_counting(monkeypatch, n) for n in ("ctc_amd_lstm_series_wide", "ctc_amd_lstm_series_backward_wide",
                                                     "ctc_amd_lstm_bias_grad_wide", "ctc_amd_lstm_cell_step")]
        out, fn, grads = _seriesfn(c, dev, cols)
        assert fn.wide and not fn.one_launch and [len(x) for x in calls] == [1, 1, 1, 0]
        assert torch.equal(out, series) and _finite(*grads)
        assert torch.equal(grads[1], rec[1]) and torch.equal(grads[2], rec[2])
        assert torch.equal(grads[5], db[0]) and torch.equal(grads[6], db[1]) and grads[5].data_ptr() != grads[6].data_ptr()
        from_dpre = _from_dpre(*rec, c, series)
        from_dpre[5], from_dpre[6] = np_(db[0]), np_(db[1])
        results = {"lstm_series_backward_wide + bias_grad": from_dpre, "_SeriesFn wide": [np_(t) for t in grads]}
    rows = []
    for what, got in results.items():
        for name, g in zip(R.REC_GRAD, got):
            ref, e32 = c.grads[name], c.err32[name]
            rows.append(("%s %s %s %s" % (what, IDS(shape), regime, name), R.rel_err(g, ref), e32, max(R.PLAIN_GRAD, 2 * e32),
                         float(np.abs(ref).max())))
    _report(rows)


# ---- the head ---------------------------------------------------------------------------------------------------------

def _head_entries(entry):
    import ctc_amd
    return (ctc_amd.head_forward, ctc_amd.head_backward) if entry == "narrow" else (ctc_amd.head_forward_wide, ctc_amd.head_backward_wide)


def _head_tensors(c, dev):
    d = c.d
    t = types.SimpleNamespace(**{k: tt(d.get(k), dev) for k in ("feat", "weight", "bias", "bn_weight", "bn_bias", "running_mean",
                                                                 "running_var", "mask", "d_out")})
    if c.lowp:
        t.feat = t.feat.to(R.LOWP[c.lowp])
    return t


def _head_forward(fwd, t, feat, eps, state=True):
    return fwd(feat, t.weight, t.bias, t.bn_weight, t.bn_bias, t.running_mean, t.running_var, eps, t.mask, want_backward_state=state)


def _head_backward(bwd, t, feat, fw, train, eps, need_dfeat=True):
    st = (fw[2], fw[4], None, None) if train else (None, None, t.running_mean, t.running_var)
    return bwd(t.d_out, feat, t.weight, t.bn_weight, t.bn_bias, fw[1], *st, eps, t.mask, need_dfeat)


def _check_head(dev, entry, c):
    """every assertion of the module docstring on one case of the head through one pair of entries"""
    fwd, bwd = _head_entries(entry)
    d, train = c.d, c.train
    T, B, K, C = c.shape
    tag = "%s %s %s %s %s %s" % (entry, IDS(c.shape), c.regime, "train" if train else "eval", "mask" if c.with_mask else "nomask",
                                 c.lowp or "fp32")
    t = _head_tensors(c, dev)
    fw = _head_forward(fwd, t, t.feat, d["eps"])
    assert fw is not None, tag
    fw2 = _head_forward(fwd, t, t.feat, d["eps"])
    plain = _head_forward(fwd, t, t.feat, d["eps"], state=False)
    torch.cuda.synchronize()
    assert _finite(*fw) and _same(fw, fw2) and torch.equal(plain[0], fw[0]) and plain[1] is None
    out, lin, mean, var, inv = fw
    if train:
        assert float(var.min()) >= 0.0 and float(inv.max()) <= R.INV_MAX
    else:
        assert mean is None and var is None and inv is None
    if c.lowp:                                               # the typed entry: bit for bit the fp32 entry on feat.float()
        assert _same(fw, _head_forward(fwd, t, t.feat.float(), d["eps"]))
    if c.regime == "duplicates":
        assert torch.equal(lin, lin[:, :1].expand_as(lin))
    g0 = torch.from_numpy(d["bn_weight"] == 0).to(dev)
    if bool(g0.any()):                                       # a dead BatchNorm channel: relu(bn_bias) x mask, exactly
        want = torch.relu(t.bn_bias[g0]).expand(T, B, -1)
        assert torch.equal(out[:, :, g0], want if t.mask is None else want * t.mask[:, :, g0])
    # accuracy of the forward
    const = c.const
    rows = []
    names = R.HEAD_OUT if train else ("out", "lin")
    for name, got in zip(names, fw):
        ref, e32 = c.fwd[name], c.err32[name]
        k = np.zeros_like(const) if name in ("lin", "mean") else const           # (lin and the mean are benign on every column)
        rows.append(("%s %s" % (tag, name), R.head_err(np_(got), ref, k, train), e32, max(R.HEAD_TOL, 2 * e32),
                     float(np.abs(ref).max())))
    if const.any():
        bound, var_bound = R.const_out_bound(c)
        k3 = np.broadcast_to(const[:, None, :], out.shape)
        diff = np.abs(np_(out) - c.fwd["out"])
        worst = float((diff - bound)[k3].max())
        print("%-60s constant columns: max |out - ref| %.3e, largest bound %.3e, worst (err - bound) %.3e; max var / bound %.3e"
              % (tag, diff[k3].max(), np.broadcast_to(bound, out.shape)[k3].max(), worst,
                 (np_(var)[const] / np.maximum(var_bound[const], 1e-300)).max()))
        assert worst <= 0.0, tag
        assert bool((np_(var)[const] <= var_bound[const]).all()), tag
    # the backward, on the forward's own saved state
    bw = _head_backward(bwd, t, t.feat, fw, train, d["eps"])
    assert bw is not None, tag
    bw2 = _head_backward(bwd, t, t.feat, fw, train, d["eps"])
    nodf = _head_backward(bwd, t, t.feat, fw, train, d["eps"], need_dfeat=False)
    torch.cuda.synchronize()
    assert _finite(*bw) and _same(bw, bw2) and nodf[0] is None and _same(bw[1:], nodf[1:])
    if c.lowp:
        b32 = _head_backward(bwd, t, t.feat.float(), fw, train, d["eps"])
        assert bw[0].dtype is R.LOWP[c.lowp] and torch.equal(bw[0], b32[0].to(bw[0].dtype)) and _same(bw[1:], b32[1:])
    assert not bool(bw[2][g0].any()) and not bool(bw[1][g0].any())              # dlin exactly 0 there: its sums are
    y = (c.fwd["lin"] - (c.fwd["mean"][:, None, :] if train else c.fwd["mean"])) * (c.fwd["invstd"][:, None, :] if train else c.fwd["invstd"]) \
        * d["bn_weight"].astype(np.float64) + d["bn_bias"].astype(np.float64)
    off = torch.from_numpy((y <= 0).all((0, 1))).to(dev)    # the output is 0 on every row of the column (the mask aside)
    assert not bool(out[:, :, off].any())
    assert not bool(bw[3][off].any()) and not bool(bw[4][off].any())
    if c.regime == "dead":
        assert bool(off.any()) and bool(g0.any())
    # accuracy of the backward.  Train mode: the entry computes on the state it is handed, so the float64 reference and the
    # float32 restatement (err32) both run on the kernel's own saved lin, mean and invstd -- on a constant column that is the
    # rounding the forward saved, times 316, and a yardstick on any other state measures numpy's sum order, not the entry.
    # Without constant columns the end-to-end float64 reference is held as well.  Train-mode d_bias is identically 0 under batch
    # statistics: a sum of T B terms of magnitude invstd |bn_weight| |dy| that cancels, rounding alone on every side (on the
    # device 1e-4 to 4e-3 of max(1, max |ref|), err32 on the same state 2e-5 to 2e-4).  Its accuracy is not asserted, as
    # tests/test_head_backward_gpu.py and tests/test_lstm_backward_gpu.py do not assert it there; it stays under the exact
    # assertions above (finite, the same bits twice and from the typed entry, exactly 0 on a dead channel).
    cases = []
    if train:
        state = (np_(lin), np_(mean), np_(inv))
        ref = dict(zip(R.HEAD_GRAD, head_backward_ref(d["d_out"], d["feat"], d["weight"], d["bn_weight"], d["bn_bias"], state[0],
                                                      mean=state[1], invstd=state[2], eps=d["eps"], mask=d["mask"])))
        r32 = R.head_restated(d, np.float32, state=state)
        cases.append((" (own state)", ref, {n: R.rel_err(r32[n], ref[n]) for n in R.HEAD_GRAD}, ("d_bias",)))
    if not const.any():
        cases.append(("", c.bwd, c.err32, ("d_bias",) if train else ()))
    rows2 = []
    for what, ref, e32s, skip in cases:
        for name, got in zip(R.HEAD_GRAD, bw):
            if name in skip:
                continue
            e32 = e32s[name]
            scale = max(1.0, float(np.abs(ref[name]).max()))
            err = float(np.abs(np_(got.float()) - ref[name]).max())
            bound = max(R.HEAD_TOL, 2 * e32) * scale
            if c.lowp and name == "d_feat":                  # rounded once to the 2-byte type (8 / 11 bits): half an ulp on top
                bound += (2.0 ** -8 if c.lowp == "bf16" else 2.0 ** -11) * scale
            rows2.append(("%s %s%s" % (tag, name, what), err / scale, e32, bound / scale, float(np.abs(ref[name]).max())))
    _report(rows + rows2)


@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("regime", R.HEAD_REGIMES)
@pytest.mark.parametrize("entry,shape", HEAD_CASES, ids=IDS)
def test_head(dev, entry, shape, regime, train):
    """head_forward / head_backward and head_forward_wide / head_backward_wide, fp32, with and without a mask"""
    for with_mask in (True, False):
        _check_head(dev, entry, R.head_case(regime, shape, train, with_mask))


@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("lowp", ["bf16", "fp16"])
@pytest.mark.parametrize("regime", R.HEAD_REGIMES + ("range16",))
@pytest.mark.parametrize("entry,shape", HEAD_CASES, ids=IDS)
def test_head_typed(dev, entry, shape, regime, lowp, train):
    """the typed entries on the same shapes and regimes, plus range16 (fp16: +-65504, subnormals, +-0; bf16: backbone)"""
    for with_mask in (True, False):
        c = R.head_case(regime, shape, train, with_mask, lowp)
        if regime == "range16" and lowp == "fp16":
            f = _head_tensors(c, dev).feat                   # the case does reach the device as drawn
            assert f.dtype is torch.float16 and bool((f == 65504).any()) and bool((f == -65504).any())
            assert bool(((f != 0) & (f.abs() < 2.0 ** -14)).any()) and bool(torch.signbit(f[f == 0]).any())
        _check_head(dev, entry, c)


@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("regime", R.HEAD_REGIMES)
def test_wide_head_has_the_narrow_bits(dev, regime, train):
    """(4,37,64,40), a shape both launches take: lin, and all of eval mode, bit for bit"""
    import ctc_amd
    for lowp in (None, "bf16"):
        c = R.head_case(regime, (4, 37, 64, 40), train, True, lowp)
        t = _head_tensors(c, dev)
        a = _head_forward(ctc_amd.head_forward, t, t.feat, c.d["eps"])
        b = _head_forward(ctc_amd.head_forward_wide, t, t.feat, c.d["eps"])
        torch.cuda.synchronize()
        assert torch.equal(a[1], b[1])
        if not train:
            assert _same(a, b)


# ---- the module -------------------------------------------------------------------------------------------------------

def _layers(dtype, hd, cd, K, C):
    lin, bn, cell = torch.nn.Linear(K, C), torch.nn.BatchNorm1d(C), torch.nn.LSTMCell(C, C)
    with torch.no_grad():
        for p, a in ((lin.weight, hd["weight"]), (lin.bias, hd["bias"]), (bn.weight, hd["bn_weight"]), (bn.bias, hd["bn_bias"]),
                     (cell.weight_ih, cd["w_ih"]), (cell.weight_hh, cd["w_hh"]), (cell.bias_ih, cd["b_ih"]), (cell.bias_hh, cd["b_hh"])):
            p.copy_(torch.from_numpy(a))
    return lin.to(dtype), bn.to(dtype), cell.to(dtype)


def _cpu_step(dtype, hd, cd, shape):
    """torch's own layers on the CPU in ``dtype``: Linear / BatchNorm1d / ReLU frame by frame, nn.LSTMCell in a loop, autograd"""
    T, B, K, C = shape
    lin, bn, cell = _layers(dtype, hd, cd, K, C)
    bn.train()
    f = torch.from_numpy(hd["feat"]).to(dtype).requires_grad_(True)
    h, c, hs = torch.from_numpy(cd["h0"]).to(dtype), torch.from_numpy(cd["c0"]).to(dtype), []
    for t in range(T):
        h, c = cell(torch.relu(bn(lin(f[t]))), (h, c))
        hs.append(h)
    series = torch.stack(hs)
    (series * torch.from_numpy(cd["d_series"]).to(dtype)[:, :, :C]).sum().backward()
    r = {"series": series, "d_feat": f.grad, "d_weight": lin.weight.grad, "d_bn_weight": bn.weight.grad, "d_bn_bias": bn.bias.grad,
         "d_w_ih": cell.weight_ih.grad, "d_w_hh": cell.weight_hh.grad, "d_b_ih": cell.bias_ih.grad, "d_b_hh": cell.bias_hh.grad,
         "running_mean": bn.running_mean, "running_var": bn.running_var}
    return {k: v.detach().double().numpy() for k, v in r.items()}


@pytest.mark.parametrize("shape", MODULE_SHAPES, ids=IDS)
def test_module_train_step(dev, monkeypatch, shape):
    """LSTM_cell, train mode, dropout off, every backward gate open: a padded head in front of a saturated cell, against the
    float64 CPU autograd of the same layers (the construction of test_lstm_cell_train_step_both_gates_open); err32: the same
    layers on the CPU in float32.  The Linear bias is identically 0 under batch statistics and skipped, as there."""
    import ctc_amd
    from ctc_amd import producer
    T, B, K, C = shape
    hd = R.head_case("padded", shape, True, False).d
    cd = R.rec_case("saturated", (T, B, C, C)).d
    ref, r32 = _cpu_step(torch.float64, hd, cd, shape), _cpu_step(torch.float32, hd, cd, shape)
    for gate in ("HEAD_BACKWARD_MAX_ROWS", "HEAD_WIDE_BACKWARD_MAX_ROWS", "HEAD_WIDE_MAX_ROWS", "SERIES_BACKWARD_MAX_ROWS",
                 "SERIES_WIDE_MAX_ROWS"):
        monkeypatch.setattr(producer, gate, OPEN)
    model = ctc_amd.LSTM_cell(types.SimpleNamespace(extract_feat_dim=K, v_class=C, batch_size=B, temporal=T)).train()
    model.v.layers[3].p = 0.0
    lin, bn, cell = _layers(torch.float32, hd, cd, K, C)
    model.v.layers[0].load_state_dict(lin.state_dict()); model.v.layers[1].load_state_dict(bn.state_dict())
    model.v_cell.load_state_dict(cell.state_dict())
    model = model.to(dev)
    names = ("ctc_amd_head_forward", "ctc_amd_head_forward_wide", "ctc_amd_head_backward", "ctc_amd_head_backward_wide",
             "ctc_amd_lstm_series", "ctc_amd_lstm_backward", "ctc_amd_lstm_series_wide", "ctc_amd_lstm_series_backward_wide",
             "ctc_amd_lstm_bias_grad_wide", "ctc_amd_lstm_cell_step")
    calls = {n: _counting(monkeypatch, n) for n in names}
    feat = tt(hd["feat"], dev).requires_grad_(True)
    series = model(feat, tt(cd["h0"], dev), tt(cd["c0"], dev))
    (series * tt(cd["d_series"], dev)[:, :, :C]).sum().backward()
    torch.cuda.synchronize()
    n = {k[8:]: len(v) for k, v in calls.items()}
    wide_head, wide_cell = B > 256, 2 * C > 80
    assert (n["head_forward"], n["head_forward_wide"], n["head_backward"], n["head_backward_wide"]) == \
        ((0, 1, 0, 1) if wide_head else (1, 0, 1, 0)), n
    # (lstm_series is asked first and refuses the wide shape: one call either way)
    assert (n["lstm_series"], n["lstm_backward"], n["lstm_series_wide"], n["lstm_series_backward_wide"], n["lstm_bias_grad_wide"],
            n["lstm_cell_step"]) == ((1, 0, 1, 1, 1, 0) if wide_cell else (1, 1, 0, 0, 0, 0)), n
    l0, l1, vc = model.v.layers[0], model.v.layers[1], model.v_cell
    got = {"series": series, "d_feat": feat.grad, "d_weight": l0.weight.grad, "d_bn_weight": l1.weight.grad, "d_bn_bias": l1.bias.grad,
           "d_w_ih": vc.weight_ih.grad, "d_w_hh": vc.weight_hh.grad, "d_b_ih": vc.bias_ih.grad, "d_b_hh": vc.bias_hh.grad}
    assert _finite(*got.values(), l0.bias.grad, l1.running_mean, l1.running_var)
    assert torch.equal(got["d_b_ih"], got["d_b_hh"]) and got["d_b_ih"].data_ptr() != got["d_b_hh"].data_ptr()
    rows = []
    for name, g in got.items():
        e32 = R.rel_err(r32[name], ref[name])
        rows.append(("LSTM_cell %s %s" % (IDS(shape), name), R.rel_err(np_(g), ref[name]), e32, max(R.HEAD_TOL, 2 * e32),
                     float(np.abs(ref[name]).max())))
    for name, g in (("running_mean", l1.running_mean), ("running_var", l1.running_var)):       # tests/test_producer_gpu.py: 1e-5 absolute
        rows.append(("LSTM_cell %s %s" % (IDS(shape), name), float(np.abs(np_(g) - ref[name]).max()),
                     float(np.abs(r32[name] - ref[name]).max()), 1e-5, float(np.abs(ref[name]).max())))
    _report(rows)
