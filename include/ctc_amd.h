/* ctc_amd.h -- C ABI of the MI355X-native CTC loss engine (libctc_amd.so).
 *
 * The drop-in boundary for the reference's loss path.  The reference has no FFI:
 * its loss is two Python nn.Modules (NoBlankCTC.py:22-141, NoBlankBinaryCTC.py:22-151)
 * called as  loss = ctc_loss(v_output, v_target, input_length, v_target_length)
 * (train.py:427, 576) followed by  loss.backward()  (train.py:444), plus
 * torch.nn.CTCLoss(blank=0) at models/layers/AsyncTFCriterion.py:198,319-321.
 * Each entry point below replaces one of those call sites' device work; the Python
 * host layer (ctc_amd/) binds them with ctypes and mirrors the modules' signatures.
 *
 * Conventions
 *  - plain pointers and sizes only; every pointer is a DEVICE pointer unless noted;
 *  - `stream` is a hipStream_t passed as void* (NULL = the null stream); calls only
 *    enqueue work: no allocation, no host synchronisation, graph-capture safe;
 *  - inputs are read-only; outputs are fully overwritten (grad rows t >= T_b get 0);
 *  - the caller owns all memory.  `workspace` must hold ctc_amd_workspace_bytes(...)
 *    bytes, be zero-filled ONCE when allocated, and not be shared by launches that
 *    may run concurrently (one workspace per stream); bytes [8,12) are the status word
 *    (ctc_amd_workspace_status), bytes [44,48) the gate word (ctc_amd_collective_gate);
 *  - return value: 0 on success, a hipError_t (> 0) from the launch, or one of the
 *    negative CTC_AMD_ERR_* codes; ctc_amd_error_string() describes any of them.
 *
 * Lengths and labels outside their range (every loss and every lattice read-out below; the library cannot check
 * device-resident values without a synchronisation, so every kernel guards itself; tests/test_bad_inputs_gpu.py):
 *  - lengths are compared as full int64 values.  A sample whose in_len is outside [1, T] or whose tgt_len is outside
 *    [1, S] (blank lattice: [0, S]) -- 0, negative, beyond the tensor, or a value beyond 32 bits whose low word would
 *    be valid -- is a sample WITHOUT AN ALIGNMENT, exactly like one that is too short (T_b < L_b): nothing of it is
 *    read beyond its lengths and labels, and it reports
 *      loss entries     nll >= 1e12 (blank lattice: +inf), never NaN; all T gradient rows exactly 0
 *      best paths       path -1 on all T frames, score -inf
 *      posteriors       nll >= 1e12 (blank lattice: +inf), never NaN; all T rows of gamma exactly 0
 *      token spans      nll +inf, path -1, score -inf, frame_conf 0, start / end -1, conf 0
 *    The other samples of the batch are not affected: they get, bit for bit, what they get beside a sample that is merely
 *    too short.  `loss` is the documented function of the nll the launch returned (so +inf with a blank-lattice
 *    sample of this kind in the batch, and a mean dominated by 1e13 on the other two).
 *    One difference, deliberate: ctc_amd_blank_loss_grad alone takes in_len = 0 -- with tgt_len = 0 that is the empty
 *    alignment of an empty target, nll = 0 (as torch); with tgt_len >= 1 no alignment.  The blank read-outs, which have
 *    no frame to report on, treat in_len = 0 like every other value outside [1, T].
 *  - labels are read by their LOW 32 BITS (an int64 label of 2^32 + k is class k), entries at l >= tgt_len[b] never.
 *    Inside tgt_len[b] a class outside [0, C) is made a class by the lattice's own rule:
 *      no-blank lattice  modulo C, negative values wrapping as a Python index does (-1 is class C - 1, C is class 0):
 *                        what the reference's lp[:, :, label] does for the negative ones
 *      blank lattice     clamped to [0, C - 1].  A clamp can land on the blank's class; such a label state emits the
 *                        blank's log-prob, is never entered by the skip edge (s - 2 -> s), and its occupancy goes to
 *                        the blank's column of the gradient -- one rule for the loss and the read-outs.  (torch would
 *                        read out of bounds, and for a target equal to the blank keeps the skip edge.)
 *    Either way the sample is computed as if the caller had passed those classes; nothing is flagged.
 *  - the Python layer (ctc_amd/) validates lengths it can see without a synchronisation (host tensors, lists) and
 *    raises ValueError before any launch; CTC_AMD_VALIDATE=1 extends that to device-resident lengths, at the cost
 *    of a synchronisation per call.  Labels are never validated.
 */
#ifndef CTC_AMD_H
#define CTC_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CTC_AMD_ABI_VERSION 2

#define CTC_AMD_ERR_BAD_ARGUMENT      (-1)  /* null pointer, non-positive size ... */
#define CTC_AMD_ERR_UNSUPPORTED_SHAPE (-2)  /* S > 256 (blank-CTC: 1023 for the loss, the best path and the posteriors); binary: T*S beyond LDS */
#define CTC_AMD_ERR_CODE_OVERFLOW     (-3)  /* target dedup in the reference's int32 row codes with C > 64: the
                                             * reference raises OverflowError there (2**o at o >= 64) */

/* variants for ctc_amd_workspace_bytes */
#define CTC_AMD_NOBLANK 0
#define CTC_AMD_BINARY  1
#define CTC_AMD_BLANK   2

int ctc_amd_abi_version(void);
const char *ctc_amd_error_string(int code);

/* Bytes of device workspace a call of this shape needs (>= 256: a header with the in-launch batch
 * reduction's words and the status word, then per-variant areas).  No-blank lattices that do not fit
 * in LDS (long sequences) and the blank-CTC lattice live in this workspace. */
size_t ctc_amd_workspace_bytes(int variant, int T, int B, int C, int S);

/* NoBlankCTC.forward (NoBlankCTC.py:129-141) + the gradient autograd would produce
 * for it (train.py:444), one fused launch.
 *   x        [T,B,C] fp32 raw logits, element strides stride_t / stride_b, unit
 *            stride over C (the module applies LogSoftmax(dim=2) itself, :136)
 *   labels   [B,S] class indices, int32 (labels_i64 = 0) or int64 (= 1); entries at
 *            l >= tgt_len[b] are never dereferenced (the dataset pads with -1)
 *   in_len   [B] int64, 1 <= T_b <= T        tgt_len [B] int64, 1 <= L_b <= S
 *            (a sample with a length outside these ranges has no alignment; labels outside [0, C) are taken modulo C:
 *            Conventions, "Lengths and labels outside their range")
 *   nll      [B]  out: -alpha[T_b-1, L_b-1]  (1e13 when no alignment exists)
 *   loss     [1]  out: loss_scale * sum_b nll[b]   (loss_scale = 1/B for the
 *            reference's batch mean :139-140; 1/B_global on a batch shard).  The sum is taken
 *            in-launch in FIXED POINT (order-independent, bitwise reproducible): every nll is
 *            rounded to a multiple of 2^-F, F = 27 - ceil(log2 B) fractional bits (B = 256: 2^-19,
 *            i.e. the loss is within 2^-20 of the exactly rounded mean; the reference's
 *            torch.mean is an fp32 sum in batch order).  nll[] itself and the gradient are
 *            not quantised.  Values that do not fit (>= 8192, the 1e13 sentinel, NaN) are
 *            added from memory in double.
 *   grad     [T,B,C] contiguous out, or NULL for a forward-only call:
 *            grad_scale * (softmax(x)[t,b,c] - sum_{l<L_b, lab[b,l]=c} gamma_t(l)),
 *            exactly 0 for t >= T_b and for samples with no alignment
 * -inf logits are allowed (a masked vocabulary), also on a label class: such a cell has probability 0, its gamma and
 * the gradient at the -inf entry are exactly 0.  A logit of -1e30 (the producer's pad value) on a label class counts the
 * same.  A sample is without an alignment when L_b > T_b or when every alignment crosses such a cell: nll >= 1e12, all
 * of its gradient rows exactly 0.  Which value >= 1e12 depends on the kernel the shape gets: the 1e13 sentinel, a
 * multiple of it, or the masked magnitude (about 1e30 times the cells crossed); callers test nll >= 1e12 (+inf passes
 * that test too, and the token spans report +inf).  The read-outs (best path, posteriors, token spans) follow the same
 * rule; the binary variant takes +-inf logits (p exactly 0 or 1, gradient exactly 0 there).  Outside the contract: a
 * live row whose logits are ALL -inf (its softmax is 0/0: NaN) and NaN logits (the loss is then NaN).
 */
int ctc_amd_noblank_loss_grad(const float *x, int64_t stride_t, int64_t stride_b,
                              const void *labels, int labels_i64,
                              const int64_t *in_len, const int64_t *tgt_len,
                              int T, int B, int C, int S,
                              float loss_scale, float grad_scale,
                              float *nll, float *loss, float *grad,
                              void *workspace, void *stream);

/* The label-smoothing variant sketched in comments at NoBlankCTC.py:100-107 ("the true class times lambda,
 * the others times (1 - lambda) / n_unit") and CrossEntropy.py: the emission of label position l becomes
 *   e[t,b,l] = lambda * lp[t,b,c_l] + (1 - lambda)/C * sum_{n != c_l} lp[t,b,n],   lp = LogSoftmax(x),
 * everything else as ctc_amd_noblank_loss_grad; grad = grad_scale * ((1 - b) softmax - a occupancy - b) with
 * b = (1 - lambda)/C, a = lambda - b.  The reference never runs this code (parity unpinned: checked against
 * the numpy restatement and finite differences).  Shapes: C even <= 256, S <= 31, T <= 168, 8-byte aligned
 * rows (the four-rows-per-wave kernel); others return CTC_AMD_ERR_UNSUPPORTED_SHAPE.  lambda in [0, 1].
 * Every one of the C columns counts as a class in the sum over n, so do not combine this entry with a pad column
 * (LSTM_cell(pad_classes=True): its lp = -1e30 enters every frame's emission and every sample reports nll >= 1e12).
 * For the same reason a -inf logit anywhere in a live row leaves the sample without an alignment here: nll >= 1e12
 * (+inf through such a row, never NaN) and all of its gradient rows exactly 0, as for every sample whose nll reaches
 * 1e12.  lambda = 1 is ctc_amd_noblank_loss_grad bit for bit; lambda <= 1 / (C + 1) (a <= 0) is defined on finite
 * logits only. */
int ctc_amd_noblank_smoothed_loss_grad(const float *x, int64_t stride_t, int64_t stride_b,
                                       const void *labels, int labels_i64,
                                       const int64_t *in_len, const int64_t *tgt_len,
                                       int T, int B, int C, int S, float label_smoothing,
                                       float loss_scale, float grad_scale,
                                       float *nll, float *loss, float *grad,
                                       void *workspace, void *stream);

/* Element types of the logits and the gradient for the typed entry points below. */
#define CTC_AMD_F32  0
#define CTC_AMD_BF16 1
#define CTC_AMD_F16  2

/* ctc_amd_noblank_loss_grad / ctc_amd_noblank_smoothed_loss_grad with the element type of x and grad as an argument
 * (mixed-precision training: logits under autocast come out in bf16 / fp16).  label_smoothing < 0: the plain loss;
 * in [0, 1]: the smoothed emission.  x_dtype CTC_AMD_F32 is exactly the untyped entries, every kernel and shape.
 * CTC_AMD_BF16 / CTC_AMD_F16: x [T,B,C] and grad [T,B,C] are 2-byte arrays (strides in elements); x is read as it
 * is and widened to fp32 in registers (exactly), the arithmetic is that of the fp32 launch, and grad is the fp32
 * value rounded once to nearest even -- on the same values nll, loss and grad are bitwise the fp32 launch's
 * nll, loss and grad converted to x_dtype.  nll and loss stay fp32.  Shapes: C even <= 256, S <= 31, T <= 168,
 * even strides, x and grad 4-byte aligned (the four-rows-per-wave kernel); others return
 * CTC_AMD_ERR_UNSUPPORTED_SHAPE.  Any other x_dtype: CTC_AMD_ERR_BAD_ARGUMENT. */
int ctc_amd_noblank_loss_grad_typed(const void *x, int x_dtype, int64_t stride_t, int64_t stride_b,
                                    const void *labels, int labels_i64,
                                    const int64_t *in_len, const int64_t *tgt_len,
                                    int T, int B, int C, int S, float label_smoothing,
                                    float loss_scale, float grad_scale,
                                    float *nll, float *loss, void *grad,
                                    void *workspace, void *stream);

/* NoBlankBinaryCTC.forward (NoBlankBinaryCTC.py:139-151) + gradient.  Same as above
 * except   y [B,S,C] fp32 multi-hot / soft targets in [0,1], contiguous;
 * emission = -BCELoss(sigmoid(x[t,b,:]), y[b,l,:]) (:112,:88, logs clamped at -100);
 * grad = grad_scale/C * (sigmoid(x) - sum_l gamma_t(l) y[b,l,c]).
 * A sample with a length outside [1, T] / [1, S]: no alignment, nll >= 1e12, gradient rows 0 (Conventions).
 */
int ctc_amd_binary_loss_grad(const float *x, int64_t stride_t, int64_t stride_b,
                             const float *y,
                             const int64_t *in_len, const int64_t *tgt_len,
                             int T, int B, int C, int S,
                             float loss_scale, float grad_scale,
                             float *nll, float *loss, float *grad,
                             void *workspace, void *stream);

/* torch.nn.CTCLoss(blank, reduction='mean', zero_infinity=False) as used at
 * models/layers/AsyncTFCriterion.py:198,319-321 (padded [B,S] targets).
 *   log_probs [T,B,C] fp32, already normalised; targets [B,S] int32/int64
 *   in_len [B] int64, 0 <= T_b <= T; tgt_len [B] int64, 0 <= L_b <= S.  A length outside these ranges: no alignment
 *         (nll = +inf, gradient rows 0); targets outside [0, C) inside L_b are clamped to [0, C-1], and one that lands
 *         on the blank's class is never skipped into (Conventions, "Lengths and labels outside their range")
 *   nll   [B]  out: un-normalised negative log-likelihood (+inf if infeasible)
 *   loss  [1]  out: loss_scale * sum_b nll[b] / max(L_b,1)
 *   grad  [T,B,C] out or NULL: (exp(lp) - occupancy) * grad_scale / max(L_b,1)
 * -inf log-probs are allowed (a masked vocabulary): the gradient at a -inf entry is exactly 0 (both terms are).  A sample
 * with no alignment -- through its lengths (T_b < L_b + adjacent repeats) or through its emissions (every path crosses a
 * -inf entry; an empty target whose blank has a hole) -- has nll = +inf and an all-zero gradient, where torch gives NaN;
 * the other samples of the batch are not touched by it (loss, their sum, is +inf).
 * NaN log-probs are outside the contract and, unlike the no-blank and binary losses, do not make the loss NaN: the max-based
 * log-sum-exp of the lattice drops a NaN cell, so the sample reports +inf, or a finite nll over the paths that avoid the cell.
 * 1 <= S <= 1023 label columns (2S+1 <= 2047 lattice states; CTC_AMD_ERR_UNSUPPORTED_SHAPE beyond, and when C no
 * longer fits beside the padded lattice row in a gradient wave's LDS: 4 (C + 2 NSP) floats <= 160 KB, NSP = 512 for
 * S <= 255).  Up to 255 labels a chain is one wave; 256..1023 labels take the WIDE path: three launches, a chain
 * spread over 2..4 waves of one workgroup (512 states each, NSP = 512 ceil((2S+1)/512)) that hand their edge states
 * on through LDS with one workgroup barrier per step -- no polling, so no bounded wait and no status bit there;
 * ctc_amd_blank_set_schedule() does not apply to it.  Everything else in this comment holds for both.  Of the read-outs
 * below the best path and the posteriors follow to S = 1023 (ctc_amd_blank_best_path_wide,
 * ctc_amd_blank_posteriors_wide): one width limit for the loss, the alignment and the posteriors.
 * Long sequences (T >= 256) on batches of #CUs/11..#CUs/2 samples with >= 4 lattice states per lane and
 * B*C >= 16384 (BASELINE config 5 and its neighbourhood) run as ONE persistent
 * launch of at most one workgroup per CU in which workgroups wait for each other (bounded: a wait
 * that runs out poisons nll / grad with NaN instead of hanging).  Kernels of other streams on the
 * same device can only delay it; the workspace belongs to one call in flight at a time, as for every
 * entry point.  ctc_amd_blank_set_schedule() forces / forbids that schedule.
 * Accuracy: the lattice scans are fp32 in the log2 domain, like torch's own fp32 kernels, and lose resolution with T
 * (alpha reaches -2e4 at T = 2000, where one ulp is 2e-3): the gradient of the BATCH-MEAN loss is within 1e-4 of float64
 * at every tested shape (8e-6 at BASELINE config 5, where torch's fp32 CPU kernel is 1.9e-4 off), but the un-normalised
 * per-sample occupancies behind it -- grad * max(L_b,1) / grad_scale -- are only good to ~1e-2 at T = 2000 (7e-3
 * measured).  A caller that rescales the gradient per sample by factors >> 1 inherits that.
 * Peaked inputs (a trained model; a peak on the wrong class with nll up to 3.7e4; -inf entries) cost no accuracy: measured
 * 1.1e-5 at most against float64 on every path, T <= 660, where torch's fp32 CPU kernel is up to 1.6e-3 off
 * (tests/test_blank_inputs_gpu.py).
 * Wide path (S > 255): the same arithmetic step for step, plus one exact cross-wave sum at the end.  Its accuracy has not
 * been measured on a device yet; the tests hold its batch-mean gradient to twice the error of torch's own fp32 CPU kernel
 * against float64 on the same inputs (1.1e-6 .. 4.9e-6 on the tested shapes up to T = 1250, S = 1023), and never looser
 * than the narrow path's bound.
 */
int ctc_amd_blank_loss_grad(const float *log_probs, int64_t stride_t, int64_t stride_b,
                            const void *targets, int targets_i64,
                            const int64_t *in_len, const int64_t *tgt_len,
                            int T, int B, int C, int S, int blank,
                            float loss_scale, float grad_scale,
                            float *nll, float *loss, float *grad,
                            void *workspace, void *stream);

/* Schedule of the long-sequence blank-CTC path: -1 = the library's own choice (default), 1 / 0 = force /
 * forbid the single persistent launch, 2 = force it with the worker pool gathering the emission rows (the
 * library's own choice around BASELINE config 5) (tests and measurements; process-wide, thread-safe).  The
 * environment variable CTC_AMD_BLANK_FUSED=1 / 0, read ONCE at first use, sets the initial value. */
int ctc_amd_blank_set_schedule(int mode);

/* In-launch hand-offs between waves / workgroups wait with a bound (~1 s).  A wait that runs out never
 * yields a plausible number: the outputs that could not be produced are filled with NaN (nll of the
 * sample, the loss, the sample's gradient rows) and a bit is ORed into the workspace's STATUS word, which
 * stays set until cleared here.  Reads the word (synchronising `stream`); clear != 0 resets it.
 * Bits: 1 no-blank, 2 binary, 4 blank-CTC launch starved, 8 blank-CTC best path starved (that sample's score NaN,
 * its path -1), 16 blank-CTC posteriors (that sample's nll and gamma rows NaN; reserved: its launches hand rows over
 * at kernel boundaries only and have no in-launch wait, so nothing sets it today).  Never observed outside
 * fault-injection builds;
 * the persistent blank-CTC launch is the one place where another process's kernels could cause it. */
int ctc_amd_workspace_status(void *workspace, int clear, void *stream, unsigned *status_host);

/* Collective gate (batch-sharded use, one process per GPU): keeps a collective from taking CUs away from the
 * NEXT loss launch.  The no-blank / binary launch at B >= #CUs wants every CU (one 1024-thread workgroup, 122 KB
 * of LDS, 288 of a SIMD's 512 registers per lane); RCCL's collective kernel (256 threads, 19.7 KB of LDS, 261-280
 * registers per lane) cannot share a CU with such a workgroup, so an all-reduce that is dispatched just BEFORE
 * the launch costs it a whole second round of workgroups (measured: 15 -> 23 us per launch with one resident
 * collective workgroup; dispatched after the launch has filled the chip it costs nothing).  Enqueue this on the
 * stream the collective will be ordered behind, AFTER the previous loss launch and BEFORE the collective: a
 * one-wave kernel that returns once min(B, #CUs) workgroups of the loss launch that uses `workspace` have
 * started, or after timeout_us (bounded: never gate a collective that no loss launch follows).  Counting is
 * switched on by the first gate used on a workspace (the loss launches of a workspace that never saw a gate pay
 * nothing for it; the launch right after the first gate is not counted yet and that gate runs into its bound):
 * every no-blank / binary workgroup then counts itself at entry in sixteen sharded words of the workspace, the
 * launch's last workgroup puts them back to 0.  The blank-CTC launches do not count (a collective is short against
 * them). */
int ctc_amd_collective_gate(void *workspace, int B, int timeout_us, void *stream);

/* backward of the autograd.Function: grad[i] *= *grad_out (a device scalar, the
 * upstream gradient of the 0-dim loss).  Every workgroup reads *grad_out and exits
 * at once when it is exactly 1.0f (the loss.backward() case, train.py:444), so the
 * common case moves no data and needs no host synchronisation.
 *
 * Under stream capture the call may add no node at all: it is FOLDED into the loss launch it
 * scales when (1) `stream` is capturing, (2) the call is issued directly behind a *_loss_grad
 * launch captured on that same stream -- nothing else has been captured or joined in behind that
 * launch -- (3) grad, n (and dtype, for the typed form) are exactly that launch's gradient buffer,
 * element count (T * B * C) and element type, (4) it is the first scale call behind that launch and
 * (5) the launched kernel takes the pointer (the no-blank r16 kernel in every form and the streamed
 * binary kernel: the kernels of the default plans for S <= 31 / S <= 64; not blank CTC).  The loss
 * kernel's graph node then receives `grad_out` as a kernel argument and multiplies every gradient
 * value by *grad_out as it stores it -- read on the device at every replay, never a captured value,
 * and with the second rounding of the scale kernel, so the result has the bits of the two launches;
 * nll and loss are not scaled.  `grad_out` must stay valid for as long as the graph is replayed, as
 * it must for the scale kernel's node.  An eager call, and every captured call that does not meet the
 * conditions, launches the scale kernel as before; the answer is the same either way. */
int ctc_amd_scale_grad(float *grad, const float *grad_out, size_t n, void *stream);

/* ctc_amd_scale_grad for a gradient of element type `dtype` (CTC_AMD_F32 / _BF16 / _F16, as
 * ctc_amd_noblank_loss_grad_typed wrote it): the same exit when *grad_out == 1.0f, otherwise
 * grad[i] = round_to_nearest_even(float(grad[i]) * *grad_out). */
int ctc_amd_scale_grad_typed(void *grad, int dtype, const float *grad_out, size_t n, void *stream);

/* Best-path (Viterbi) alignment on the no-blank lattice: the max-semiring twin of
 * the alpha recursion (the reference evaluates with per-step argmax and
 * DTW-like helpers, train.py:82-136,434).
 *   path  [B,T] int32 out: label position l_t of the best alignment for t < T_b,
 *         -1 for t >= T_b or when no alignment exists
 *   score [B]   out: log-probability of that alignment
 * Lengths outside [1, T] / [1, S]: no alignment (path -1 on all T frames, score -inf); labels outside [0, C): modulo C
 * (Conventions).
 */
int ctc_amd_noblank_best_path(const float *x, int64_t stride_t, int64_t stride_b,
                              const void *labels, int labels_i64,
                              const int64_t *in_len, const int64_t *tgt_len,
                              int T, int B, int C, int S,
                              int32_t *path, float *score,
                              void *workspace, void *stream);

/* The same on the lattice of the binary variant (SURVEY 8f-1 for NoBlankBinaryCTC): y [B,S,C] float label rows;
 * cell (t, l) costs -nn.BCELoss()(sigmoid(x[t,b,:]), y[b,l,:]) (NoBlankBinaryCTC.py:112,:88,:146).  path [B,T] (label-row
 * positions, -1 behind T_b or when no alignment exists), score [B] its log-probability.  Lengths outside their range: no
 * alignment, as above. */
int ctc_amd_binary_best_path(const float *x, int64_t stride_t, int64_t stride_b, const float *y,
                             const int64_t *in_len, const int64_t *tgt_len,
                             int T, int B, int C, int S,
                             int32_t *path, float *score, void *workspace, void *stream);

/* Token spans on the no-blank lattice: one record per label of the transcript -- the frame where the best alignment
 * starts it, the frame where it ends, and how sure the model is -- in ONE launch, without gamma [B,T,S] ever being
 * written.  Inputs: those of ctc_amd_noblank_best_path (float32 logits, stride over classes 1; int32 / int64 labels,
 * negative ones inside L_b wrap as there).  Every element of every output is written; nothing needs clearing.
 *   path       [B,T] int32, score [B]: what ctc_amd_noblank_best_path writes for the same inputs, bit for bit (the same
 *              emission stage and the same max-scan): -1 for t >= T_b, -1 / -inf for a sample without an alignment
 *   nll        [B]: -alpha[T_b-1, L_b-1], the chain of ctc_amd_noblank_loss_grad; +inf for a sample without an
 *              alignment (L_b > T_b, lengths outside the tensor) -- the loss itself reports the reference's sentinel
 *              magnitude (1e13) there
 *   frame_conf [B,T] fp32: gamma_t(path_t), the row-normalised posterior exp(alpha_t(l) + beta'_t(l) - e_t(l)) /
 *              sum_l' (same) at the state the best path occupies; 0 where path is -1
 *   start, end [B,S] int32: label j < L_b of an aligned sample owns the frames start .. end-1, the t < T_b with
 *              path[b,t] = j; every such label owns at least one frame and the spans partition [0, T_b):
 *              start[b,0] = 0, end[b,j] = start[b,j+1], end[b,L_b-1] = T_b.  -1 / -1 for j >= L_b and for every j of a
 *              sample without an alignment
 *   conf       [B,S] fp32: the sum of frame_conf[b,t] over t = start .. end-1 -- from 0.0f, in ascending t, in fp32 --
 *              followed by one correctly rounded fp32 division by float(end - start); 0 where start is -1.  The order is
 *              part of the contract: a float32 loop in that order reproduces the bits (as ctc_amd_blank_token_spans).
 * The class of span j is labels[b,j].  One 1024-thread workgroup per sample holds the sample's lattice in LDS: S <= 256,
 * and ((3T + 8) SP + 2T + 3SP + 8) * 4 + T * SP + 16 bytes <= 160 KB, SP = S rounded up to the states per lane (1, 2, 4
 * for S <= 64, 128, 256) -- 13 bytes per lattice cell, T = 150 at every S <= 64; CTC_AMD_ERR_UNSUPPORTED_SHAPE beyond.
 * Null pointers and T, B, C, S < 1 return CTC_AMD_ERR_BAD_ARGUMENT before anything is dereferenced or launched.
 * `workspace` is ignored and may be NULL.  No atomics, no waiting between workgroups: deterministic.
 * Lengths outside [1, T] / [1, S]: a sample without an alignment (nll +inf, path -1, score -inf, frame_conf 0, spans -1 / -1,
 * conf 0); labels outside [0, C) inside L_b: modulo C, read by their low 32 bits (Conventions). */
int ctc_amd_noblank_token_spans(const float *x, int64_t stride_t, int64_t stride_b,
                                const void *labels, int labels_i64,
                                const int64_t *in_len, const int64_t *tgt_len,
                                int T, int B, int C, int S,
                                int32_t *path, float *score, float *nll, float *frame_conf,
                                int32_t *start, int32_t *end, float *conf,
                                void *workspace, void *stream);

/* The same on the lattice of the binary variant: y [B,S,C] float label rows, path / score those of
 * ctc_amd_binary_best_path bit for bit, nll the chain of ctc_amd_binary_loss_grad; the class of span j is row j of y.
 * LDS: the bound above with the label table replaced by the waves' row buffers,
 * ((3T + 8) SP + 2T + 2SP + 16 C + 8) * 4 + T * SP + 16 bytes <= 160 KB (T = 150 at every S <= 64 and C <= 256; no
 * T <= 168 limit as in ctc_amd_binary_posteriors). */
int ctc_amd_binary_token_spans(const float *x, int64_t stride_t, int64_t stride_b, const float *y,
                               const int64_t *in_len, const int64_t *tgt_len,
                               int T, int B, int C, int S,
                               int32_t *path, float *score, float *nll, float *frame_conf,
                               int32_t *start, int32_t *end, float *conf,
                               void *workspace, void *stream);

/* Best-path (Viterbi) forced alignment on the blank-CTC lattice (torch.nn.CTCLoss semantics, as
 * ctc_amd_blank_loss_grad): which frame belongs to which label of a KNOWN target sequence, and the score of that
 * alignment.  Inputs: the same layout and contract as ctc_amd_blank_loss_grad (log_probs used as given, no
 * normalisation; 0 <= L_b <= S, 1 <= T_b <= T).  Extended labels l'_s, s = 0..2L (even s = blank, odd s = label
 * (s-1)/2):  v_0(0) = lp[0,blank], v_0(1) = lp[0,l'_1], others -inf;  v_t(s) = best(v_{t-1}(s), v_{t-1}(s-1),
 * [v_{t-1}(s-2) when l'_s != blank and l'_s != l'_{s-2}]) + lp[t,l'_s], candidates in the order stay, advance, skip,
 * a later one taken only when strictly greater; one fp32 add per step (natural log, -inf kept).
 *   path  [B,T] int32 out: state s_t of the best alignment for t < T_b (the final state is 2L when
 *         v(2L) > v(2L-1), else 2L-1; 0 when L = 0), -1 for t >= T_b and for samples with no alignment
 *   score [B]   out: v of the final state (-inf: no alignment -- too short for L plus its adjacent repeats, or every
 *         path crosses a -inf log-prob, e.g. a label's class masked on every frame; the path is -1 on every frame either
 *         way, exactly the samples for which ctc_amd_blank_loss_grad gives nll = +inf).  A length outside [1, T] /
 *         [0, S]: the same (path -1 on all T frames, score -inf); targets outside [0, C) are clamped (Conventions)
 * workspace: at least ctc_amd_workspace_bytes(CTC_AMD_BLANK, T, B, C, S) bytes; the 256-byte header is left alone
 * except for status bit 8.  S <= 255 (CTC_AMD_ERR_UNSUPPORTED_SHAPE beyond: 256..1023 label columns are
 * ctc_amd_blank_best_path_wide's), any T (back-pointers beyond LDS go to the workspace). */
int ctc_amd_blank_best_path(const float *log_probs, int64_t stride_t, int64_t stride_b,
                            const void *targets, int targets_i64,
                            const int64_t *in_len, const int64_t *tgt_len,
                            int T, int B, int C, int S, int blank,
                            int32_t *path, float *score, void *workspace, void *stream);

/* ctc_amd_blank_best_path for 256 <= S <= 1023 label columns (513 <= 2S+1 <= 2047 lattice states, the widths of
 * ctc_amd_blank_loss_grad's wide path; CTC_AMD_ERR_UNSUPPORTED_SHAPE outside that range -- S <= 255 is the entry
 * above).  The same inputs, the same contract and the same arithmetic step for step: v_t(s) with the candidates in
 * the order stay, advance, skip, a later one taken only when strictly greater, one fp32 add per step in natural log,
 * -inf kept; the final state is 2L when v(2L) > v(2L-1), else 2L-1 (0 when L = 0).  A sample's path and score do not
 * depend on which of the two entries served it (L_b <= 255 inside a wide call included).
 *   path  [B,T] int32 out: state s_t for t < T_b, -1 for t >= T_b and for samples with no alignment
 *   score [B]   out: v of the final state (-inf: no alignment)
 * Null pointers, T, B, C, S < 1 and a blank outside [0, C) return CTC_AMD_ERR_BAD_ARGUMENT before anything is
 * dereferenced or launched.  One workgroup of ceil((2S+1)/512) waves per sample; the waves hand their edge state on
 * through LDS with one workgroup barrier per step -- no polling, so no bounded wait, and no status bit is ever set.
 * workspace: at least ctc_amd_workspace_bytes(CTC_AMD_BLANK, T, B, C, S) bytes; only the lattice areas behind the
 * 256-byte header are written (the emission table and the back-pointers: (288 W + 4) of their 1536 W words per
 * (b, t), W = ceil((2S+1)/512)), not the header and not the loss's state tables and hand-off words behind the areas.
 * Any T.  Deterministic. */
int ctc_amd_blank_best_path_wide(const float *log_probs, int64_t stride_t, int64_t stride_b,
                                 const void *targets, int targets_i64,
                                 const int64_t *in_len, const int64_t *tgt_len,
                                 int T, int B, int C, int S, int blank,
                                 int32_t *path, float *score, void *workspace, void *stream);

/* Per-frame state posteriors on the blank-CTC lattice: gamma_t(s) = P(state s at frame t | log_probs, targets), the soft
 * alignment beside ctc_amd_blank_best_path's hard one.  Inputs: the same layout and contract as ctc_amd_blank_loss_grad
 * and ctc_amd_blank_best_path (log_probs used as given; stride over classes 1; 0 <= L_b <= S, 1 <= T_b <= T).
 * Extended labels l'_s, s = 0..2L (even s = blank, odd s = label (s-1)/2).  alpha_0(0) = lp[0,blank],
 * alpha_0(1) = lp[0,l'_1], others -inf; alpha_t(s) = LSE(alpha_{t-1}(s), alpha_{t-1}(s-1), [alpha_{t-1}(s-2) when
 * l'_s != blank and l'_s != l'_{s-2}]) + lp[t,l'_s].  beta' leaves out the emission of its own step:
 * beta'_{T_b-1}(2L) = beta'_{T_b-1}(2L-1) = 0 (state 0 only when L = 0), others -inf, and the mirror recursion over the
 * successors s, s+1, [s+2 under the same skip rule], each carrying its emission lp[t+1, l'_.].
 *   nll   [B] out: -LSE(alpha_{T_b-1}(2L), alpha_{T_b-1}(2L-1)), as ctc_amd_blank_loss_grad writes it (+inf: no alignment,
 *         a length outside [1, T] / [0, S] included: all T rows of gamma are 0 then; Conventions)
 *   gamma [B,T,2S+1] fp32 contiguous out: exp(alpha_t(s) + beta'_t(s) + nll) for t < T_b, s <= 2L_b, formed as
 *         alpha + beta' normalised per row; exactly 0 for t >= T_b, s > 2L_b, at states no path passes through and on
 *         every row of a sample with no alignment (L_b = 0: gamma[b,t,0] = 1 for t < T_b)
 * The chains are fp32 but rescaled (the row maximum subtracted every few steps, alpha's offsets summed in double for
 * nll), so gamma keeps its resolution at long T: within 5e-4 of float64 at T = 2000 (the loss's occupancies: ~1e-2).
 * workspace: at least ctc_amd_workspace_bytes(CTC_AMD_BLANK, T, B, C, S) bytes; only the lattice areas behind the
 * 256-byte header are written (not the loss's state tables and hand-off words behind them; the header is left alone
 * except for status bit 16).  S <= 255 (CTC_AMD_ERR_UNSUPPORTED_SHAPE beyond: 256..1023 label columns are
 * ctc_amd_blank_posteriors_wide's), any T.  Deterministic. */
int ctc_amd_blank_posteriors(const float *log_probs, int64_t stride_t, int64_t stride_b,
                             const void *targets, int targets_i64,
                             const int64_t *in_len, const int64_t *tgt_len,
                             int T, int B, int C, int S, int blank,
                             float *nll, float *gamma, void *workspace, void *stream);

/* ctc_amd_blank_posteriors for 256 <= S <= 1023 label columns (513 <= 2S+1 <= 2047 lattice states, the widths of
 * ctc_amd_blank_loss_grad's wide path and of ctc_amd_blank_best_path_wide; CTC_AMD_ERR_UNSUPPORTED_SHAPE outside that
 * range -- S <= 255 is the entry above).  The same inputs, outputs and contract, the same arithmetic step for step.
 * Null pointers, T, B, C, S < 1 and a blank outside [0, C) return CTC_AMD_ERR_BAD_ARGUMENT before anything is
 * dereferenced or launched, and before the range of S is looked at.
 * W = ceil((2S+1)/512) waves span a lattice row.  alpha and beta' run in two workgroups of W waves per sample; the
 * waves hand their edge states on through LDS with one workgroup barrier per step -- no polling, so no bounded wait, and
 * no status bit is ever set (bit 16 stays reserved).  What is subtracted from the chains is the same in every wave of a
 * sample: the per-frame emission maximum is formed once per row by the gather launch, and the state maximum taken off
 * every few steps is the maximum over all W waves (exchanged through LDS with a step's hand-off), so alpha' + beta' has
 * no seam where two waves meet.  gamma is normalised per row over all 2S+1 states.
 * workspace: at least ctc_amd_workspace_bytes(CTC_AMD_BLANK, T, B, C, S) bytes; only the lattice areas behind the
 * 256-byte header are written (the emission table and the alpha' / beta' rows: (1280 W + 4) of their 1536 W words per
 * (b, t)), not the header and not the loss's state tables and hand-off words behind the areas.  Any T.  Deterministic. */
int ctc_amd_blank_posteriors_wide(const float *log_probs, int64_t stride_t, int64_t stride_b,
                                  const void *targets, int targets_i64,
                                  const int64_t *in_len, const int64_t *tgt_len,
                                  int T, int B, int C, int S, int blank,
                                  float *nll, float *gamma, void *workspace, void *stream);

/* Token spans on the blank-CTC lattice: one record per target label -- where the best alignment puts it and how sure
 * the model is -- from ctc_amd_blank_best_path's path and ctc_amd_blank_posteriors' gamma in ONE call, without gamma
 * [B,T,2S+1] ever being written.  Inputs: the same layout and contract as ctc_amd_blank_best_path (log_probs used as
 * given; stride over classes 1; 0 <= L_b <= S, 1 <= T_b <= T).  1 <= S <= 1023: up to 255 label columns run the narrow
 * kernels, 256..1023 the wide ones, chosen here.  Every element of every output is written.
 *   path       [B,T] int32, score [B]: what ctc_amd_blank_best_path / _wide write for the same inputs, bit for bit
 *   nll        [B]: what ctc_amd_blank_posteriors / _wide write, bit for bit
 *   frame_conf [B,T] fp32: gamma[b, t, path[b,t]] -- the very value the posteriors entry stores at that position (the
 *              same z * inv of the same row maximum and row sum); 0 where path[b,t] = -1
 *   start, end [B,S] int32: for label j < L_b of a sample with an alignment, start = the first frame t with
 *              path[b,t] = 2j+1 and end = one past the last (the path is monotone: those frames are contiguous and there
 *              is at least one); -1 / -1 for j >= L_b and for every j of a sample with no alignment or with lengths out
 *              of contract
 *   conf       [B,S] fp32: the sum of frame_conf[b,t] over t = start .. end-1 -- from 0.0f, in ascending t, in fp32 --
 *              followed by one correctly rounded fp32 division by float(end - start); 0 where start is -1.  The order is
 *              part of the contract: a float32 loop in that order reproduces the bits.
 * The class of span j is targets[b,j].  Samples with no alignment or with lengths out of contract get in path, score,
 * nll and frame_conf what the two entries above leave there (path -1, score -inf, nll +inf, frame_conf 0).
 * Null pointers, T, B, C, S < 1 and a blank outside [0, C) return CTC_AMD_ERR_BAD_ARGUMENT before anything is
 * dereferenced or launched, and before S is looked at; S > 1023, or a lattice that does not fit the workspace,
 * CTC_AMD_ERR_UNSUPPORTED_SHAPE.
 * Launches, all on `stream`: the best path's (gather, scan + walk back), the posteriors' chains on the lattice areas the
 * back-pointers have left (S <= 255: on the best path's own table, one gather for both; wider: behind a gather of
 * their own), one launch that forms each gamma row as ctc_amd_blank_posteriors does and stores the one selected value,
 * one launch that turns path and frame_conf into the spans.  No workgroup waits on another in the two new launches; the
 * narrow best path and chains may raise their status bits 8 and 16 as in their own entries, the wide stages raise none.
 * workspace: at least ctc_amd_workspace_bytes(CTC_AMD_BLANK, T, B, C, S) bytes; only the lattice areas behind the
 * 256-byte header are written.  Any T.  Deterministic. */
int ctc_amd_blank_token_spans(const float *log_probs, int64_t stride_t, int64_t stride_b,
                              const void *targets, int targets_i64,
                              const int64_t *in_len, const int64_t *tgt_len,
                              int T, int B, int C, int S, int blank,
                              int32_t *path, float *score, float *nll, float *frame_conf,
                              int32_t *start, int32_t *end, float *conf,
                              void *workspace, void *stream);

/* Target construction: the dedup step of the reference's dataset preparation,
 * datasets/charades_ctc_next_pred.py:646-651,663-678 (same code at :503-505,523-531) -- out[b] = the rows of
 * rows[b] whose code is new, in order of first appearance, remaining rows filled with -1 (:676-678);
 * length[b] = how many.  rows, out: [B,S,C] int32; length [B] int64.  No workspace.
 *   exact_rows = 0 (the reference's arithmetic, bit-exact at every C <= 64): rows are compared through the
 *     int32 code  sum_o row[o] * 2**o  as torch accumulates it into an IntTensor -- wrapped to 32 bits, so
 *     class 31 is the sign bit and classes 32..63 drop out (opts.py:60-61 default to 38 / 33 classes: rows
 *     that differ only there collide, rows made only of them never enter); a row enters when its code is
 *     not among the kept codes, an array that starts as zeros (code 0 never enters).  C > 64 returns
 *     CTC_AMD_ERR_CODE_OVERFLOW: the reference raises OverflowError at 2**64.
 *   exact_rows = 1: rows compared exactly over all C classes (which classes are non-zero), any C. */
int ctc_amd_dedup_multihot_targets(const int32_t *rows, int B, int S, int C, int exact_rows,
                                   int32_t *out, int64_t *length, void *stream);

/* Per-step posteriors of the no-blank lattice: gamma[b,t,l] = P(state l at step
 * t | x, targets) = exp(alpha_t(l) + beta_t(l) + nll), the quantity the loss gradient scatters
 * by class; rows sum to 1 for t < T_b and are 0 beyond T_b / L_b.  Same inputs as
 * ctc_amd_noblank_loss_grad; gamma is [B,T,S] fp32 contiguous; nll [B] is also produced.  A sample with a length
 * outside [1, T] / [1, S]: nll >= 1e12, all T rows of gamma 0; labels outside [0, C): modulo C (Conventions). */
int ctc_amd_noblank_posteriors(const float *x, int64_t stride_t, int64_t stride_b,
                               const void *labels, int labels_i64,
                               const int64_t *in_len, const int64_t *tgt_len,
                               int T, int B, int C, int S,
                               float *nll, float *gamma,
                               void *workspace, void *stream);

/* The same for the binary lattice (NoBlankBinaryCTC): gamma[b,t,l] = P(target row l at step t | x, y) -- what the
 * binary loss gradient contracts with the target rows.  y [B,S,C] as ctc_amd_binary_loss_grad; gamma [B,T,S], nll [B].
 * Shapes of the pipelined binary kernel only (S <= 64, T <= 168, C <= 256, LDS images fit); others return
 * CTC_AMD_ERR_UNSUPPORTED_SHAPE.  Lengths outside their range: as ctc_amd_noblank_posteriors. */
int ctc_amd_binary_posteriors(const float *x, int64_t stride_t, int64_t stride_b, const float *y,
                              const int64_t *in_len, const int64_t *tgt_len,
                              int T, int B, int C, int S,
                              float *nll, float *gamma,
                              void *workspace, void *stream);

/* The read-outs of the no-blank and the binary lattice on typed logits: each entry below is its untyped sibling's
 * argument list with (const void *x, int x_dtype) in place of (const float *x) -- the convention of
 * ctc_amd_noblank_loss_grad_typed and of the typed head entries.  A model trained under autocast hands its logits
 * over in bf16 / fp16, and the read-outs take them as they lie instead of an fp32 copy.
 *   x_dtype CTC_AMD_F32: exactly the untyped entry -- the same kernel, the same instantiation, the same answers.
 *   CTC_AMD_BF16 / CTC_AMD_F16: x [T,B,C] is a 2-byte array, strides in elements, stride over the classes 1.  Every kernel
 *     reads each logit with ONE 2-byte load by the lane that read the fp32 element and widens it exactly (bf16: a 16-bit
 *     shift; fp16: the exact conversion, subnormals kept); everything behind that load is the fp32 kernel's code.  So
 *     every output is BIT FOR BIT what the untyped entry writes for the fp32 image of x (NaN logits aside).
 *   Any other x_dtype: CTC_AMD_ERR_BAD_ARGUMENT, before anything else is looked at.
 * Outputs keep their types: path / start / end int32; score, nll, gamma, frame_conf, conf fp32.  Null pointers and T, B,
 * C, S < 1: CTC_AMD_ERR_BAD_ARGUMENT; S > 256: CTC_AMD_ERR_UNSUPPORTED_SHAPE -- all before any HIP call.
 * Shape domains for 2-byte x:
 *   best paths, token spans, binary posteriors: those of the untyped entry -- any C, any strides, x 2-byte aligned, the
 *     same LDS bounds.
 *   ctc_amd_noblank_posteriors_typed: the four-rows-per-wave kernel only, as ctc_amd_noblank_loss_grad_typed -- C even
 *     <= 256, S <= 31, T <= 168, even strides, x 4-byte aligned, arrays within LDS; CTC_AMD_ERR_UNSUPPORTED_SHAPE
 *     otherwise (the untyped entry on an fp32 copy takes every shape). */
int ctc_amd_noblank_best_path_typed(const void *x, int x_dtype, int64_t stride_t, int64_t stride_b,
                                    const void *labels, int labels_i64,
                                    const int64_t *in_len, const int64_t *tgt_len,
                                    int T, int B, int C, int S,
                                    int32_t *path, float *score,
                                    void *workspace, void *stream);
int ctc_amd_binary_best_path_typed(const void *x, int x_dtype, int64_t stride_t, int64_t stride_b, const float *y,
                                   const int64_t *in_len, const int64_t *tgt_len,
                                   int T, int B, int C, int S,
                                   int32_t *path, float *score, void *workspace, void *stream);
int ctc_amd_noblank_token_spans_typed(const void *x, int x_dtype, int64_t stride_t, int64_t stride_b,
                                      const void *labels, int labels_i64,
                                      const int64_t *in_len, const int64_t *tgt_len,
                                      int T, int B, int C, int S,
                                      int32_t *path, float *score, float *nll, float *frame_conf,
                                      int32_t *start, int32_t *end, float *conf,
                                      void *workspace, void *stream);
int ctc_amd_binary_token_spans_typed(const void *x, int x_dtype, int64_t stride_t, int64_t stride_b, const float *y,
                                     const int64_t *in_len, const int64_t *tgt_len,
                                     int T, int B, int C, int S,
                                     int32_t *path, float *score, float *nll, float *frame_conf,
                                     int32_t *start, int32_t *end, float *conf,
                                     void *workspace, void *stream);
int ctc_amd_noblank_posteriors_typed(const void *x, int x_dtype, int64_t stride_t, int64_t stride_b,
                                     const void *labels, int labels_i64,
                                     const int64_t *in_len, const int64_t *tgt_len,
                                     int T, int B, int C, int S,
                                     float *nll, float *gamma,
                                     void *workspace, void *stream);
int ctc_amd_binary_posteriors_typed(const void *x, int x_dtype, int64_t stride_t, int64_t stride_b, const float *y,
                                    const int64_t *in_len, const int64_t *tgt_len,
                                    int T, int B, int C, int S,
                                    float *nll, float *gamma,
                                    void *workspace, void *stream);

/* The producer step of the logits: one torch.nn.LSTMCell step of the reference's LSTM_cell.forward
 * (LSTM.py:39-51: `v_hsn, v_csn = self.v_cell(v, (v_hsn, v_csn)); v_series[time] = v_hsn`), fused with the write of
 * the hidden state into the logits tensor the losses read.
 *   x [B,I], h [B,H], c [B,H]: the cell's input and state (contiguous fp32);  w_ih [4H,I], w_hh [4H,H], b_ih, b_hh [4H]:
 *   nn.LSTMCell's parameters (gate order i, f, g, o);  h_out, c_out [B,H]: the new state (may alias h / c);
 *   gates_out [B,4H] or NULL: the gate activations (what a backward pass needs);
 *   series_row or NULL: row b of v_series[time] starts at series_row + b * series_stride_b; columns [0,H) get the new
 *   hidden state, columns [H, series_cols) get pad_value (a pitch of H + 1 with pad_value = -1e30 gives an odd class
 *   count the even, 8-byte aligned rows of the fastest loss kernel; the padded class has softmax 0: no loss or gradient
 *   value changes).  gates = x W_ih^T + b_ih + h W_hh^T + b_hh; c' = sigma(f) c + sigma(i) tanh(g); h' = sigma(o) tanh(c'). */
int ctc_amd_lstm_cell_step(const float *x, const float *h, const float *c,
                           const float *w_ih, const float *w_hh, const float *b_ih, const float *b_hh,
                           int B, int I, int H,
                           float *h_out, float *c_out, float *gates_out,
                           float *series_row, int64_t series_stride_b, int series_cols, float pad_value,
                           void *stream);

/* The whole loop of LSTM_cell.forward (LSTM.py:44-51) over the T frames as ONE launch, for the reference's class counts
 * (I + H <= 80, I <= 64, H <= 64; other sizes: CTC_AMD_ERR_UNSUPPORTED_SHAPE -- step frame by frame with the call above).
 *   x [T,B,I]: the cell inputs of all frames (contiguous fp32: `self.v(feat[time])` for every time);  h0, c0 [B,H];
 *   series: row (t, b) of v_series starts at series + t * series_stride_t + b * series_stride_b (columns as above);
 *   gates_out [T,B,4H], cells_out [T+1,B,H] (c_0 .. c_T) or NULL: what a backward pass needs;  h_out, c_out [B,H] or NULL:
 *   the state after the last frame.  Same arithmetic, in the same order, as T calls of ctc_amd_lstm_cell_step. */
int ctc_amd_lstm_series(const float *x, const float *h0, const float *c0,
                        const float *w_ih, const float *w_hh, const float *b_ih, const float *b_hh,
                        int T, int B, int I, int H,
                        float *series, int64_t series_stride_t, int64_t series_stride_b, int series_cols, float pad_value,
                        float *gates_out, float *cells_out, float *h_out, float *c_out, void *stream);

/* The backward RECURRENCE of ctc_amd_lstm_series as one launch (H <= 64): from the upstream gradient of v_series
 * (row (t, b) at d_series + t * ds_stride_t + b * ds_stride_b, unit stride over the classes, columns [0,H) read) and the
 * gates_out / cells_out of the forward launch to dpre_out [T,B,4H] -- the gradient of every frame's gate pre-activations --
 * and the gradients of the initial state dh0_out, dc0_out [B,H].  What is left of the backward pass has no recurrence in
 * it: dx = dpre W_ih, dW_ih = sum_tb dpre^T x, dW_hh = sum_tb dpre^T h_{t-1}, db = sum_tb dpre -- ctc_amd_lstm_backward
 * (below) runs this launch and those products behind it. */
int ctc_amd_lstm_series_backward(const float *d_series, int64_t ds_stride_t, int64_t ds_stride_b,
                                 const float *gates, const float *cells, const float *w_hh,
                                 int T, int B, int H, float *dpre_out, float *dh0_out, float *dc0_out, void *stream);

/* The HEAD of the producer (LSTM.py:8-18 `nn.Linear(inDim, outDim) -> nn.BatchNorm1d -> nn.ReLU -> nn.Dropout`,
 * called once per frame at LSTM.py:48) for all T frames as ONE launch: out[t] = dropout(relu(batchnorm(feat[t] W^T + b))).
 *   feat: row (t, b) of K floats at feat + t * feat_stride_t + b * feat_stride_b (16-byte aligned rows, K a multiple of 16);
 *   weight [C,K], bias [C]: the Linear layer;  bn_weight, bn_bias [C]: BatchNorm1d's affine parameters;
 *   running_mean / running_var [C]: eval mode (BatchNorm on its running statistics); both NULL: train mode -- the
 *   statistics of each FRAME's batch of B rows (biased variance, eps inside the square root), as the reference's per-frame
 *   calls compute them (B <= 256: one workgroup holds a frame's rows; B >= 2);
 *   mask [T,B,C] or NULL: the dropout mask, already scaled by 1 / (1 - p) (the caller draws it: the random stream stays
 *   the framework's);  out: row (t, b) of C floats at out + t * out_stride_t + b * out_stride_b;
 *   linear_out [T,B,C], save_mean / save_var / save_invstd [T,C] or NULL: what a backward pass and the update of the
 *   running statistics need (train mode; running = (1 - m) running + m stat, frame after frame, var unbiased: the caller).
 * The product is exact fp32 on the matrix cores (an fmaf chain per output; the order of the sum over k differs from a
 * BLAS GEMM's: results agree with torch's layers to ~1e-6 relative). */
int ctc_amd_head_forward(const float *feat, int64_t feat_stride_t, int64_t feat_stride_b,
                         const float *weight, const float *bias, const float *bn_weight, const float *bn_bias,
                         const float *running_mean, const float *running_var, float eps, const float *mask,
                         int T, int B, int K, int C,
                         float *out, int64_t out_stride_t, int64_t out_stride_b,
                         float *linear_out, float *save_mean, float *save_var, float *save_invstd, void *stream);

/* EVAL mode: ctc_amd_head_forward (running statistics, no mask) and ctc_amd_lstm_series as ONE launch -- feat in, v_series
 * out; the head's output [T,B,C] never goes to memory (a workgroup keeps the rows of its four samples in LDS).  The LSTM is
 * nn.LSTMCell(C, C).  Arguments as the two calls take them: feat / weight / bias / bn_weight / bn_bias / running_mean /
 * running_var / eps as ctc_amd_head_forward (the running statistics are REQUIRED: there is no train mode here -- BatchNorm's
 * batch statistics would tie the workgroups together);  h0, c0, w_ih, w_hh, b_ih, b_hh, series ..., pad_value, h_out, c_out
 * as ctc_amd_lstm_series with I = H = C.  No workspace, no host synchronisation: safe under stream capture.
 * v_series, h_out and c_out are bit-identical to the two calls (the same fmaf chains in the same order).
 * CTC_AMD_ERR_UNSUPPORTED_SHAPE: 2 C > 80, K not a multiple of 16, feat strides not multiples of 4, feat or weight not
 * 16-byte aligned, or 4 T C floats + the recurrence's staging beyond the LDS of a compute unit (use the two calls). */
int ctc_amd_lstm_forward(const float *feat, int64_t feat_stride_t, int64_t feat_stride_b,
                         const float *weight, const float *bias, const float *bn_weight, const float *bn_bias,
                         const float *running_mean, const float *running_var, float eps,
                         const float *h0, const float *c0,
                         const float *w_ih, const float *w_hh, const float *b_ih, const float *b_hh,
                         int T, int B, int K, int C,
                         float *series, int64_t series_stride_t, int64_t series_stride_b, int series_cols, float pad_value,
                         float *h_out, float *c_out, void *stream);

/* The BACKWARD of ctc_amd_head_forward on the same launch path: from d_out, the upstream gradient of the head's output (row
 * (t, b) of C floats at d_out + t * dout_stride_t + b * dout_stride_b), and what the forward call took and saved to the
 * gradients of feat (d_feat, rows of K floats at (dfeat_stride_t, dfeat_stride_b); NULL: not wanted), of the Linear layer
 * (d_weight [C,K], d_bias [C]) and of BatchNorm's affine parameters (d_bn_weight, d_bn_bias [C]).  All fp32.
 *   linear_out [T,B,C]: the forward's linear_out;  TRAIN mode: save_mean / save_invstd [T,C] as the forward saved them
 *   (running_mean, running_var NULL);  EVAL mode: running_mean / running_var [C] and eps (save_mean, save_invstd NULL);
 *   mask [T,B,C] or NULL as the forward took it.  With mean, inv the statistics the forward normalised with:
 *     xhat = (lin - mean) inv;   dy = d_out mask [y > 0], y being the forward's own BatchNorm output (same operations, same
 *     order: the gate agrees with the forward's ReLU bit for bit);   dbeta_t = sum_b dy, dgamma_t = sum_b dy xhat per frame;
 *     train: dlin = inv g (dy - dbeta_t / B - xhat dgamma_t / B) (BatchNorm over each frame's B rows);  eval: dlin = dy g inv;
 *     d_bn_bias = sum_t dbeta_t, d_bn_weight = sum_t dgamma_t, d_bias = sum_tb dlin, d_weight = sum_tb dlin^T feat,
 *     d_feat = dlin W.
 * The products are exact fp32 on the matrix cores (an fmaf chain per output element).  Deterministic: no atomics, every sum
 * in an order fixed by the shape (rows of a frame: lane quarters, then waves; frames ascending; d_weight: rows ascending
 * inside one of S = min(64, ceil(T B / 128)) row ranges, the ranges added ascending).  Two launches on `stream` (three when
 * S > 1), no allocation, no host synchronisation: safe under stream capture.  Every element of every output that is not NULL
 * is written; d_feat rows only in columns [0,K).  scratch: at least ctc_amd_head_backward_scratch_bytes(T, B, K, C) bytes of
 * device memory, any alignment, contents irrelevant (nothing is read from it that the same call has not written).
 * CTC_AMD_ERR_BAD_ARGUMENT (decided first): a NULL among the required pointers, a size < 1, statistics that are not exactly
 * one complete pair, train mode with B < 2, dout_stride_b < C, dfeat_stride_b < K, scratch_bytes below the query.
 * CTC_AMD_ERR_UNSUPPORTED_SHAPE: what ctc_amd_head_forward refuses (B > 256, K not a multiple of 16, feat strides not
 * multiples of 4, feat or weight not 16-byte aligned) and T B > 2^22 rows.  d_feat needs no alignment beyond a float's (it
 * is written with 4-byte stores).  The query answers 0 for sizes < 1 and for shapes the entry does not take. */
size_t ctc_amd_head_backward_scratch_bytes(int T, int B, int K, int C);
int ctc_amd_head_backward(const float *d_out, int64_t dout_stride_t, int64_t dout_stride_b,
                          const float *feat, int64_t feat_stride_t, int64_t feat_stride_b,
                          const float *weight, const float *bn_weight, const float *bn_bias,
                          const float *linear_out,
                          const float *save_mean, const float *save_invstd,
                          const float *running_mean, const float *running_var, float eps,
                          const float *mask,
                          int T, int B, int K, int C,
                          float *d_feat, int64_t dfeat_stride_t, int64_t dfeat_stride_b,
                          float *d_weight, float *d_bias, float *d_bn_weight, float *d_bn_bias,
                          void *scratch, size_t scratch_bytes, void *stream);

/* The BACKWARD of ctc_amd_lstm_series, whole: from d_series, the upstream gradient of v_series (as ctc_amd_lstm_series_backward
 * takes it), and what the forward call took and saved to the gradients of the cell inputs, the initial state and nn.LSTMCell's
 * four parameters.  All fp32.
 *   gates [T,B,4H], cells [T+1,B,H]: gates_out / cells_out of the forward call;  x: the cell inputs, row (t, b) of I floats at
 *   x + t * x_stride_t + b * x_stride_b;  h0 [B,H];  series: the forward's v_series, row (t, b) at series + t * series_stride_t
 *   + b * series_stride_b -- columns [0,H) of row (t - 1, b) are h_{t-1}, read in place (h_{-1} = h0: no concatenated copy);
 *   w_ih [4H,I], w_hh [4H,H].  With dpre [T,B,4H] the pre-activation gradients of ctc_amd_lstm_series_backward:
 *     d_x[t,b,:] = dpre[t,b,:] W_ih (rows of I floats at (dx_stride_t, dx_stride_b); NULL: not wanted),
 *     d_w_ih [4H,I] = sum_tb dpre[t,b,:]^T x[t,b,:],   d_w_hh [4H,H] = sum_tb dpre[t,b,:]^T h_{t-1}[b,:],
 *     d_b_ih = d_b_hh [4H] = sum_tb dpre[t,b,:] (two arrays, the same values),   dh0, dc0 [B,H] as that call writes them.
 * Launches, all on `stream`: lstm_series_bwd_kernel (the launch of ctc_amd_lstm_series_backward, the same bits: dpre goes to the
 * scratch, dh0 and dc0 to the caller); one products launch -- d^T x against x and against h_{t-1}, d W, the column sums -- exact
 * fp32 on the matrix cores (v_mfma_f32_16x16x4_f32, one fmaf chain per output element); and, when the row range splits, one
 * reduce launch.  Row-range splits (the head's rule): with R = T B, the weight and bias gradients sum their rows in ranges of
 * chunk = 16 ceil(ceil(R / min(64, ceil(R / 128))) / 16) rows, S = ceil(R / chunk) of them (R <= 128: one; 140: two of 80;
 * 9600: 60 of 160), rows ascending inside a range, the ranges added ascending -- a function of T B alone, no atomics: the same
 * inputs give the same bits.  No allocation, no host synchronisation:
 * safe under stream capture.  Every element of every output that is not NULL is written; d_x rows only in columns [0,I).
 * scratch: at least ctc_amd_lstm_backward_scratch_bytes(T, B, I, H) bytes of device memory, any alignment, contents irrelevant
 * (nothing is read from it that the same call has not written).
 * CTC_AMD_ERR_BAD_ARGUMENT (decided first, before any HIP call): a NULL among the required pointers (all but d_x), a size < 1,
 * ds_stride_b < H, series_stride_b < H, x_stride_b < I, dx_stride_b < I (with d_x), scratch_bytes below the query.
 * CTC_AMD_ERR_UNSUPPORTED_SHAPE: what ctc_amd_lstm_series refuses (I + H > 80, I > 64, H > 64) and T B > 2^22 rows.
 * The query answers 0 for sizes < 1 and for shapes the entry does not take. */
size_t ctc_amd_lstm_backward_scratch_bytes(int T, int B, int I, int H);
int ctc_amd_lstm_backward(const float *d_series, int64_t ds_stride_t, int64_t ds_stride_b,
                          const float *gates, const float *cells,
                          const float *x, int64_t x_stride_t, int64_t x_stride_b,
                          const float *h0,
                          const float *series, int64_t series_stride_t, int64_t series_stride_b,
                          const float *w_ih, const float *w_hh,
                          int T, int B, int I, int H,
                          float *d_x, int64_t dx_stride_t, int64_t dx_stride_b,
                          float *dh0, float *dc0,
                          float *d_w_ih, float *d_w_hh, float *d_b_ih, float *d_b_hh,
                          void *scratch, size_t scratch_bytes, void *stream);

/* ctc_amd_lstm_series beyond the reference's class counts: every 1 <= I <= 160 and 1 <= H <= 160 (the benchmark's C = 158;
 * the narrow shapes too).  Arguments and outputs are those of ctc_amd_lstm_series -- series at any pitch, pad columns
 * [H, series_cols) filled with pad_value, gates_out [T,B,4H], cells_out [T+1,B,H] (cells[0] = c0), h_out, c_out, each of the
 * last four or NULL -- and the arithmetic is, bit for bit, that of T calls of ctc_amd_lstm_cell_step: per (sample, gate row)
 * one fp32 fmaf chain from 0 over k ascending through the W_ih part, then through the W_hh part, then + (b_ih[r] + b_hh[r]).
 * The weights (800 KB at 158) fit neither the LDS nor a workgroup's registers: they stay in L2 and are streamed every frame,
 * from a transposed copy [I + H][4H] so that the reads are coalesced.  Launches, all on `stream`: the transposed copy into the
 * scratch; the x part of every (t, b) row's pre-activations into the scratch (no recurrence in it: all T B rows at once, the
 * chain from 0 through the W_ih part); the recurrence, one workgroup per four samples for all T frames, which starts every
 * W_hh chain from the stored x part (an fp32 store and load is exact).  No allocation, no host synchronisation: safe under
 * stream capture.
 * scratch: at least ctc_amd_lstm_series_wide_scratch_bytes(T, B, I, H) bytes of device memory, any alignment, contents
 * irrelevant.  The query answers 0 for sizes < 1 and for shapes the entry does not take.
 * CTC_AMD_ERR_BAD_ARGUMENT (decided first, before any HIP call): a NULL among x, h0, c0, the four parameters, series and
 * scratch; a size < 1; series_cols < H; series_stride_b < series_cols; scratch_bytes below the query.
 * CTC_AMD_ERR_UNSUPPORTED_SHAPE: I > 160, H > 160, or T B > 2^22 rows. */
size_t ctc_amd_lstm_series_wide_scratch_bytes(int T, int B, int I, int H);
int ctc_amd_lstm_series_wide(const float *x, const float *h0, const float *c0,
                             const float *w_ih, const float *w_hh, const float *b_ih, const float *b_hh,
                             int T, int B, int I, int H,
                             float *series, int64_t series_stride_t, int64_t series_stride_b, int series_cols, float pad_value,
                             float *gates_out, float *cells_out, float *h_out, float *c_out,
                             void *scratch, size_t scratch_bytes, void *stream);

/* ctc_amd_lstm_series_backward for every 1 <= H <= 160 (H > 160: CTC_AMD_ERR_UNSUPPORTED_SHAPE): the same arguments, the same
 * formulas, one launch, no scratch.  W_hh is streamed from L2 as it lies (row-major, lanes over the columns); the sum over the
 * 4H gate rows runs as four chains of H rows, one per gate chunk, added in ascending chunk order -- no atomics, a fixed order:
 * two calls give the same bits.  No bitwise tie to ctc_amd_lstm_series_backward, whose sum is one chain. */
int ctc_amd_lstm_series_backward_wide(const float *d_series, int64_t ds_stride_t, int64_t ds_stride_b,
                                      const float *gates, const float *cells, const float *w_hh,
                                      int T, int B, int H, float *dpre_out, float *dh0_out, float *dc0_out, void *stream);

/* The bias gradients behind ctc_amd_lstm_series_backward_wide: d_b_ih[c] = d_b_hh[c] = sum_r dpre[r][c] over the `rows` = T B rows
 * of dpre [rows][4H] (two arrays, the same values), H <= 160.  One launch: lanes over the columns, sixteen waves over the rows,
 * the partial sums added in a fixed order -- no atomics, no scratch, nothing that has to be cleared first; two calls give the
 * same bits.  No allocation, no host synchronisation: safe under stream capture.  CTC_AMD_ERR_BAD_ARGUMENT: a NULL pointer,
 * rows < 1, H < 1;  CTC_AMD_ERR_UNSUPPORTED_SHAPE: H > 160. */
int ctc_amd_lstm_bias_grad_wide(const float *dpre, int64_t rows, int H, float *d_b_ih, float *d_b_hh, void *stream);

/* ctc_amd_head_forward for batches beyond one workgroup's 256 rows: every 1 <= B <= 65536 (the B <= 256 it already takes too).
 * Arguments, outputs and formulas are ctc_amd_head_forward's, followed by the scratch.  Every Linear output is the same fmaf chain
 * as the narrow entry's (bit for bit, and so is all of eval mode: no value there depends on another row).  Train mode: the
 * statistics of each frame's B rows in two passes -- the mean, then the centred second moment; biased variance, eps inside the
 * root -- with the sums over a frame's rows crossing workgroups at a kernel boundary:
 *   eval   ONE launch: grid (frame, block of 256 rows, group of <= 3 column tiles); a wave takes 16 rows and every column tile
 *          of its group, so feat is read ceil(ceil(C / 16) / 3) times, not ceil(C / 16) times;
 *   train  TWO launches: the same grid writes the Linear output (to linear_out, or to the scratch when that is NULL) and the
 *          column sums of its 256 rows (lane quarters, then waves) to the scratch; then one workgroup per (frame, column tile)
 *          adds those sums in ascending block order (mean), walks the Linear output for the centred moment (per lane: row blocks
 *          ascending, then its four rows; then lane quarters, then waves), and applies BatchNorm, ReLU and the mask.
 * No atomics, every order fixed by the shape: two calls give the same bits.  No allocation, no host synchronisation: safe under
 * stream capture.  Every element of every output that is not NULL is written (save_* in train mode only, as the narrow entry).
 * scratch: at least ctc_amd_head_forward_wide_scratch_bytes(T, B, K, C) bytes of device memory, any alignment, contents
 * irrelevant.  CTC_AMD_ERR_BAD_ARGUMENT (decided first, before any HIP call): a NULL among feat, the four parameters, out and
 * scratch; a size < 1; one running statistic without the other; out_stride_b < C; train mode with B < 2; scratch_bytes below
 * the query.  CTC_AMD_ERR_UNSUPPORTED_SHAPE: K not a multiple of 16, feat strides not multiples of 4, feat or weight not
 * 16-byte aligned, T B > 2^22 rows, B > 65536.  The query answers 0 for sizes < 1 and for shapes the entry does not take. */
size_t ctc_amd_head_forward_wide_scratch_bytes(int T, int B, int K, int C);
int ctc_amd_head_forward_wide(const float *feat, int64_t feat_stride_t, int64_t feat_stride_b,
                              const float *weight, const float *bias, const float *bn_weight, const float *bn_bias,
                              const float *running_mean, const float *running_var, float eps, const float *mask,
                              int T, int B, int K, int C,
                              float *out, int64_t out_stride_t, int64_t out_stride_b,
                              float *linear_out, float *save_mean, float *save_var, float *save_invstd,
                              void *scratch, size_t scratch_bytes, void *stream);

/* ctc_amd_head_backward for every 1 <= B <= 65536: the same arguments, the same formulas, the same errors (with the batch bound
 * at 65536) and the same scratch layout.  Only the row pass differs: one workgroup per (frame, column tile) walks the frame's
 * blocks of 256 rows -- dbeta_t and dgamma_t per lane over the row blocks ascending, then lane quarters, then waves; in train
 * mode a second walk writes dlin and sums it (eval mode has no cross-row term and writes dlin in the first walk).  The products
 * launch and the reduce launch are ctc_amd_head_backward's own.  Two launches on `stream`, three when T B > 128; no atomics, no
 * allocation, no host synchronisation: safe under stream capture, and two calls give the same bits. */
size_t ctc_amd_head_backward_wide_scratch_bytes(int T, int B, int K, int C);
int ctc_amd_head_backward_wide(const float *d_out, int64_t dout_stride_t, int64_t dout_stride_b,
                               const float *feat, int64_t feat_stride_t, int64_t feat_stride_b,
                               const float *weight, const float *bn_weight, const float *bn_bias,
                               const float *linear_out,
                               const float *save_mean, const float *save_invstd,
                               const float *running_mean, const float *running_var, float eps,
                               const float *mask,
                               int T, int B, int K, int C,
                               float *d_feat, int64_t dfeat_stride_t, int64_t dfeat_stride_b,
                               float *d_weight, float *d_bias, float *d_bn_weight, float *d_bn_bias,
                               void *scratch, size_t scratch_bytes, void *stream);

/* The five head entries on a feature operand of element type `feat_dtype` (CTC_AMD_F32 / _BF16 / _F16, as
 * ctc_amd_noblank_loss_grad_typed takes x): a backbone under autocast hands feat over in bf16 or fp16, and the launches read it
 * as it lies instead of an fp32 copy.  Each entry is its untyped sibling with these changes only: feat is `const void *feat,
 * int feat_dtype`; on the backward entries d_feat is `void *d_feat`, of feat's element type; the strides of both are in elements.
 * CTC_AMD_F32 is exactly the untyped entry.  CTC_AMD_BF16 / CTC_AMD_F16: a lane's four features of a k-block are ONE 8-byte load,
 * widened to fp32 in registers -- bf16 by a 16-bit shift, fp16 by the exact conversion (subnormals are not flushed) -- and fed to
 * the fp32 launch's own v_mfma_f32_16x16x4_f32 chain in the fp32 launch's order (k is not re-tiled): every output of the forward
 * entries and d_weight, d_bias, d_bn_weight, d_bn_bias are bit for bit what the untyped entry gives on the features converted to
 * fp32, and d_feat is the untyped entry's fp32 value rounded once to nearest even.  Weights, bias, BatchNorm's parameters and
 * statistics, the mask, linear_out and every other output stay fp32.  The scratch queries do not depend on the element type: the
 * untyped entries' queries serve.  Same launches, same determinism, same safety under stream capture as the siblings.
 * Errors: the sibling's, decided in the sibling's order before any HIP call, with these differences.
 * CTC_AMD_ERR_BAD_ARGUMENT: also a feat_dtype that is none of the three.  CTC_AMD_ERR_UNSUPPORTED_SHAPE for the 2-byte types:
 * the 16-byte rule on feat becomes an 8-byte rule -- feat not 8-byte aligned, a feat stride that is not a multiple of 4 elements,
 * K not a multiple of 16 (the weight keeps its 16-byte rule) -- and a d_feat that is not 2-byte aligned (it is written with
 * 2-byte stores; dfeat_stride_b < K stays CTC_AMD_ERR_BAD_ARGUMENT). */
/* ctc_amd_head_forward on a typed feat */
int ctc_amd_head_forward_typed(const void *feat, int feat_dtype, int64_t feat_stride_t, int64_t feat_stride_b,
                               const float *weight, const float *bias, const float *bn_weight, const float *bn_bias,
                               const float *running_mean, const float *running_var, float eps, const float *mask,
                               int T, int B, int K, int C,
                               float *out, int64_t out_stride_t, int64_t out_stride_b,
                               float *linear_out, float *save_mean, float *save_var, float *save_invstd, void *stream);

/* ctc_amd_head_forward_wide on a typed feat (only the product launch reads feat; scratch: ctc_amd_head_forward_wide_scratch_bytes) */
int ctc_amd_head_forward_wide_typed(const void *feat, int feat_dtype, int64_t feat_stride_t, int64_t feat_stride_b,
                                    const float *weight, const float *bias, const float *bn_weight, const float *bn_bias,
                                    const float *running_mean, const float *running_var, float eps, const float *mask,
                                    int T, int B, int K, int C,
                                    float *out, int64_t out_stride_t, int64_t out_stride_b,
                                    float *linear_out, float *save_mean, float *save_var, float *save_invstd,
                                    void *scratch, size_t scratch_bytes, void *stream);

/* ctc_amd_lstm_forward on a typed feat (v_series, h_out and c_out stay fp32) */
int ctc_amd_lstm_forward_typed(const void *feat, int feat_dtype, int64_t feat_stride_t, int64_t feat_stride_b,
                               const float *weight, const float *bias, const float *bn_weight, const float *bn_bias,
                               const float *running_mean, const float *running_var, float eps,
                               const float *h0, const float *c0,
                               const float *w_ih, const float *w_hh, const float *b_ih, const float *b_hh,
                               int T, int B, int K, int C,
                               float *series, int64_t series_stride_t, int64_t series_stride_b, int series_cols, float pad_value,
                               float *h_out, float *c_out, void *stream);

/* ctc_amd_head_backward on a typed feat; d_feat has feat's element type (scratch: ctc_amd_head_backward_scratch_bytes).  Only the
 * products launch sees feat and d_feat: the row pass and the reduce launch are the untyped entry's. */
int ctc_amd_head_backward_typed(const float *d_out, int64_t dout_stride_t, int64_t dout_stride_b,
                                const void *feat, int feat_dtype, int64_t feat_stride_t, int64_t feat_stride_b,
                                const float *weight, const float *bn_weight, const float *bn_bias,
                                const float *linear_out,
                                const float *save_mean, const float *save_invstd,
                                const float *running_mean, const float *running_var, float eps,
                                const float *mask,
                                int T, int B, int K, int C,
                                void *d_feat, int64_t dfeat_stride_t, int64_t dfeat_stride_b,
                                float *d_weight, float *d_bias, float *d_bn_weight, float *d_bn_bias,
                                void *scratch, size_t scratch_bytes, void *stream);

/* ctc_amd_head_backward_wide on a typed feat; d_feat has feat's element type (scratch: ctc_amd_head_backward_wide_scratch_bytes) */
int ctc_amd_head_backward_wide_typed(const float *d_out, int64_t dout_stride_t, int64_t dout_stride_b,
                                     const void *feat, int feat_dtype, int64_t feat_stride_t, int64_t feat_stride_b,
                                     const float *weight, const float *bn_weight, const float *bn_bias,
                                     const float *linear_out,
                                     const float *save_mean, const float *save_invstd,
                                     const float *running_mean, const float *running_var, float eps,
                                     const float *mask,
                                     int T, int B, int K, int C,
                                     void *d_feat, int64_t dfeat_stride_t, int64_t dfeat_stride_b,
                                     float *d_weight, float *d_bias, float *d_bn_weight, float *d_bn_bias,
                                     void *scratch, size_t scratch_bytes, void *stream);

/* Evaluation: from per-frame decisions to a token sequence, and from a token sequence to its distance
 * from the reference transcript.  Target-free: no logits, no lattice, no workspace.  Both entries are integer-exact, use
 * no atomics and no waiting between workgroups (deterministic), allocate nothing and never synchronise the host.
 * int64 labels are read through their low 32 bits, as everywhere in this library (class indices and -1 fit).
 *
 * ctc_amd_collapse_frames: merge maximal runs of equal labels, drop the blank runs.
 *   frames     label of frame t of sample b at frames[b * stride_b + t * stride_t] (strides in elements; int32, or int64
 *              with frames_i64 = 1): a [B,T] tensor, a [T,B] one (argmax of [T,B,C]) or a slice of a wider batch alike --
 *              a best path (ctc_amd_blank_best_path: collapse the path's classes; ctc_amd_noblank_best_path /
 *              ctc_amd_binary_best_path: the label positions themselves, blank < 0) or logits.argmax(-1)
 *   in_len     [B] int64, 0 <= T_b <= T (clamped to that range); frames t >= T_b are never read
 *   blank      >= 0: runs of this label separate tokens and are dropped (a, blank, a -> two tokens; a, a -> one);
 *              < 0: there is no blank -- every run is a token, a run of -1 (a failed best path) included
 *   frame_conf per-frame confidence at frame_conf[b * conf_stride_b + t * conf_stride_t], or NULL; NULL exactly when conf is
 *   tokens     [B,W] int32 out: the label of the run (its low 32 bits)
 *   out_len    [B] int64 out: the number of tokens -- the true count even when it exceeds W (the first W are stored)
 *   start, end [B,W] int32 out: first and last frame of the run, both INCLUSIVE
 *   conf       [B,W] fp32 out or NULL: the sum of frame_conf over start .. end -- from 0.0f, in ascending t, in fp32 --
 *              followed by one correctly rounded fp32 division by float(end - start + 1).  The order is part of the
 *              contract: a float32 loop in that order reproduces the bits.
 * Columns at and beyond out_len[b] hold -1 / -1 / -1 / 0: every element of every output is written.
 * NULL pointers (conf and frame_conf apart: both or neither), T, B or W < 1: CTC_AMD_ERR_BAD_ARGUMENT before any HIP
 * call.  One workgroup per sample keeps the sample's labels and the spans of its first min(W, T) tokens in LDS:
 * 4 (T + 2 min(W, T) + 1) bytes <= 160 KB -- every T <= 13653 with any W (T <= 40957 at W = 1);
 * CTC_AMD_ERR_UNSUPPORTED_SHAPE beyond. */
int ctc_amd_collapse_frames(const void *frames, int frames_i64,
                            int64_t stride_b, int64_t stride_t,
                            const int64_t *in_len,
                            const float *frame_conf, int64_t conf_stride_b, int64_t conf_stride_t,
                            int T, int B, int blank, int W,
                            int32_t *tokens, int64_t *out_len,
                            int32_t *start, int32_t *end, float *conf,
                            void *stream);

/* ctc_amd_edit_distance: dist[b] = the Levenshtein distance (insertions, deletions, substitutions, unit costs) between
 * hyp[b, :hyp_len[b]] and ref[b, :ref_len[b]] -- the numerator of the label error rate.
 *   hyp  [B,N], ref [B,M]: row b at hyp + b * hyp_stride_b / ref + b * ref_stride_b (strides in elements), unit stride
 *        inside a row; int32, or int64 with hyp_i64 / ref_i64 = 1 (the two may differ).  A pointer may be NULL only
 *        where its width is 0.
 *   hyp_len, ref_len [B] int64, 0 <= . <= N / M (clamped to that range); elements beyond a length are never read
 *   dist [B] int32 out
 * NULL pointers, B < 1, N < 0 or M < 0: CTC_AMD_ERR_BAD_ARGUMENT; M > 1023, the library's one limit on target widths:
 * CTC_AMD_ERR_UNSUPPORTED_SHAPE; both before any HIP call.  Any N >= 0 (a hypothesis may be as long as T).
 * One wave per sample holds the row of the recurrence over the reference in registers (1, 2, 4, 8 or 16 cells per lane
 * for M <= 64, 128, 256, 512, 1023) and steps through the hypothesis. */
int ctc_amd_edit_distance(const void *hyp, int hyp_i64, int64_t hyp_stride_b, const int64_t *hyp_len,
                          const void *ref, int ref_i64, int64_t ref_stride_b, const int64_t *ref_len,
                          int B, int N, int M, int32_t *dist, void *stream);

/* Decoding without a transcript: CTC prefix beam search, the most probable LABEL SEQUENCES of each sample
 * -- a sequence's probability is the sum over all of its alignments, which argmax + ctc_amd_collapse_frames (the best
 * single alignment) does not give.  One launch, one workgroup per sample; no atomics, no waiting between workgroups
 * (deterministic: the same inputs give the same bits), no allocation and no host synchronisation.
 *
 * ctc_amd_beam_search_scratch_bytes: the bytes `scratch` must hold -- 8 B (T W + 1), the trie of prefixes; 0 when T, B or
 *   W is out of range.  The caller allocates; the contents before and after a call mean nothing.
 * ctc_amd_beam_search:
 *   x          [T,B,C] fp32 at x[t * stride_t + b * stride_b + c] (strides in elements, unit class stride).  blank >= 0:
 *              normalised log-probabilities, the contract of ctc_amd_blank_loss_grad.  blank < 0: the no-blank lattice,
 *              x holds raw logits and the kernel subtracts each row's log-sum-exp in fp32.
 *   in_len     [B] int64, 0 <= T_b <= T (clamped to that range); frames t >= T_b are never read
 *   W, K, N, L beam width (1 .. 64); classes a prefix is extended by per frame (1 .. 32, clamped to the number of
 *              non-blank classes); hypotheses written per sample (1 .. W); token columns per hypothesis (>= 1)
 *   tokens     [B,N,L] int32 out; lengths [B,N] int64 out: the true token count, also beyond L (the first L are stored,
 *              the rest of the row holds -1); scores [B,N] fp32 out: natural-log probability of the label sequence as the
 *              search summed it (a lower bound of the exact value: alignments through pruned prefixes are missing);
 *              count [B] int32 out: the hypotheses that exist, <= N.  Hypotheses are sorted best first; rows at and
 *              beyond count[b] hold -1 / 0 / -inf: every element of every output is written.  T_b = 0: the one empty
 *              hypothesis, score 0.
 * The search, per frame of row lp (x, or x - logsumexp(x)): the class candidates are the K non-blank classes of the largest
 * x[t,b,c] (ties to the lower class, -inf left out).  Beam i (pb, pnb: log probability of its prefix ending in blank / in
 * a label; tot = logaddexp(pb, pnb)) stays with pb' = tot + lp[blank], pnb' = pnb + lp[last] and is extended by candidate
 * c with v = lp[c] + (c == last ? pb : tot); an extension that is the prefix of a beam j (j's parent prefix is beam i's,
 * j's last token is c) is added into j's pnb', every other one is a candidate with pb' = -inf, pnb' = v.  The W best
 * candidates of score logaddexp(pb', pnb') > -inf are kept under the total order: score descending, stay before
 * extension, beam slot ascending, class rank ascending.  The no-blank lattice has no pb: lp[blank] counts as -inf.
 * NaN inputs: the result is unspecified, the launch ends.
 * A NULL pointer, T or B < 1, C < 2, blank >= C, W, K, N or L out of range (N <= W), scratch_bytes below
 * ctc_amd_beam_search_scratch_bytes(T, B, W): CTC_AMD_ERR_BAD_ARGUMENT before any HIP call.  Any C: the row is streamed. */
size_t ctc_amd_beam_search_scratch_bytes(int T, int B, int W);
int ctc_amd_beam_search(const float *x, int64_t stride_t, int64_t stride_b, const int64_t *in_len,
                        int T, int B, int C, int blank /* < 0: the no-blank lattice, x raw logits */,
                        int W, int K, int N, int L,
                        int32_t *tokens, int64_t *lengths, float *scores, int32_t *count,
                        void *scratch, size_t scratch_bytes, void *stream);

/* The same search under a prior over label sequences: shallow fusion with a bigram language model and a
 * token insertion bonus, or a transition grammar -- one dense table covers both.
 *   lm           [C+1, C] fp32 at lm[p * lm_stride + c] (lm_stride >= C in elements, unit column stride), shared by the
 *                batch.  lm[p, c], p < C: the log-score of token c behind token p; row C scores a sequence's first token.
 *                A finite entry is a score; -inf FORBIDS the transition, whatever lm_weight is.
 *   lm_weight    alpha, finite and >= 0;  token_bonus  beta, finite
 *   scores       [B,N] fp32 out: the fused score logaddexp(pb, pnb) + g; hypotheses are sorted by it, best first
 *   ctc_scores   [B,N] fp32 out: logaddexp(pb, pnb) alone, the acoustic log-probability as the search summed it (what
 *                `scores` of ctc_amd_beam_search means); -inf in rows at and beyond count[b]
 *   every other argument: as for ctc_amd_beam_search, the same limits, the same scratch.
 * The rules are those above with three differences.  Every prefix carries g beside (pb, pnb): g(empty) = 0,
 * g(prefix + c) = g(prefix) + inc, inc = alpha lm[last or C, c] + beta; where lm[last or C, c] is -inf the extension is no
 * candidate.  (1) The selection key of a stay candidate is logaddexp(pb', pnb') + g(beam), that of an extension candidate
 * v + (g(beam) + inc); the tie order is unchanged and keys of -inf are dropped.  (2) An extension that is the prefix of a
 * beam j still adds its acoustic v into j's pnb'; g(j) is untouched (g depends on the prefix alone and was formed from the
 * same numbers when j was created; a forbidden bigram is never a beam).  (3) The outputs, as listed.  Unchanged: the K class
 * candidates of a frame are chosen on x alone; the blank's column of lm is never read, nor the diagonal on the no-blank
 * lattice (a label has no equal neighbour there); T_b = 0 gives the empty hypothesis with both scores 0.
 * NaN or +inf in lm: the result is unspecified, but nothing outside the table is read -- the row is a beam's own last token
 * or C, the column one of the kernel's own class candidates.
 * Whatever ctc_amd_beam_search refuses, a NULL lm or ctc_scores, lm_stride < C, lm_weight negative or not finite,
 * token_bonus not finite: CTC_AMD_ERR_BAD_ARGUMENT before any HIP call. */
int ctc_amd_beam_search_lm(const float *x, int64_t stride_t, int64_t stride_b, const int64_t *in_len,
                           int T, int B, int C, int blank, int W, int K, int N, int L,
                           const float *lm, int64_t lm_stride, float lm_weight, float token_bonus,
                           int32_t *tokens, int64_t *lengths, float *scores, float *ctc_scores, int32_t *count,
                           void *scratch, size_t scratch_bytes, void *stream);

/* Scores of given label sequences: scores[b, n] = the natural-log probability of candidate n for sample b,
 * summed over ALL of its alignments of the first T_b frames -- the exact value `scores` of ctc_amd_beam_search is a lower
 * bound of; N-best rescoring, transcript retrieval, scoring hypotheses made elsewhere.  One launch for all N candidates
 * of all samples: a sample's rows are brought on chip once per group of 8 candidates and every candidate's forward chain
 * is fed from them.  (The gradient: ctc_amd_sequence_scores_grad below.)  No scratch, no atomics, no waiting between workgroups (deterministic: the same inputs
 * give the same bits), no allocation and no host synchronisation.
 *   x          [T,B,C] fp32 at x[t * stride_t + b * stride_b + c] (strides in elements, unit class stride).  blank >= 0:
 *              normalised log-probabilities, the contract of ctc_amd_blank_loss_grad; the lattice is torch.nn.CTCLoss's
 *              (blanks optional, mandatory between equal neighbours) and the score is -nll of ctc_amd_blank_loss_grad on
 *              that sequence as the target, where that is finite.  blank < 0: the no-blank lattice, x holds raw logits and
 *              the kernel subtracts each row's log-sum-exp in fp32; transitions are stay / advance from state 0 at frame 0
 *              to state len - 1 at frame T_b - 1 (the lattice of ctc_amd_noblank_loss_grad): for a sequence without equal
 *              neighbours the probability that the frames collapse to it, with equal neighbours what that lattice gives
 *              (the two labels are two states; it is not a collapse probability).
 *   in_len     [B] int64, 0 <= T_b <= T (clamped to that range); frames t >= T_b are never read
 *   seq        the labels of candidate n of sample b at seq[b * seq_stride_b + n * seq_stride_n + i], i < L; int32, or
 *              int64 when seq_i64 != 0; strides in elements.  seq_stride_b = 0: one set of candidates shared by the batch
 *              (the same bits as the set repeated per sample).  Elements at and behind a candidate's length are never
 *              read (-1 padding is fine).
 *   seq_len    the lengths at seq_len[b * len_stride_b + n], int64 (len_stride_b = 0: shared)
 *   count      [B] int32 or NULL: the candidates of sample b that exist (the `count` of ctc_amd_beam_search)
 *   scores     [B,N] fp32 out; every element is written
 * Decided inside the launch, in this order:
 *   n >= count[b]                                   -inf  (rows of a beam search's output that do not exist stay -inf)
 *   len < 0 or len > L                              NaN   ("not scored": e.g. a hypothesis the beam search truncated)
 *   a label among the first len outside [0, C), or equal to blank             NaN
 *   T_b = 0                                         0 for len = 0, else -inf
 *   no alignment                                    -inf, never NaN and never the losses' 1e13 sentinel: too few frames
 *                                                   (T_b < len; blank lattice: T_b < len + repeats), or every
 *                                                   alignment crosses a -inf input (-inf inputs are allowed: a masked
 *                                                   vocabulary)
 *   len = 0                                         blank lattice: the all-blank path, the sum over t < T_b of
 *                                                   x[t, blank]; no-blank lattice: -inf for T_b >= 1
 * NaN inputs, and a no-blank row that is -inf throughout: the value is unspecified, the launch ends.
 * Arithmetic: log2-domain fp32 chains, renormalised every 8 frames against an exactly kept offset (the largest of the
 * candidate's own states goes to [0, 1); register states beyond its lattice are held at -inf), so a step rounds at the size
 * of a state's distance from the best one, not of the score: within 1e-5 max(1, |score|) of float64 at T = 2000, for scores
 * of magnitude 10 as for 10^4.
 * A NULL x, in_len, seq, seq_len or scores, T, B, C, N or L < 1, blank >= C: CTC_AMD_ERR_BAD_ARGUMENT; L > 255 (511
 * blank-lattice states, 8 per lane of one wave), or more than 2^31 - 1 workgroups (B ceil(N / 8)):
 * CTC_AMD_ERR_UNSUPPORTED_SHAPE; both before any HIP call.  Any T, any N, any C (C > 4096: the rows are not staged on chip,
 * every chain gathers from memory -- correct and slow). */
int ctc_amd_sequence_scores(const float *x, int64_t stride_t, int64_t stride_b, const int64_t *in_len,
                            int T, int B, int C, int blank /* < 0: the no-blank lattice, x raw logits */,
                            const void *seq, int seq_i64, int64_t seq_stride_b, int64_t seq_stride_n, int L,
                            const int64_t *seq_len, int64_t len_stride_b, const int32_t *count /* or NULL */,
                            int N, float *scores, void *stream);

/* Gradient of those scores, for N-best discriminative training (minimum word error rate, MMI against
 * competitors, contrastive training among transcripts): the weighted sum over a sample's candidates
 *     grad[t, b, c] = sum over n "scored finite" of  w[b, n] * d scores[b, n] / d x[t, b, c],
 * "scored finite": n < count[b] and scores[b, n] (as ctc_amd_sequence_scores gives it) finite.  All arguments up to N mean
 * what they mean there; then
 *   w          [B,N] fp32 at w[b * w_stride_b + n]: the weight of every score (d loss / d scores[b, n])
 *   grad       [T,B,C] fp32 out at grad[t * grad_stride_t + b * grad_stride_b + c], strides of its own (in elements, unit
 *              class stride); EVERY element is written
 *   scores     [B,N] fp32 out or NULL: the scores, bit for bit those of ctc_amd_sequence_scores on the same inputs
 *   scratch    ctc_amd_sequence_scores_grad_scratch_bytes(T, B, C, N, L, blank) bytes of device memory, 8-byte aligned; the
 *              caller allocates, the contents before and after a call mean nothing
 * The derivative, x taken as FREE inputs:
 *   blank >= 0   d score / d x[t, c] = sum over the states s of the candidate's lattice that carry class c of gamma_t(s),
 *                the class occupancy of the candidate's own lattice, t < T_b.  x holds log-probabilities and the kernel
 *                does not know where they came from: this is the true partial derivative, NOT torch.nn.CTCLoss's
 *                exp(x) - occupancy form, which has the log_softmax in front of the loss folded in.  Behind a log_softmax
 *                the two agree (its backward subtracts softmax times the row sum, which is 1 per candidate).
 *   blank < 0    x holds raw logits, the row's log-sum-exp is taken inside: d score / d x[t, c] = occupancy_t(c) -
 *                softmax(x_t)[c], t < T_b; so grad = sum_n w_n occupancy_n - (sum over n scored finite of w_n) softmax(x_t),
 *                the softmax taken once per row for all candidates.
 *   Rows t >= T_b, and every row of a sample with T_b = 0, are exactly 0.  Where x is -inf the gradient is 0 (occupancy and
 *   softmax are both 0 there), never NaN, for finite weights.
 *   A candidate that is not scored finite -- n >= count[b], a NaN score (bad length, bad label), a -inf score (no
 *   alignment) -- contributes exactly nothing whatever w[b, n] holds, NaN and inf included: it is skipped by its score, not
 *   multiplied by 0.  The w of a candidate that IS scored finite must be finite.
 * Scratch bytes: B N (8 T (S_L + 1) + 4 (L + 2)) rounded up to a multiple of 256, S_L = 2 L + 1 for blank >= 0 and L for
 *   blank < 0 -- per candidate and frame the S_L forward states and their S_L emissions (fp32) and one offset (double);
 *   per candidate L + 1 label ranks and the score.  0 when an argument is out of range (T, B, C, N or L < 1, L > 255,
 *   C > 4096, blank >= C).  About 1.5 GB at T = 2000, B = 64, N = 4, L = 180 on the blank lattice.
 * Deterministic: no atomics and no arrival order anywhere.  The candidates of a sample are added in the order n = 0, 1, ..;
 *   inside a candidate the blank states are summed by one fixed tree and the k-th occurrences of the classes are added in
 *   the order k = 0, 1, ..  So two calls, and the replay of a captured graph, give the same bits; candidates that follow with
 *   w = 0 do not change them; a shared candidate set (seq_stride_b = 0) gives the bits of the expanded one.
 * Three launches on `stream` (the forward kernel storing its rows, a backward chain per candidate, a fold over the
 *   candidates per frame), no allocation, no host synchronisation: safe under stream capture.
 * Arithmetic as for the scores; gamma within 2e-4 (T <= 300) / 5e-4 (T = 2000) of float64, so |grad - exact| <= that
 *   times sum_n |w[b, n]|.
 * A NULL x, in_len, seq, seq_len, w, grad or scratch, T, B, C, N or L < 1, blank >= C, a scratch not 8-byte aligned:
 * CTC_AMD_ERR_BAD_ARGUMENT; then L > 255, C > 4096 (only the staged path of ctc_amd_sequence_scores is taken), more than
 * 2^31 - 1 workgroups, scratch_bytes below the formula: CTC_AMD_ERR_UNSUPPORTED_SHAPE; all before any HIP call. */
size_t ctc_amd_sequence_scores_grad_scratch_bytes(int T, int B, int C, int N, int L, int blank);
int ctc_amd_sequence_scores_grad(const float *x, int64_t stride_t, int64_t stride_b, const int64_t *in_len,
                                 int T, int B, int C, int blank /* < 0: the no-blank lattice, x raw logits */,
                                 const void *seq, int seq_i64, int64_t seq_stride_b, int64_t seq_stride_n, int L,
                                 const int64_t *seq_len, int64_t len_stride_b, const int32_t *count /* or NULL */, int N,
                                 const float *w, int64_t w_stride_b,
                                 float *grad, int64_t grad_stride_t, int64_t grad_stride_b, float *scores /* or NULL */,
                                 void *scratch, size_t scratch_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* CTC_AMD_H */
