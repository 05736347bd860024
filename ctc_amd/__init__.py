"""ctc_amd -- MI355X-native CTC loss engine (hand-written HIP for gfx950).

Drop-in for the loss path of gotaku6629/CTC: ``CTCLoss.apply`` plus ``NoBlankCTC`` /
``NoBlankBinaryCTC`` / ``BlankCTC`` modules over the C ABI of include/ctc_amd.h.
"""
from ._lib import CtcAmdError, SO_PATH  # noqa: F401
from .functional import (CTCLoss, binary_best_path, binary_ctc_loss, binary_posteriors, blank_best_path, blank_ctc_loss,  # noqa: F401
                         blank_posteriors, blank_token_spans, BlankTokenSpans,
                         blank_forced_align, check_status, collective_gate,
                         dedup_multihot_targets,
                         noblank_best_path, noblank_ctc_loss, noblank_posteriors, release_workspaces, set_blank_schedule,
                         TokenSpans, binary_token_spans, noblank_token_spans,
                         workspace_status,
                         CollapsedTokens, collapse_frames, edit_distance, label_error_rate,
                         BeamHypotheses, FusedBeamHypotheses, blank_beam_search, noblank_beam_search,
                         blank_sequence_scores, noblank_sequence_scores)
from .modules import BlankCTC, NoBlankBinaryCTC, NoBlankCTC  # noqa: F401
from .producer import LSTM_cell, head_backward, head_forward, lstm_backward, lstm_cell_step, lstm_forward, lstm_series  # noqa: F401
from .producer import lstm_bias_grad_wide, lstm_series_backward_wide, lstm_series_wide  # noqa: F401
from .producer import head_backward_wide, head_forward_wide  # noqa: F401

__all__ = ["CTCLoss", "NoBlankCTC", "NoBlankBinaryCTC", "BlankCTC", "noblank_ctc_loss",
           "binary_ctc_loss", "blank_ctc_loss", "noblank_best_path", "noblank_posteriors", "CtcAmdError",
           "workspace_status", "release_workspaces", "check_status", "set_blank_schedule", "dedup_multihot_targets", "collective_gate", "LSTM_cell", "head_forward", "head_backward", "lstm_cell_step", "lstm_series", "lstm_forward", "lstm_backward", "lstm_series_wide", "lstm_series_backward_wide", "lstm_bias_grad_wide", "head_forward_wide", "head_backward_wide", "binary_posteriors", "binary_best_path",
           "blank_best_path", "blank_forced_align", "blank_posteriors", "blank_token_spans", "BlankTokenSpans",
           "TokenSpans", "noblank_token_spans", "binary_token_spans",
           "CollapsedTokens", "collapse_frames", "edit_distance", "label_error_rate",
           "BeamHypotheses", "FusedBeamHypotheses", "blank_beam_search", "noblank_beam_search",
           "blank_sequence_scores", "noblank_sequence_scores"]
