// Scores of candidate label sequences, gfx950: the forward entry.  The kernel, its description and its
// launch plan are in sequence_scores.hpp, which the gradient entry (sequence_scores_grad.hip) shares.
#include "sequence_scores.hpp"

using namespace ctc;

extern "C" int ctc_amd_sequence_scores(const float *x, int64_t stride_t, int64_t stride_b, const int64_t *in_len,
                                       int T, int B, int C, int blank,
                                       const void *seq, int seq_i64, int64_t seq_stride_b, int64_t seq_stride_n, int L,
                                       const int64_t *seq_len, int64_t len_stride_b, const int32_t *count,
                                       int N, float *scores, void *stream)
{
    if (!x || !in_len || !seq || !seq_len || !scores) return CTC_AMD_ERR_BAD_ARGUMENT;
    if (T < 1 || B < 1 || C < 1 || N < 1 || L < 1 || blank >= C) return CTC_AMD_ERR_BAD_ARGUMENT;
    if (L > kSeqMaxL) return CTC_AMD_ERR_UNSUPPORTED_SHAPE;
    const int64_t groups = ((int64_t)N + kSeqGroup - 1) / kSeqGroup;
    if (groups * B > INT_MAX) return CTC_AMD_ERR_UNSUPPORTED_SHAPE;
    SeqParams p;
    p.x = x; p.st = stride_t; p.sb = stride_b; p.in_len = in_len;
    p.T = T; p.B = B; p.C = C; p.blank = blank < 0 ? -1 : blank;
    p.seq = seq; p.is64 = seq_i64 != 0; p.seq_sb = seq_stride_b; p.seq_sn = seq_stride_n; p.L = L;
    p.len = seq_len; p.len_sb = len_stride_b; p.count = count;
    p.N = N; p.groups = (int)groups; p.scores = scores;
    return seq_launch<false>(p, static_cast<hipStream_t>(stream));
}
