// Gradient of the sequence scores, gfx950:
//     grad[t, b, c] = sum over the candidates n of sample b whose score is finite of  w[b, n] d score[b, n] / d x[t, b, c]
// on both lattices of sequence_scores.hpp.  Three launches on the caller's stream, nothing between workgroups, no atomics:
// every sum has one order, fixed by the code, so two calls (or a graph replay) give the same bits.
//   1  sequence_scores_kernel<.., STORE>   the forward kernel itself with its row sink: the scores (the forward entry's
//                                          bits), and per candidate and frame the states alpha_t(s), s < S, in the log2
//                                          domain, their emissions e_t(s) and the integer offset the states are relative to.
//   2  seq_beta_kernel                     one wave per candidate whose score is finite, from frame T_b - 1 down: beta in
//                                          registers (K = 1 / 2 / 4 / 8 states per lane like the forward chain, neighbours by
//                                          DPP wave_shl, an exact offset of its own every 8 frames), fed by the stored
//                                          emissions -- consecutive floats, four frames in flight -- and
//                                          gamma_t(s) = 2^(alpha + beta - total + offsets) written over alpha_t(s) in place.
//                                          It also ranks every label among the earlier equal labels of its candidate.
//   3  seq_fold_kernel                     one wave per group of frames of a sample, a row of C floats in LDS per frame:
//                                          the row starts at 0 (blank lattice) or at -(sum of the live w) softmax(x_t)
//                                          (no-blank: the row's log-sum-exp once for all candidates), then the candidates
//                                          in the order n = 0, 1, ..: gamma divided by the frame's sum over the candidate's
//                                          states (1 in exact arithmetic: the drift alpha, beta and the total share over
//                                          a long clip goes out); the blank states' w gamma summed per lane in state order
//                                          and across the wave by the fixed DPP tree, one add; the label states in rounds
//                                          of their rank (round r: the (r+1)-th occurrence of every class -- distinct
//                                          classes, so the lanes' read-modify-writes never meet).  The row is stored once;
//                                          rows t >= T_b are stored as zeros.  Every element of grad is written.
// Scratch (ctc_amd_sequence_scores_grad_scratch_bytes): offsets [B N][T] double, alpha / gamma [B N][T][S_L] float,
// emissions the same, ranks [B N][L + 1] int32 (slot L: the largest rank), scores [B N] float.
#include "sequence_scores.hpp"

namespace ctc {

constexpr int kSeqBetaDepth = 4;                                // frames of a candidate in flight in the beta pass
constexpr int kSeqFoldWaves = 4;                                // waves of a fold workgroup
constexpr int kSeqFoldLdsFloats = 16384;                        // 64 KB: C floats per row, rows per wave = 4096 / C in [1, 8]
constexpr int kSeqFoldMaxRows = 8;
constexpr int kSeqPasses = 8;                                   // 64 states per pass cover the 511 of a candidate

struct SeqGradParams {
    SeqParams f;
    const float *w;                             // [B][N] through w_sb
    int64_t w_sb;
    float *grad;                                // [T][B][C] through (gst, gsb)
    int64_t gst, gsb;
    int32_t *rank;                              // [B N][L + 1]
    int RW;                                     // rows per wave of the fold kernel
};

inline int seq_states(int L, int blank) { return blank >= 0 ? 2 * L + 1 : L; }

__host__ __device__ inline int seq_clamp_len(int64_t Tb64, int T) { return Tb64 < 0 ? 0 : (Tb64 > T ? T : (int)Tb64); }

__device__ __forceinline__ bool seq_finite(float v) { return fabsf(v) < __builtin_inff(); }   // (false for NaN)

// beta of one candidate whose score is finite (so T_b >= 1, 0 <= len <= L, every label inside the row), K states per lane.
// A / E / O: the candidate's rows as the forward pass left them.
template <bool BLANK, int K>
__device__ __forceinline__ void seq_beta(const SeqGradParams &g, int Tb, const void *q, int len, float *A, const float *E,
                                         const double *O)
{
    constexpr int D = kSeqBetaDepth;
    const float ninf = -__builtin_inff();
    const int lane = lane_id(), SL = g.f.SL, S = BLANK ? 2 * len + 1 : len;
    bool skip_up[K], fin[K];                                    // s -> s + 2 is a transition; s is a state of the read-out
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const int s = lane * K + j;
        skip_up[j] = false;
        if (BLANK && (s & 1) != 0 && s + 2 < S) {
            const int i = (s - 1) >> 1;
            skip_up[j] = seq_label(q, g.f.is64, i) != seq_label(q, g.f.is64, i + 1);
        }
        fin[j] = s == S - 1 || (BLANK && s == S - 2);
    }

    // the total, in the log2 domain, from the row the forward read-out used: otot + ftot
    float v = ninf, al[K];
    {
        const float *row = A + (int64_t)(Tb - 1) * SL;
#pragma unroll
        for (int j = 0; j < K; ++j) {
            const int s = lane * K + j;
            al[j] = s < S ? row[s] : ninf;
            if (fin[j]) v = fmaxf(v, al[j]);
        }
    }
    const float M = wave_max(v);
    if (!(M > ninf)) return;
    float sum = 0.0f;
#pragma unroll
    for (int j = 0; j < K; ++j)
        if (fin[j]) sum += __builtin_amdgcn_exp2f(al[j] - M);
    sum = wave_sum(sum);
    const float ftot = M + __builtin_amdgcn_logf(sum);
    const double otot = O[Tb - 1];

    auto load = [&](int t, float (&xa)[K], float (&xe)[K], double &xo) {
        if (t < 0) return;                                      // (wave-uniform)
        const float *ra = A + (int64_t)t * SL, *re = E + (int64_t)t * SL;
#pragma unroll
        for (int j = 0; j < K; ++j) {
            const int s = lane * K + j;
            xa[j] = s < S ? ra[s] : ninf;
            xe[j] = s < S ? re[s] : ninf;
        }
        xo = O[t];
    };

    float ca[D][K], ce[D][K], na[D][K], ne[D][K];
    double co[D], no[D];
#pragma unroll
    for (int d = 0; d < D; ++d) {
        co[d] = 0.0; no[d] = 0.0;
#pragma unroll
        for (int j = 0; j < K; ++j) { ca[d][j] = ninf; ce[d][j] = ninf; na[d][j] = ninf; ne[d][j] = ninf; }
    }
#pragma unroll
    for (int d = 0; d < D; ++d) load(Tb - 1 - d, ca[d], ce[d], co[d]);

    float bt[K];                                                // beta of frame t + 1, its emission included
#pragma unroll
    for (int j = 0; j < K; ++j) bt[j] = ninf;
    double offb = 0.0;
    for (int tc = Tb - 1; tc >= 0; tc -= D) {
#pragma unroll
        for (int d = 0; d < D; ++d) load(tc - D - d, na[d], ne[d], no[d]);     // in flight across this chunk's steps
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const int t = tc - d;
            if (t < 0) break;
            float bb[K];                                        // beta of frame t without its emission
            if (t == Tb - 1) {
#pragma unroll
                for (int j = 0; j < K; ++j) bb[j] = fin[j] ? 0.0f : ninf;
            } else {
                // states s + 1 and s + 2 of the lane's last states: the first ones of the lane above
                const float n1 = wave_shl1(bt[0], ninf);
                float n2 = ninf;
                if constexpr (BLANK && K == 1) n2 = wave_shl1(n1, ninf);
                if constexpr (BLANK && K >= 2) n2 = wave_shl1(bt[1], ninf);
#pragma unroll
                for (int j = 0; j < K; ++j) {
                    const float u1 = j + 1 < K ? bt[j + 1 < K ? j + 1 : 0] : n1;
                    if (BLANK && (K == 1 || (j & 1) != 0)) {    // (K >= 2: the even states of a lane are blanks, no skip)
                        const float u2 = j + 2 < K ? bt[j + 2 < K ? j + 2 : 0] : (j + 2 == K ? n1 : n2);
                        bb[j] = seq_lse3(bt[j], u1, skip_up[j] ? u2 : ninf);
                    } else {
                        bb[j] = seq_lse2(bt[j], u1);
                    }
                }
            }
            const float shift = (float)(co[d] + offb - otot);   // (integers in doubles: exact)
            float *row = A + (int64_t)t * SL;
#pragma unroll
            for (int j = 0; j < K; ++j) {
                const int s = lane * K + j;
                const float gm = __builtin_amdgcn_exp2f((ca[d][j] + bb[j] - ftot) + shift);
                if (s < S) row[s] = gm;
                bt[j] = bb[j] + ce[d][j];
            }
            if ((t & (kSeqRenorm - 1)) == 0) {
                float m = bt[0];
#pragma unroll
                for (int j = 1; j < K; ++j) m = fmaxf(m, bt[j]);
                m = wave_max(m);
                if (m > ninf) {
                    const float fl = floorf(m);
#pragma unroll
                    for (int j = 0; j < K; ++j) bt[j] -= fl;
                    offb += (double)fl;
                }
            }
        }
#pragma unroll
        for (int d = 0; d < D; ++d) {
            co[d] = no[d];
#pragma unroll
            for (int j = 0; j < K; ++j) { ca[d][j] = na[d][j]; ce[d][j] = ne[d][j]; }
        }
    }
}

template <bool BLANK>
__global__ __launch_bounds__(kWave) void seq_beta_kernel(SeqGradParams g)
{
    const SeqParams &p = g.f;
    const int64_t cand = blockIdx.x;
    const int b = (int)(cand / p.N), n = (int)(cand % p.N);
    const float score = p.scores[cand];
    if (!seq_finite(score)) return;                             // absent, not scored, no alignment: nothing to give
    const int Tb = seq_clamp_len(p.in_len[b], p.T);
    if (Tb == 0) return;
    const int len = __builtin_amdgcn_readfirstlane((int)p.len[(int64_t)b * p.len_sb + n]);   // (finite score: 0 <= len <= L)
    if (len < 0 || len > p.L) return;
    const char *q = static_cast<const char *>(p.seq) +
                    ((int64_t)b * p.seq_sb + (int64_t)n * p.seq_sn) * (p.is64 ? 8 : 4);
    const int lane = lane_id();

    // rank of label i: the earlier labels of the candidate that are equal to it
    int32_t *rk = g.rank + cand * (p.L + 1);
    int top = 0;
    for (int i = lane; i < len; i += kWave) {
        const int64_t lab = seq_label(q, p.is64, i);
        int r = 0;
        for (int k = 0; k < i; ++k) r += seq_label(q, p.is64, k) == lab;
        rk[i] = r;
        top = max(top, r);
    }
    top = (int)wave_max((float)top);
    if (lane == 0) rk[p.L] = top;

    const int64_t rows = cand * p.T;
    float *A = p.sink_a + rows * p.SL;
    const float *E = p.sink_e + rows * p.SL;
    const double *O = p.sink_off + rows;
    const int S = BLANK ? 2 * len + 1 : len;
    if (S <= kWave) seq_beta<BLANK, 1>(g, Tb, q, len, A, E, O);
    else if (S <= 2 * kWave) seq_beta<BLANK, 2>(g, Tb, q, len, A, E, O);
    else if (S <= 4 * kWave) seq_beta<BLANK, 4>(g, Tb, q, len, A, E, O);
    else seq_beta<BLANK, 8>(g, Tb, q, len, A, E, O);
}

// Wave w of workgroup (b, chunk) folds frames [t0, t0 + RW), t0 = (chunk kSeqFoldWaves + w) RW, into its own RW rows of LDS.
template <bool BLANK>
__global__ __launch_bounds__(kSeqFoldWaves * kWave) void seq_fold_kernel(SeqGradParams g, int chunks)
{
    extern __shared__ float4 fold_raw[];
    const SeqParams &p = g.f;
    const int lane = lane_id(), wave = wave_id(), C = p.C, RW = g.RW, SL = p.SL;
    const int b = blockIdx.x / chunks, chunk = blockIdx.x % chunks;
    const int t0 = (chunk * kSeqFoldWaves + wave) * RW;
    if (t0 >= p.T) return;                                      // (no barrier in this kernel: waves are independent)
    float *acc = reinterpret_cast<float *>(fold_raw) + (size_t)wave * RW * C;
    const int Tb = seq_clamp_len(p.in_len[b], p.T);
    const int live = max(0, min(RW, Tb - t0)), rows = min(RW, p.T - t0);
    const float *xb = p.x + (int64_t)b * p.sb;
    float *gb = g.grad + (int64_t)b * g.gsb;

    if (live > 0) {
        if constexpr (BLANK) {
            for (int e = lane; e < live * C; e += kWave) acc[e] = 0.0f;
        } else {
            float wsum = 0.0f;                                  // the weights of the candidates that give a gradient, in order
            for (int n = 0; n < p.N; ++n)
                if (seq_finite(p.scores[(int64_t)b * p.N + n])) wsum += g.w[(int64_t)b * g.w_sb + n];
            for (int r = 0; r < live; ++r) {
                const float *xr = xb + (int64_t)(t0 + r) * p.st;
                const float l2 = seq_row_lse2(xr, C, lane);
                for (int c = lane; c < C; c += kWave)
                    acc[r * C + c] = 0.0f - wsum * __builtin_amdgcn_exp2f(__builtin_fmaf(xr[c], kLog2e, -l2));
            }
        }
        for (int n = 0; n < p.N; ++n) {
            const int64_t cand = (int64_t)b * p.N + n;
            if (!seq_finite(p.scores[cand])) continue;          // skipped by the score, whatever w holds (wave-uniform)
            const float wn = g.w[(int64_t)b * g.w_sb + n];
            const int len = __builtin_amdgcn_readfirstlane((int)p.len[(int64_t)b * p.len_sb + n]);
            if (len < 0 || len > p.L) continue;
            const int S = BLANK ? 2 * len + 1 : len, passes = (S + kWave - 1) / kWave;
            const char *q = static_cast<const char *>(p.seq) +
                            ((int64_t)b * p.seq_sb + (int64_t)n * p.seq_sn) * (p.is64 ? 8 : 4);
            const int32_t *rk = g.rank + cand * (p.L + 1);
            const int top = __builtin_amdgcn_readfirstlane(rk[p.L]);
            int col[kSeqPasses], rnk[kSeqPasses];               // label states: class and rank; -1: a blank or no state
#pragma unroll
            for (int k = 0; k < kSeqPasses; ++k) {
                const int s = k * kWave + lane;
                col[k] = 0; rnk[k] = -1;
                const bool is_label = BLANK ? (s & 1) != 0 : true;
                const int i = BLANK ? (s - 1) >> 1 : s;
                if (k < passes && s < S && is_label) {
                    const int64_t lab = seq_label(q, p.is64, i);
                    if (lab >= 0 && lab < C) { col[k] = (int)lab; rnk[k] = rk[i]; }     // (a finite score: always)
                }
            }
            const float *A = p.sink_a + cand * p.T * SL;
            for (int r = 0; r < live; ++r) {
                const float *row = A + (int64_t)(t0 + r) * SL;
                // The posteriors of a frame sum to 1 (every alignment is in exactly one state there).  What alpha, beta and
                // the total have drifted apart over a long clip -- roundings that all states of the frame share -- is in
                // the frame's sum: dividing by it leaves the roundings that differ from state to state.
                float gm[kSeqPasses], bsum = 0.0f, tot = 0.0f;
#pragma unroll
                for (int k = 0; k < kSeqPasses; ++k) {
                    const int s = k * kWave + lane;
                    gm[k] = (k < passes && s < S) ? row[s] : 0.0f;
                    tot += gm[k];
                }
                tot = wave_sum(tot);
                const float scale = tot > 0.0f ? wn / tot : 0.0f;
#pragma unroll
                for (int k = 0; k < kSeqPasses; ++k) {
                    const int s = k * kWave + lane;
                    gm[k] *= scale;
                    if (BLANK && (s & 1) == 0) bsum += gm[k];
                }
                if constexpr (BLANK) {
                    bsum = wave_sum(bsum);
                    if (lane == 0) acc[r * C + p.blank] += bsum;
                }
                for (int rr = 0; rr <= top; ++rr) {
#pragma unroll
                    for (int k = 0; k < kSeqPasses; ++k)
                        if (k < passes && rnk[k] == rr) acc[r * C + col[k]] += gm[k];
                    lds_order();
                }
            }
        }
    }
    for (int r = 0; r < rows; ++r) {
        float *out = gb + (int64_t)(t0 + r) * g.gst;
        if (r < live) {
            for (int c = lane; c < C; c += kWave) stream_store(out + c, acc[r * C + c]);
        } else {
            for (int c = lane; c < C; c += kWave) stream_store(out + c, 0.0f);
        }
    }
}

inline size_t seq_grad_scratch(int T, int B, int N, int L, int blank, size_t *a_off, size_t *e_off, size_t *r_off,
                               size_t *s_off)
{
    const size_t cands = (size_t)B * N, rows = cands * T, SL = (size_t)seq_states(L, blank);
    size_t at = rows * sizeof(double);
    if (a_off) *a_off = at;
    at += rows * SL * sizeof(float);
    if (e_off) *e_off = at;
    at += rows * SL * sizeof(float);
    if (r_off) *r_off = at;
    at += cands * ((size_t)L + 1) * sizeof(int32_t);
    if (s_off) *s_off = at;
    at += cands * sizeof(float);
    return (at + 255) & ~(size_t)255;
}

}  // namespace ctc

using namespace ctc;

extern "C" size_t ctc_amd_sequence_scores_grad_scratch_bytes(int T, int B, int C, int N, int L, int blank)
{
    if (T < 1 || B < 1 || C < 1 || N < 1 || L < 1 || L > kSeqMaxL || blank >= C || C > kSeqStagedMaxC) return 0;
    return seq_grad_scratch(T, B, N, L, blank, nullptr, nullptr, nullptr, nullptr);
}

extern "C" int ctc_amd_sequence_scores_grad(const float *x, int64_t stride_t, int64_t stride_b, const int64_t *in_len,
                                            int T, int B, int C, int blank,
                                            const void *seq, int seq_i64, int64_t seq_stride_b, int64_t seq_stride_n, int L,
                                            const int64_t *seq_len, int64_t len_stride_b, const int32_t *count, int N,
                                            const float *w, int64_t w_stride_b,
                                            float *grad, int64_t grad_stride_t, int64_t grad_stride_b, float *scores,
                                            void *scratch, size_t scratch_bytes, void *stream)
{
    if (!x || !in_len || !seq || !seq_len || !w || !grad || !scratch) return CTC_AMD_ERR_BAD_ARGUMENT;
    if (T < 1 || B < 1 || C < 1 || N < 1 || L < 1 || blank >= C) return CTC_AMD_ERR_BAD_ARGUMENT;
    if (reinterpret_cast<uintptr_t>(scratch) % 8 != 0) return CTC_AMD_ERR_BAD_ARGUMENT;
    if (L > kSeqMaxL || C > kSeqStagedMaxC) return CTC_AMD_ERR_UNSUPPORTED_SHAPE;
    const int64_t groups = ((int64_t)N + kSeqGroup - 1) / kSeqGroup;
    if (groups * B > INT_MAX || (int64_t)B * N > INT_MAX) return CTC_AMD_ERR_UNSUPPORTED_SHAPE;
    SeqGradParams g;
    SeqParams &p = g.f;
    p.x = x; p.st = stride_t; p.sb = stride_b; p.in_len = in_len;
    p.T = T; p.B = B; p.C = C; p.blank = blank < 0 ? -1 : blank;
    p.seq = seq; p.is64 = seq_i64 != 0; p.seq_sb = seq_stride_b; p.seq_sn = seq_stride_n; p.L = L;
    p.len = seq_len; p.len_sb = len_stride_b; p.count = count;
    p.N = N; p.groups = (int)groups;
    size_t a_off, e_off, r_off, s_off;
    if (scratch_bytes < seq_grad_scratch(T, B, N, L, p.blank, &a_off, &e_off, &r_off, &s_off))
        return CTC_AMD_ERR_UNSUPPORTED_SHAPE;
    int RW = kSeqFoldLdsFloats / kSeqFoldWaves / C;
    RW = RW < 1 ? 1 : (RW > kSeqFoldMaxRows ? kSeqFoldMaxRows : RW);
    const int64_t chunks = ((int64_t)T + kSeqFoldWaves * RW - 1) / (kSeqFoldWaves * RW);
    if (chunks * B > INT_MAX) return CTC_AMD_ERR_UNSUPPORTED_SHAPE;
    char *base = static_cast<char *>(scratch);
    p.sink_off = reinterpret_cast<double *>(base);
    p.sink_a = reinterpret_cast<float *>(base + a_off);
    p.sink_e = reinterpret_cast<float *>(base + e_off);
    p.SL = seq_states(L, p.blank);
    g.rank = reinterpret_cast<int32_t *>(base + r_off);
    p.scores = scores ? scores : reinterpret_cast<float *>(base + s_off);
    g.w = w; g.w_sb = w_stride_b;
    g.grad = grad; g.gst = grad_stride_t; g.gsb = grad_stride_b;
    g.RW = RW;
    hipStream_t s = static_cast<hipStream_t>(stream);
    int rc = seq_launch<true>(p, s);
    if (rc != 0) return rc;
    const dim3 cands((unsigned)((int64_t)B * N)), wave(kWave);
    rc = p.blank >= 0 ? launch<seq_beta_kernel<true>>(cands, wave, 0, s, g)
                      : launch<seq_beta_kernel<false>>(cands, wave, 0, s, g);
    if (rc != 0) return rc;
    const dim3 fold((unsigned)(chunks * B)), threads(kSeqFoldWaves * kWave);
    const size_t lds = (size_t)kSeqFoldWaves * RW * C * sizeof(float);
    return p.blank >= 0 ? launch<seq_fold_kernel<true>>(fold, threads, lds, s, g, (int)chunks)
                        : launch<seq_fold_kernel<false>>(fold, threads, lds, s, g, (int)chunks);
}
