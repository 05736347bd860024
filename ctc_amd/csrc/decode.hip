// Best-path (Viterbi) alignment on the no-blank lattice, gfx950.
//
// The max-semiring twin of the alpha recursion (computes_transition, NoBlankCTC.py:71-87,
// with max in place of _logsumexp): v_t(l) = max(v_{t-1}(l), v_{t-1}(l-1)) + lp_t(lab_l),
// first step "stay" only (:75-76), states l >= L_b masked (:79-80), read out at
// (T_b-1, L_b-1) like the loss (:58-68,139).  SURVEY 8(f) rank 1: the reference has no such
// routine (it evaluates with per-step argmax and DTW-like helpers, train.py:82-136,434), so
// there is no reference output to pin this against (parity unpinned).
//
// One 256-thread workgroup per sample: every wave normalises rows (log-softmax statistics,
// emission gather) into LDS; wave 0 runs the max-scan, one state per lane and K states
// per lane for S > 64, recording one back-pointer byte per cell; lane 0 walks them back.
// decode_spans.hpp (token spans) runs the same emission stage and the same max-scan beside the alpha / beta' chains.
#include "lattice.hpp"
#include "launch.hpp"

namespace ctc {

struct DecodeParams {
    const void *x;                              // logits [T,B,C] of the kernel's element type E (float, __bf16, _Float16)
    int64_t st, sb;
    const void *lab;
    int lab64;
    const int64_t *in_len, *tgt_len;
    int T, B, C, S, SP;
    int32_t *path;
    float *score;
};

constexpr int kDecThreads = 256;
constexpr int kDecWaves = kDecThreads / kWave;

// the max-scan over em[T_b][SP] by ONE wave (one back-pointer byte per cell), the read-out and the walk back
template <int K>
__device__ __forceinline__ void viterbi_wave(const float *em, unsigned char *bp, const DecodeParams &p, int b, int Tb, int L, bool ok,
                                             int *lpath = nullptr)          // lpath (LDS, [T]): the path once more, for the workgroup
{
    const int lane = lane_id();
    {
        const int l0 = lane * K;
        float a[K];
        float sc = 0.f;
        if (Tb > 0) {
#pragma unroll
            for (int k = 0; k < K; ++k) {
                a[k] = (l0 + k == 0) ? em[0] : kNeg;
                if (l0 + k < p.SP) bp[l0 + k] = 0;
            }
            for (int t = 1; t < Tb; ++t) {
                const float nb = wave_shr1(a[K - 1], kNeg);
                float n[K];
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    const int l = l0 + k;
                    const float adv = k == 0 ? nb : a[k - 1];
                    const bool take = adv > a[k];                           // ties: stay
                    const float e = l < p.SP ? em[t * p.SP + l] : kNeg;
                    n[k] = (take ? adv : a[k]) + e;
                    if (l < p.SP) bp[t * p.SP + l] = take ? 1 : 0;
                }
#pragma unroll
                for (int k = 0; k < K; ++k) a[k] = n[k];
            }
            // score = v[T_b-1][L_b-1]
#pragma unroll
            for (int k = 0; k < K; ++k) sc += (l0 + k == L - 1) ? a[k] : 0.f;
            sc = wave_sum(sc);
        }
        const bool feasible = ok && sc > -kInfeasible;
        if (lane == 0) {
            p.score[b] = feasible ? sc : -__builtin_inff();
            int32_t *out = p.path + (int64_t)b * p.T;
            int l = L - 1;
            for (int t = p.T - 1; t >= 0; --t) {
                if (!feasible || t >= Tb) {
                    out[t] = -1;
                    if (lpath) lpath[t] = -1;
                    continue;
                }
                out[t] = l;
                if (lpath) lpath[t] = l;
                if (bp[t * p.SP + l]) --l;
            }
        }
    }
}

// The emission stage of the no-blank read-outs, by the NW waves of a workgroup: the sample's label classes into lab[SP]
// (negative labels wrap), then per row the log-softmax statistics and em[t][l] = lp_t(lab_l) for l < L, the sentinel
// beyond.  Shared by the best-path and the token-span kernels: the same statements, so the same bits in em.
// E: the element type of the logits; it only decides how logit_f32 (common.hpp) brings one into an fp32 register.
template <int NW, typename E>
__device__ __forceinline__ void noblank_emissions(const DecodeParams &p, float *em, int *lab, int b, int Tb, int L)
{
    const int tid = threadIdx.x, w = wave_id(), lane = lane_id();
    for (int l = tid; l < p.SP; l += NW * kWave) {
        int k = 0;
        if (l < L) {
            k = load_label(p.lab, p.lab64, (int64_t)b * p.S + l) % p.C;
            if (k < 0) k += p.C;
        }
        lab[l] = k;
    }
    __syncthreads();
    for (int t = w; t < Tb; t += NW) {                                      // rows: any C
        const E *row = static_cast<const E *>(p.x) + (int64_t)t * p.st + (int64_t)b * p.sb;
        float m = -__builtin_inff();
        for (int c = lane; c < p.C; c += kWave) m = fmaxf(m, logit_f32(row + c));
        m = wave_max(m);
        float s = 0.f;
        for (int c = lane; c < p.C; c += kWave) s += fast_exp(logit_f32(row + c) - m);
        s = wave_sum(s);
        const float lsum = fast_log(s);
        for (int l = lane; l < p.SP; l += kWave) em[t * p.SP + l] = (l < L) ? fmaxf((logit_f32(row + lab[l]) - m) - lsum, kMasked) : kNeg;
    }
}

// The same for the binary lattice: per row the two clamped logs, their difference in the wave's own LDS row
// (drow [NW][C]), one dot product per label row of the targets y [B,S,C].
template <int NW, typename E>
__device__ __forceinline__ void binary_emissions(const DecodeParams &p, const float *y, float *em, float *drow, int b, int Tb,
                                                 int L)
{
    const int w = wave_id(), lane = lane_id();
    const float *yb = y + (int64_t)b * p.S * p.C;
    float *d = drow + (size_t)w * p.C;
    const float invC = 1.0f / (float)p.C;
    for (int t = w; t < Tb; t += NW) {
        const E *row = static_cast<const E *>(p.x) + (int64_t)t * p.st + (int64_t)b * p.sb;
        float q = 0.f;
        for (int c = lane; c < p.C; c += kWave) {
            float pr, lp, lq;
            bce_logs(logit_f32(row + c), pr, lp, lq);
            d[c] = lp - lq;
            q += lq;
        }
        q = wave_sum(q);
        for (int l = 0; l < p.SP; ++l) {                                    // (the wave's own LDS row: in order)
            float e = kNeg;
            if (l < L) {
                float acc = 0.f;
                for (int c = lane; c < p.C; c += kWave) acc = __builtin_fmaf(yb[(int64_t)l * p.C + c], d[c], acc);
                e = (wave_sum(acc) + q) * invC;
            }
            if (lane == 0) em[t * p.SP + l] = e;
        }
    }
}

template <int K, typename E = float>
__global__ __launch_bounds__(kDecThreads) void noblank_best_path_kernel(DecodeParams p)
{
    extern __shared__ float4 smem_raw[];
    float *em = reinterpret_cast<float *>(smem_raw);                       // [T][SP]
    int *lab = reinterpret_cast<int *>(em + (size_t)p.T * p.SP);            // [SP]
    unsigned char *bp = reinterpret_cast<unsigned char *>(lab + p.SP);      // [T][SP]: 1 = came from l-1
    const int b = blockIdx.x, w = wave_id();
    const int64_t Tb64 = p.in_len[b], L64 = p.tgt_len[b];
    const bool ok = L64 >= 1 && L64 <= p.S && Tb64 >= L64 && Tb64 <= p.T;
    const int Tb = ok ? (int)Tb64 : 0, L = ok ? (int)L64 : 0;

    noblank_emissions<kDecWaves, E>(p, em, lab, b, Tb, L);
    __syncthreads();

    if (w == 0) viterbi_wave<K>(em, bp, p, b, Tb, L, ok);
}

// The same read-out on the lattice of the binary (multi-label sigmoid) variant: cell (t, l) costs
// -nn.BCELoss()(sigmoid(x[t,b,:]), y[b,l,:]) (NoBlankBinaryCTC.py:112,:88,:146) -- per row the two clamped logs, their
// difference in a wave-private LDS row, one dot product per label row of the targets.
template <int K, typename E = float>
__global__ __launch_bounds__(kDecThreads) void binary_best_path_kernel(DecodeParams p, const float *y)
{
    extern __shared__ float4 smem_raw[];
    float *em = reinterpret_cast<float *>(smem_raw);                       // [T][SP]
    float *drow = em + (size_t)p.T * p.SP;                                 // [kDecWaves][C]
    unsigned char *bp = reinterpret_cast<unsigned char *>(drow + (size_t)kDecWaves * p.C);   // [T][SP]
    const int b = blockIdx.x, w = wave_id();
    const int64_t Tb64 = p.in_len[b], L64 = p.tgt_len[b];
    const bool ok = L64 >= 1 && L64 <= p.S && Tb64 >= L64 && Tb64 <= p.T;
    const int Tb = ok ? (int)Tb64 : 0, L = ok ? (int)L64 : 0;
    binary_emissions<kDecWaves, E>(p, y, em, drow, b, Tb, L);
    __syncthreads();
    if (w == 0) viterbi_wave<K>(em, bp, p, b, Tb, L, ok);
}

}  // namespace ctc

#include "decode_spans.hpp"

using namespace ctc;

static bool logit_dtype_known(int x_dtype) { return x_dtype == CTC_AMD_F32 || x_dtype == CTC_AMD_BF16 || x_dtype == CTC_AMD_F16; }

// Best paths: y == nullptr is the no-blank lattice (labels), else the binary one (targets y [B,S,C] float; SURVEY 8f-1: the
// reference has no such routine).  x_dtype: the element type of x, CTC_AMD_F32 for the untyped entries.
static int best_path_entry(const void *x, int x_dtype, int64_t stride_t, int64_t stride_b, const void *labels, int labels_i64,
                           const float *y, const int64_t *in_len, const int64_t *tgt_len, int T, int B, int C, int S,
                           int32_t *path, float *score, void *stream)
{
    if (!logit_dtype_known(x_dtype)) return CTC_AMD_ERR_BAD_ARGUMENT;
    if (!x || (!labels && !y) || !in_len || !tgt_len || !path || !score) return CTC_AMD_ERR_BAD_ARGUMENT;
    if (T < 1 || B < 1 || C < 1 || S < 1) return CTC_AMD_ERR_BAD_ARGUMENT;
    const auto [K, SP] = lane_states(S);
    if (K > 4) return CTC_AMD_ERR_UNSUPPORTED_SHAPE;
    DecodeParams p;
    p.x = x; p.st = stride_t; p.sb = stride_b;
    p.lab = labels; p.lab64 = labels_i64;
    p.in_len = in_len; p.tgt_len = tgt_len;
    p.T = T; p.B = B; p.C = C; p.S = S;
    p.SP = SP;
    p.path = path; p.score = score;
    const size_t smem = y ? ((size_t)T * p.SP + (size_t)kDecWaves * C) * 4 + (size_t)T * p.SP + 16
                          : ((size_t)T * p.SP + p.SP) * 4 + (size_t)T * p.SP + 16;
    if (smem > kMaxLds) return CTC_AMD_ERR_UNSUPPORTED_SHAPE;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid(B), block(kDecThreads);
    const int k = K;                                         // (a structured binding cannot be captured)
    return with_logit_elem(x_dtype, [&](auto elem) {
        using E = typename decltype(elem)::type;
        if (y) {
            switch (k) {
                case 1: return launch<binary_best_path_kernel<1, E>>(grid, block, smem, s, p, y);
                case 2: return launch<binary_best_path_kernel<2, E>>(grid, block, smem, s, p, y);
                default: return launch<binary_best_path_kernel<4, E>>(grid, block, smem, s, p, y);
            }
        }
        switch (k) {
            case 1: return launch<noblank_best_path_kernel<1, E>>(grid, block, smem, s, p);
            case 2: return launch<noblank_best_path_kernel<2, E>>(grid, block, smem, s, p);
            default: return launch<noblank_best_path_kernel<4, E>>(grid, block, smem, s, p);
        }
    });
}

extern "C" int ctc_amd_noblank_best_path(const float *x, int64_t stride_t, int64_t stride_b,
                                         const void *labels, int labels_i64,
                                         const int64_t *in_len, const int64_t *tgt_len,
                                         int T, int B, int C, int S,
                                         int32_t *path, float *score,
                                         void *workspace, void *stream)
{
    (void)workspace;
    if (!labels) return CTC_AMD_ERR_BAD_ARGUMENT;
    return best_path_entry(x, CTC_AMD_F32, stride_t, stride_b, labels, labels_i64, nullptr, in_len, tgt_len, T, B, C, S, path,
                           score, stream);
}

extern "C" int ctc_amd_noblank_best_path_typed(const void *x, int x_dtype, int64_t stride_t, int64_t stride_b,
                                               const void *labels, int labels_i64,
                                               const int64_t *in_len, const int64_t *tgt_len,
                                               int T, int B, int C, int S,
                                               int32_t *path, float *score,
                                               void *workspace, void *stream)
{
    (void)workspace;
    if (!labels) return CTC_AMD_ERR_BAD_ARGUMENT;
    return best_path_entry(x, x_dtype, stride_t, stride_b, labels, labels_i64, nullptr, in_len, tgt_len, T, B, C, S, path,
                           score, stream);
}

extern "C" int ctc_amd_binary_best_path(const float *x, int64_t stride_t, int64_t stride_b, const float *y,
                                        const int64_t *in_len, const int64_t *tgt_len,
                                        int T, int B, int C, int S,
                                        int32_t *path, float *score, void *workspace, void *stream)
{
    (void)workspace;
    if (!y) return CTC_AMD_ERR_BAD_ARGUMENT;
    return best_path_entry(x, CTC_AMD_F32, stride_t, stride_b, nullptr, 0, y, in_len, tgt_len, T, B, C, S, path, score, stream);
}

extern "C" int ctc_amd_binary_best_path_typed(const void *x, int x_dtype, int64_t stride_t, int64_t stride_b, const float *y,
                                              const int64_t *in_len, const int64_t *tgt_len,
                                              int T, int B, int C, int S,
                                              int32_t *path, float *score, void *workspace, void *stream)
{
    (void)workspace;
    if (!y) return CTC_AMD_ERR_BAD_ARGUMENT;
    return best_path_entry(x, x_dtype, stride_t, stride_b, nullptr, 0, y, in_len, tgt_len, T, B, C, S, path, score, stream);
}


// Token spans: one launch of decode_spans.hpp's kernel per call.
static int token_spans_entry(const void *x, int x_dtype, int64_t stride_t, int64_t stride_b, const void *labels, int labels_i64,
                             const float *y, const int64_t *in_len, const int64_t *tgt_len, int T, int B, int C, int S,
                             int32_t *path, float *score, float *nll, float *frame_conf, int32_t *start, int32_t *end,
                             float *conf, void *stream)
{
    if (!logit_dtype_known(x_dtype)) return CTC_AMD_ERR_BAD_ARGUMENT;
    if (!x || (!labels && !y) || !in_len || !tgt_len || !path || !score || !nll || !frame_conf || !start || !end || !conf)
        return CTC_AMD_ERR_BAD_ARGUMENT;
    if (T < 1 || B < 1 || C < 1 || S < 1) return CTC_AMD_ERR_BAD_ARGUMENT;
    const auto [K, SP] = lane_states(S);
    if (K > 4) return CTC_AMD_ERR_UNSUPPORTED_SHAPE;
    TokenSpanParams q;
    DecodeParams &p = q.d;
    p.x = x; p.st = stride_t; p.sb = stride_b;
    p.lab = labels; p.lab64 = labels_i64;
    p.in_len = in_len; p.tgt_len = tgt_len;
    p.T = T; p.B = B; p.C = C; p.S = S;
    p.SP = SP;
    p.path = path; p.score = score;
    q.nll = nll; q.frame_conf = frame_conf;
    q.start = start; q.end = end; q.conf = conf;
    const int k = K;
    return with_logit_elem(x_dtype, [&](auto elem) {
        return run_token_spans<typename decltype(elem)::type>(q, y, k, static_cast<hipStream_t>(stream));
    });
}

extern "C" int ctc_amd_noblank_token_spans(const float *x, int64_t stride_t, int64_t stride_b,
                                           const void *labels, int labels_i64,
                                           const int64_t *in_len, const int64_t *tgt_len,
                                           int T, int B, int C, int S,
                                           int32_t *path, float *score, float *nll, float *frame_conf,
                                           int32_t *start, int32_t *end, float *conf,
                                           void *workspace, void *stream)
{
    (void)workspace;
    return token_spans_entry(x, CTC_AMD_F32, stride_t, stride_b, labels, labels_i64, nullptr, in_len, tgt_len, T, B, C, S, path,
                             score, nll, frame_conf, start, end, conf, stream);
}

extern "C" int ctc_amd_noblank_token_spans_typed(const void *x, int x_dtype, int64_t stride_t, int64_t stride_b,
                                                 const void *labels, int labels_i64,
                                                 const int64_t *in_len, const int64_t *tgt_len,
                                                 int T, int B, int C, int S,
                                                 int32_t *path, float *score, float *nll, float *frame_conf,
                                                 int32_t *start, int32_t *end, float *conf,
                                                 void *workspace, void *stream)
{
    (void)workspace;
    return token_spans_entry(x, x_dtype, stride_t, stride_b, labels, labels_i64, nullptr, in_len, tgt_len, T, B, C, S, path,
                             score, nll, frame_conf, start, end, conf, stream);
}

extern "C" int ctc_amd_binary_token_spans(const float *x, int64_t stride_t, int64_t stride_b, const float *y,
                                          const int64_t *in_len, const int64_t *tgt_len,
                                          int T, int B, int C, int S,
                                          int32_t *path, float *score, float *nll, float *frame_conf,
                                          int32_t *start, int32_t *end, float *conf,
                                          void *workspace, void *stream)
{
    (void)workspace;
    return token_spans_entry(x, CTC_AMD_F32, stride_t, stride_b, nullptr, 0, y, in_len, tgt_len, T, B, C, S, path, score, nll,
                             frame_conf, start, end, conf, stream);
}

extern "C" int ctc_amd_binary_token_spans_typed(const void *x, int x_dtype, int64_t stride_t, int64_t stride_b, const float *y,
                                                const int64_t *in_len, const int64_t *tgt_len,
                                                int T, int B, int C, int S,
                                                int32_t *path, float *score, float *nll, float *frame_conf,
                                                int32_t *start, int32_t *end, float *conf,
                                                void *workspace, void *stream)
{
    (void)workspace;
    return token_spans_entry(x, x_dtype, stride_t, stride_b, nullptr, 0, y, in_len, tgt_len, T, B, C, S, path, score, nll,
                             frame_conf, start, end, conf, stream);
}
