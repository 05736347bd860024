// The step immediately upstream of the loss: the reference's LSTM_cell.forward (LSTM.py:39-51) runs
//     for time in range(temporal):  v = self.v(feat[time]);  v_hsn, v_csn = self.v_cell(v, (v_hsn, v_csn));
//                                   v_series[time] = v_hsn
// i.e. one torch.nn.LSTMCell step per frame whose hidden state IS the logits row the CTC losses read.  This file
// is that step as ONE launch: both gate products, the cell update, and the hidden state written straight into
// v_series[time] -- in the row layout the loss kernels want (unit stride over classes, any row pitch; pad columns
// behind the last class filled with a value of the caller's choice: a pitch of C + 1 with -1e30 there turns an
// odd class count (the reference's 33) into the even, 8-byte aligned rows of the four-rows-per-wave loss kernel
// without changing a single loss or gradient value -- softmax gives that column exactly 0).
//
// torch.nn.LSTMCell semantics:  gates = x W_ih^T + b_ih + h W_hh^T + b_hh, chunks (i, f, g, o) of H rows each;
//     i, f, o = sigmoid, g = tanh;   c' = f c + i g;   h' = o tanh(c').
//
// Small and latency-bound at the reference's sizes (B = 10, H = 33: 17 kFLOP per step) and still small at the
// benchmark's (B = 256, H = 158: 0.1 GFLOP): one workgroup per kLstmSamples samples stages [x | h] in LDS, every
// thread owns gate rows r = tid, tid + 256, ... of [W_ih | W_hh] and walks them once for all staged samples (the
// weights, <= 0.8 MB, stay in L2; the staged inputs are LDS broadcasts), the pre-activations meet in LDS and one
// thread per hidden unit finishes the cell.  fp32 fma chains in k order (W_ih part, then W_hh part, then the biases).
#include "common.hpp"
#include "launch.hpp"

namespace ctc {

constexpr int kLstmSamples = 8, kLstmThreads = 256;

struct LstmParams {
    const float *x, *h, *c, *w_ih, *w_hh, *b_ih, *b_hh;
    int B, I, H;
    float *h_out, *c_out, *gates;                            // gates: optional [B][4H] activations (i, f, g, o)
    float *series;                                           // optional: row b at series + b * series_stride_b
    int64_t series_stride_b;
    int series_cols;                                         // columns [H, series_cols) of a row get pad_value
    float pad_value;
};

__device__ __forceinline__ float sigmoid_f(float v) { return 1.0f / (1.0f + __expf(-v)); }

__global__ __launch_bounds__(kLstmThreads) void lstm_cell_step_kernel(LstmParams p)
{
    extern __shared__ float lstm_smem[];
    const int K = p.I + p.H, G = 4 * p.H;
    float *xh = lstm_smem;                                   // [kLstmSamples][K]
    float *pre = xh + kLstmSamples * K;                      // [kLstmSamples][G]
    const int tid = threadIdx.x, b0 = blockIdx.x * kLstmSamples;
    const int ns = min(kLstmSamples, p.B - b0);
    for (int i = tid; i < kLstmSamples * K; i += kLstmThreads) {
        const int s = i / K, k = i - s * K;
        float v = 0.f;
        if (s < ns) v = k < p.I ? p.x[(size_t)(b0 + s) * p.I + k] : p.h[(size_t)(b0 + s) * p.H + (k - p.I)];
        xh[i] = v;
    }
    __syncthreads();
    for (int r = tid; r < G; r += kLstmThreads) {
        float acc[kLstmSamples];
#pragma unroll
        for (int s = 0; s < kLstmSamples; ++s) acc[s] = 0.f;
        const float *wi = p.w_ih + (size_t)r * p.I, *wh = p.w_hh + (size_t)r * p.H;
#pragma unroll 4
        for (int k = 0; k < p.I; ++k) {
            const float w = wi[k];
#pragma unroll
            for (int s = 0; s < kLstmSamples; ++s) acc[s] = __builtin_fmaf(w, xh[s * K + k], acc[s]);
        }
#pragma unroll 4
        for (int k = 0; k < p.H; ++k) {
            const float w = wh[k];
#pragma unroll
            for (int s = 0; s < kLstmSamples; ++s) acc[s] = __builtin_fmaf(w, xh[s * K + p.I + k], acc[s]);
        }
        const float bias = p.b_ih[r] + p.b_hh[r];
#pragma unroll
        for (int s = 0; s < kLstmSamples; ++s) pre[s * G + r] = acc[s] + bias;
    }
    __syncthreads();
    for (int i = tid; i < ns * p.H; i += kLstmThreads) {
        const int s = i / p.H, j = i - s * p.H, b = b0 + s;
        const float *g4 = pre + s * G;
        const float gi = sigmoid_f(g4[j]), gf = sigmoid_f(g4[p.H + j]), gg = tanhf(g4[2 * p.H + j]), go = sigmoid_f(g4[3 * p.H + j]);
        const float cn = __builtin_fmaf(gf, p.c[(size_t)b * p.H + j], gi * gg);
        const float hn = go * tanhf(cn);
        p.c_out[(size_t)b * p.H + j] = cn;
        p.h_out[(size_t)b * p.H + j] = hn;
        if (p.series) p.series[b * p.series_stride_b + j] = hn;
        if (p.gates) {
            float *q = p.gates + (size_t)b * G;
            q[j] = gi; q[p.H + j] = gf; q[2 * p.H + j] = gg; q[3 * p.H + j] = go;
        }
    }
    if (p.series && p.series_cols > p.H) {
        const int np = p.series_cols - p.H;
        for (int i = tid; i < ns * np; i += kLstmThreads) {
            const int s = i / np, j = p.H + (i - s * np);
            p.series[(b0 + s) * p.series_stride_b + j] = p.pad_value;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// The whole recurrence of LSTM_cell.forward as ONE launch (the reference's class counts, 33 / 38: I + H <= kSeriesK).
// One 256-thread workgroup per kSeriesSamples samples walks all T frames: thread r holds gate row r of [W_ih | W_hh] in
// REGISTERS for the whole launch, [x_t | h_{t-1}] of the samples sits in LDS (16-byte broadcast reads), the cell state
// stays in LDS between frames, x_{t+1} is in flight while frame t is computed, and h_t goes straight into v_series[t].
// Same fma chains, in the same order, as lstm_cell_step_kernel: the two paths agree bit for bit.  Two barriers per frame.
constexpr int kSeriesSamples = 4, kSeriesK = 80;

struct LstmSeriesParams {
    const float *x, *h0, *c0, *w_ih, *w_hh, *b_ih, *b_hh;
    int T, B, I, H;
    float *series;
    int64_t series_stride_t, series_stride_b;
    int series_cols;
    float pad_value;
    float *gates, *cells;                                    // optional [T][B][4H] activations, [T + 1][B][H] cell states (backward)
    float *h_out, *c_out;                                    // optional final state [B][H]
};

// the parameter block of every forward recurrence (narrow, wide, fused), in the order of the entries' argument lists
inline LstmSeriesParams series_params(const float *x, const float *h0, const float *c0,
                                      const float *w_ih, const float *w_hh, const float *b_ih, const float *b_hh,
                                      int T, int B, int I, int H,
                                      float *series, int64_t series_stride_t, int64_t series_stride_b, int series_cols, float pad_value,
                                      float *gates, float *cells, float *h_out, float *c_out)
{
    return LstmSeriesParams{x, h0, c0, w_ih, w_hh, b_ih, b_hh, T, B, I, H, series, series_stride_t, series_stride_b,
                            series_cols, pad_value, gates, cells, h_out, c_out};
}

// What a thread of the recurrence owns, and where the workgroup's staging lies in LDS (lstm_series_kernel and
// lstm_forward_kernel: one layout, one prologue, one frame body -- the same fma chains in both, bit for bit).
struct SeriesLane {
    float *xh, *pre, *cst;                                   // [kSeriesSamples][4 * K4]: [x_t | h_{t-1} | zeros]; [kSeriesSamples][G]; [kSeriesSamples][H]
    int K4, G, tid, b0, ns;
    int xs, xk, cs, cj;                                      // this thread's element of the next frame's inputs; its (sample, unit) of the cell update
    bool xmine, cmine;
};

__host__ __device__ inline size_t series_smem_floats(int I, int H)
{
    return (size_t)kSeriesSamples * (4 * (size_t)((I + H + 3) / 4) + 4 * (size_t)H + H);
}

__device__ __forceinline__ SeriesLane series_lane(const LstmSeriesParams &p, float *smem)
{
    SeriesLane L;
    L.K4 = (p.I + p.H + 3) >> 2; L.G = 4 * p.H;
    L.xh = smem;
    L.pre = L.xh + kSeriesSamples * 4 * L.K4;
    L.cst = L.pre + kSeriesSamples * L.G;
    L.tid = threadIdx.x; L.b0 = blockIdx.x * kSeriesSamples;
    L.ns = min(kSeriesSamples, p.B - L.b0);
    // (kSeriesSamples * I <= 256 and kSeriesSamples * H <= 256 are checked on the host)
    L.xs = L.tid / p.I; L.xk = L.tid - L.xs * p.I;
    L.xmine = L.xs < L.ns && L.tid < kSeriesSamples * p.I;
    L.cs = L.tid / p.H; L.cj = L.tid - L.cs * p.H;
    L.cmine = L.cs < L.ns && L.tid < kSeriesSamples * p.H;
    return L;
}

// gate row `tid` of [W_ih | W_hh] -> registers (zeros behind K: the staged vectors are padded alike)
__device__ __forceinline__ void series_gate_row(const LstmSeriesParams &p, const SeriesLane &L, float (&wr)[kSeriesK], float &bias)
{
    const int K = p.I + p.H;
    bias = 0.f;
    if (L.tid < L.G) {
#pragma unroll
        for (int k = 0; k < kSeriesK; ++k)
            wr[k] = k < p.I ? p.w_ih[(size_t)L.tid * p.I + k] : k < K ? p.w_hh[(size_t)L.tid * p.H + (k - p.I)] : 0.f;
        bias = p.b_ih[L.tid] + p.b_hh[L.tid];
    }
}

// [x_0 | h_0 | zeros] and c_0 of the workgroup's samples -> LDS; x0(s, k): element k of sample s's input of frame 0
template <typename X0>
__device__ __forceinline__ void series_stage(const LstmSeriesParams &p, const SeriesLane &L, X0 x0)
{
    const int K = p.I + p.H, K4 = L.K4;
    for (int i = L.tid; i < kSeriesSamples * 4 * K4; i += kLstmThreads) {
        const int s = i / (4 * K4), k = i - s * 4 * K4;
        float v = 0.f;
        if (s < L.ns && k < p.I) v = x0(s, k);
        else if (s < L.ns && k < K) v = p.h0[(size_t)(L.b0 + s) * p.H + (k - p.I)];
        L.xh[i] = v;
    }
    for (int i = L.tid; i < kSeriesSamples * p.H; i += kLstmThreads) {
        const int s = i / p.H, j = i - s * p.H;
        const float c = s < L.ns ? p.c0[(size_t)(L.b0 + s) * p.H + j] : 0.f;
        L.cst[i] = c;
        if (p.cells && s < L.ns) p.cells[(size_t)(L.b0 + s) * p.H + j] = c;
    }
}

// Frame t behind its first barrier ([x_t | h_{t-1}] is complete; the caller has x_{t+1} in flight as `xnext`): the gate
// products, the second barrier, the cell update, h_t into LDS and into v_series[t].
__device__ __forceinline__ void series_frame(const LstmSeriesParams &p, const SeriesLane &L, const float (&wr)[kSeriesK],
                                             float bias, int t, float xnext)
{
    const int K4 = L.K4, G = L.G, tid = L.tid, cs_ = L.cs, cj = L.cj;
    float *xh = L.xh, *pre = L.pre, *cst = L.cst;
    if (tid < G) {
        float acc[kSeriesSamples];
#pragma unroll
        for (int s = 0; s < kSeriesSamples; ++s) acc[s] = 0.f;
#pragma unroll
        for (int k4 = 0; k4 < kSeriesK / 4; ++k4) {
            if (k4 < K4) {                                   // (uniform)
#pragma unroll
                for (int s = 0; s < kSeriesSamples; ++s) {
                    const float4 v = *reinterpret_cast<const float4 *>(xh + (s * K4 + k4) * 4);
                    acc[s] = __builtin_fmaf(wr[4 * k4], v.x, acc[s]);
                    acc[s] = __builtin_fmaf(wr[4 * k4 + 1], v.y, acc[s]);
                    acc[s] = __builtin_fmaf(wr[4 * k4 + 2], v.z, acc[s]);
                    acc[s] = __builtin_fmaf(wr[4 * k4 + 3], v.w, acc[s]);
                }
            }
        }
#pragma unroll
        for (int s = 0; s < kSeriesSamples; ++s) pre[s * G + tid] = acc[s] + bias;
    }
    __syncthreads();                                         // the pre-activations are there; the staged vectors are free
    if (L.xmine) xh[L.xs * 4 * K4 + L.xk] = xnext;
    if (L.cmine) {
        const int b = L.b0 + cs_;
        const float *g4 = pre + cs_ * G;
        const float gi = sigmoid_f(g4[cj]), gf = sigmoid_f(g4[p.H + cj]), gg = tanhf(g4[2 * p.H + cj]), go = sigmoid_f(g4[3 * p.H + cj]);
        const float cn = __builtin_fmaf(gf, cst[cs_ * p.H + cj], gi * gg);
        const float hn = go * tanhf(cn);
        cst[cs_ * p.H + cj] = cn;
        xh[cs_ * 4 * K4 + p.I + cj] = hn;                    // h_t: the next frame's recurrent input
        p.series[t * p.series_stride_t + b * p.series_stride_b + cj] = hn;
        if (p.gates) {
            float *q = p.gates + ((size_t)t * p.B + b) * G;
            q[cj] = gi; q[p.H + cj] = gf; q[2 * p.H + cj] = gg; q[3 * p.H + cj] = go;
        }
        if (p.cells) p.cells[((size_t)(t + 1) * p.B + b) * p.H + cj] = cn;
        if (t == p.T - 1) {
            if (p.h_out) p.h_out[(size_t)b * p.H + cj] = hn;
            if (p.c_out) p.c_out[(size_t)b * p.H + cj] = cn;
        }
    }
    if (p.series_cols > p.H) {
        const int np = p.series_cols - p.H;
        for (int i = tid; i < L.ns * np; i += kLstmThreads) {
            const int s = i / np, j = p.H + (i - s * np);
            p.series[t * p.series_stride_t + (L.b0 + s) * p.series_stride_b + j] = p.pad_value;
        }
    }
}

__global__ __launch_bounds__(kLstmThreads) void lstm_series_kernel(LstmSeriesParams p)
{
    extern __shared__ float4 series_smem[];
    const SeriesLane L = series_lane(p, reinterpret_cast<float *>(series_smem));
    float wr[kSeriesK];
    float bias;
    series_gate_row(p, L, wr, bias);
    series_stage(p, L, [&](int s, int k) { return p.x[(size_t)(L.b0 + s) * p.I + k]; });
    for (int t = 0; t < p.T; ++t) {
        __syncthreads();                                     // [x_t | h_{t-1}] is complete
        float xnext = 0.f;
        if (L.xmine && t + 1 < p.T) xnext = p.x[((size_t)(t + 1) * p.B + L.b0 + L.xs) * p.I + L.xk];
        series_frame(p, L, wr, bias, t, xnext);
    }
}

// The backward recurrence of the same loop as one launch.  Only what is SEQUENTIAL stays in the kernel: thread (s, j) owns
// hidden unit j of sample s for all T frames -- dh and dc live in its registers -- turns (dh_t, dc_t) into the four
// pre-activation gradients of its unit (written out: [T][B][4H]), and takes dh_{t-1}(s, j) = sum_r W_hh[r][j] dpre(s, r) with
// column j of W_hh in registers and the pre-activation gradients of the sample's 4H gate rows read from LDS (16-byte
// broadcasts, double-buffered: one barrier per frame).  Everything that is not a recurrence -- dx_t = dpre_t W_ih, the three
// parameter gradients -- runs over all frames at once on the result: lstm_bwd_products_kernel behind this launch in
// ctc_amd_lstm_backward (below), or GEMMs of the caller's (ctc_amd_lstm_series_backward alone: rocBLAS through torch).
constexpr int kSeriesG = 4 * 64;

struct LstmSeriesBwdParams {
    const float *d_series;                                   // upstream gradient of v_series, unit stride over classes
    int64_t ds_stride_t, ds_stride_b;
    const float *gates, *cells, *w_hh;                       // [T][B][4H] (i, f, g, o), [T + 1][B][H], [4H][H]
    int T, B, H;
    float *dpre, *dh0, *dc0;                                 // [T][B][4H], [B][H], [B][H]
};

// the parameter block of both backward recurrences (narrow, wide), in the order of the entries' argument lists
inline LstmSeriesBwdParams series_bwd_params(const float *d_series, int64_t ds_stride_t, int64_t ds_stride_b,
                                             const float *gates, const float *cells, const float *w_hh,
                                             int T, int B, int H, float *dpre, float *dh0, float *dc0)
{
    return LstmSeriesBwdParams{d_series, ds_stride_t, ds_stride_b, gates, cells, w_hh, T, B, H, dpre, dh0, dc0};
}

__global__ __launch_bounds__(kLstmThreads) void lstm_series_bwd_kernel(LstmSeriesBwdParams p)
{
    extern __shared__ float4 bwd_smem[];
    const int G = 4 * p.H, G4 = p.H;                         // (G floats = H float4)
    float *dp = reinterpret_cast<float *>(bwd_smem);         // [2][kSeriesSamples][G]: the frame's pre-activation gradients
    const int tid = threadIdx.x, b0 = blockIdx.x * kSeriesSamples;
    const int ns = min(kSeriesSamples, p.B - b0);
    const int s = tid / p.H, j = tid - s * p.H;
    const bool mine = s < ns && tid < kSeriesSamples * p.H;
    const int b = b0 + (mine ? s : 0);
    float wc[kSeriesG];                                      // column j of W_hh
#pragma unroll
    for (int r = 0; r < kSeriesG; ++r) wc[r] = (mine && r < G) ? p.w_hh[(size_t)r * p.H + j] : 0.f;
    for (int i = tid; i < 2 * kSeriesSamples * G; i += kLstmThreads) dp[i] = 0.f;
    float dh = 0.f, dc = 0.f;                                // gradient arriving from frame t + 1
    // frame T - 1's operands (then always one frame ahead)
    auto fetch = [&](int t, float (&q)[4], float &ct, float &cp, float &ds) {
        const float *g = p.gates + ((size_t)t * p.B + b) * G;
        q[0] = g[j]; q[1] = g[p.H + j]; q[2] = g[2 * p.H + j]; q[3] = g[3 * p.H + j];
        ct = p.cells[((size_t)(t + 1) * p.B + b) * p.H + j];
        cp = p.cells[((size_t)t * p.B + b) * p.H + j];
        ds = p.d_series[t * p.ds_stride_t + b * p.ds_stride_b + j];
    };
    float q[4] = {0.f, 0.f, 0.f, 0.f}, ct = 0.f, cp = 0.f, ds = 0.f;
    if (mine) fetch(p.T - 1, q, ct, cp, ds);
    for (int t = p.T - 1; t >= 0; --t) {
        float *cur = dp + (size_t)(t & 1) * kSeriesSamples * G;
        float qn[4] = {0.f, 0.f, 0.f, 0.f}, ctn = 0.f, cpn = 0.f, dsn = 0.f;
        if (mine && t > 0) fetch(t - 1, qn, ctn, cpn, dsn);
        if (mine) {
            const float gi = q[0], gf = q[1], gg = q[2], go = q[3];
            const float dht = dh + ds;
            const float tc = tanhf(ct);
            const float dct = __builtin_fmaf(dht * go, 1.0f - tc * tc, dc);
            const float d_i = dct * gg * gi * (1.0f - gi);
            const float d_f = dct * cp * gf * (1.0f - gf);
            const float d_g = dct * gi * (1.0f - gg * gg);
            const float d_o = dht * tc * go * (1.0f - go);
            cur[s * G + j] = d_i; cur[s * G + p.H + j] = d_f; cur[s * G + 2 * p.H + j] = d_g; cur[s * G + 3 * p.H + j] = d_o;
            float *o = p.dpre + ((size_t)t * p.B + b) * G;
            o[j] = d_i; o[p.H + j] = d_f; o[2 * p.H + j] = d_g; o[3 * p.H + j] = d_o;
            dc = dct * gf;
        }
        __syncthreads();                                     // the frame's 4H pre-activation gradients of every sample are in LDS
        if (mine) {
            float acc = 0.f;
            const float4 *row = reinterpret_cast<const float4 *>(cur + s * G);
#pragma unroll
            for (int r4 = 0; r4 < kSeriesG / 4; ++r4) {
                if (r4 < G4) {                               // (uniform)
                    const float4 v = row[r4];
                    acc = __builtin_fmaf(wc[4 * r4], v.x, acc);
                    acc = __builtin_fmaf(wc[4 * r4 + 1], v.y, acc);
                    acc = __builtin_fmaf(wc[4 * r4 + 2], v.z, acc);
                    acc = __builtin_fmaf(wc[4 * r4 + 3], v.w, acc);
                }
            }
            dh = acc;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) q[k] = qn[k];
        ct = ctn; cp = cpn; ds = dsn;
    }
    if (mine) {
        p.dh0[(size_t)b * p.H + j] = dh;
        p.dc0[(size_t)b * p.H + j] = dc;
    }
}

}  // namespace ctc

using namespace ctc;

// The T steps of ctc_amd_lstm_cell_step as one launch, for the reference's class counts (I + H <= 80, H <= 64, I <= 64).
// Other sizes: CTC_AMD_ERR_UNSUPPORTED_SHAPE (ctc_amd_lstm_series_wide takes up to 160 classes, lstm_wide.hpp; beyond, the caller steps
// frame by frame).
extern "C" int ctc_amd_lstm_series(const float *x, const float *h0, const float *c0,
                                   const float *w_ih, const float *w_hh, const float *b_ih, const float *b_hh,
                                   int T, int B, int I, int H,
                                   float *series, int64_t series_stride_t, int64_t series_stride_b, int series_cols, float pad_value,
                                   float *gates_out, float *cells_out, float *h_out, float *c_out, void *stream)
{
    if (!x || !h0 || !c0 || !w_ih || !w_hh || !b_ih || !b_hh || !series) return CTC_AMD_ERR_BAD_ARGUMENT;
    if (T < 1 || B < 1 || I < 1 || H < 1) return CTC_AMD_ERR_BAD_ARGUMENT;
    if (series_cols < H || series_stride_b < series_cols) return CTC_AMD_ERR_BAD_ARGUMENT;
    if (I + H > kSeriesK || 4 * H > kLstmThreads || kSeriesSamples * I > kLstmThreads || kSeriesSamples * H > kLstmThreads)
        return CTC_AMD_ERR_UNSUPPORTED_SHAPE;
    const LstmSeriesParams p = series_params(x, h0, c0, w_ih, w_hh, b_ih, b_hh, T, B, I, H, series, series_stride_t,
                                             series_stride_b, series_cols, pad_value, gates_out, cells_out, h_out, c_out);
    const size_t smem = series_smem_floats(I, H) * sizeof(float);
    return launch<lstm_series_kernel>(dim3((B + kSeriesSamples - 1) / kSeriesSamples), dim3(kLstmThreads), smem,
                                      static_cast<hipStream_t>(stream), p);
}

extern "C" int ctc_amd_lstm_cell_step(const float *x, const float *h, const float *c,
                                      const float *w_ih, const float *w_hh, const float *b_ih, const float *b_hh,
                                      int B, int I, int H,
                                      float *h_out, float *c_out, float *gates_out,
                                      float *series_row, int64_t series_stride_b, int series_cols, float pad_value,
                                      void *stream)
{
    if (!x || !h || !c || !w_ih || !w_hh || !b_ih || !b_hh || !h_out || !c_out) return CTC_AMD_ERR_BAD_ARGUMENT;
    if (B < 1 || I < 1 || H < 1) return CTC_AMD_ERR_BAD_ARGUMENT;
    if (series_row && (series_cols < H || series_stride_b < series_cols)) return CTC_AMD_ERR_BAD_ARGUMENT;
    const size_t smem = (size_t)kLstmSamples * ((size_t)I + H + 4 * (size_t)H) * sizeof(float);
    if (smem > kMaxLds) return CTC_AMD_ERR_UNSUPPORTED_SHAPE;
    LstmParams p;
    p.x = x; p.h = h; p.c = c; p.w_ih = w_ih; p.w_hh = w_hh; p.b_ih = b_ih; p.b_hh = b_hh;
    p.B = B; p.I = I; p.H = H;
    p.h_out = h_out; p.c_out = c_out; p.gates = gates_out;
    p.series = series_row; p.series_stride_b = series_stride_b; p.series_cols = series_cols; p.pad_value = pad_value;
    return launch<lstm_cell_step_kernel>(dim3((B + kLstmSamples - 1) / kLstmSamples), dim3(kLstmThreads), smem,
                                         static_cast<hipStream_t>(stream), p);
}


// The enqueue of lstm_series_bwd_kernel, shared by ctc_amd_lstm_series_backward and ctc_amd_lstm_backward (the callers have
// checked the arguments): one launch on `stream`.
static int enqueue_series_backward(const LstmSeriesBwdParams &p, hipStream_t stream)
{
    const size_t smem = (size_t)2 * kSeriesSamples * 4 * p.H * sizeof(float);
    return launch<lstm_series_bwd_kernel>(dim3((p.B + kSeriesSamples - 1) / kSeriesSamples), dim3(kLstmThreads), smem, stream, p);
}

// The backward recurrence of ctc_amd_lstm_series (same sizes): from the upstream gradient of v_series and the state the
// forward launch saved to the pre-activation gradients of every frame and the gradients of (h0, c0).  The rest of the
// backward pass has no recurrence in it: ctc_amd_lstm_backward (below) runs this launch and the products behind it.
extern "C" int ctc_amd_lstm_series_backward(const float *d_series, int64_t ds_stride_t, int64_t ds_stride_b,
                                            const float *gates, const float *cells, const float *w_hh,
                                            int T, int B, int H, float *dpre_out, float *dh0_out, float *dc0_out, void *stream)
{
    if (!d_series || !gates || !cells || !w_hh || !dpre_out || !dh0_out || !dc0_out) return CTC_AMD_ERR_BAD_ARGUMENT;
    if (T < 1 || B < 1 || H < 1) return CTC_AMD_ERR_BAD_ARGUMENT;
    if (4 * H > kSeriesG || kSeriesSamples * H > kLstmThreads) return CTC_AMD_ERR_UNSUPPORTED_SHAPE;
    return enqueue_series_backward(series_bwd_params(d_series, ds_stride_t, ds_stride_b, gates, cells, w_hh, T, B, H, dpre_out,
                                                     dh0_out, dc0_out),
                                   static_cast<hipStream_t>(stream));
}

// ---------------------------------------------------------------------------------------------------------------------
// The HEAD of the producer (LSTM.py:8-18, called per frame at :48): Linear(K -> C) + BatchNorm1d + ReLU +
// Dropout for ALL frames in one launch.  One workgroup per (frame, tile of 16 output columns); wave m owns batch rows
// 16 m .. 16 m + 15 (B <= 256 rows of one frame fit one workgroup, which is what BatchNorm's per-frame batch statistics
// need: a column's mean and variance are taken over the B rows of ONE frame, as the reference's per-frame calls do).
// The product runs on the matrix cores in exact fp32 (v_mfma_f32_16x16x4_f32, an fmaf chain per output): a lane loads
// 16 bytes of its feature row and 16 bytes of its weight row per four MFMAs -- the k index is permuted the same way on
// both operands (lane (r, q) holds k = 16 kb + 4 q + i for MFMA i), which a sum over k does not see.
// Train mode: batch statistics (two passes: mean, then the centred second moment, like torch), saved per (frame, column)
// for the backward pass and for the running statistics, which the reference updates frame after frame (a closed form
// over the T frames, applied by the caller).  Eval mode: the running statistics.  Dropout is a mask tensor the caller
// hands in (already scaled by 1 / (1 - p)): the random stream stays torch's.
namespace ctc {

constexpr int kHeadMaxBatch = 256;                           // B beyond this: the wide entries (head_wide.hpp)

struct HeadParams {
    const void *feat;                                        // [T][B][K] of the kernel's element type E (strides in elements)
    int64_t fst, fsb;
    const float *w, *bias, *gamma, *beta;                    // Linear [C][K], [C]; BatchNorm weight / bias [C]
    const float *rmean, *rvar;                               // eval mode: running statistics; NULL: batch statistics
    const float *mask;                                       // [T][B][C] or NULL
    float eps;
    int T, B, K, C;
    float *out;                                              // [T][B] rows of C at (ost, osb)
    int64_t ost, osb;
    float *lin, *smean, *svar, *sinv;                        // optional: Linear output [T][B][C]; batch mean / biased variance / 1/sqrt(var + eps) [T][C]
};

typedef float head_f4 __attribute__((ext_vector_type(4)));

// The FEATURE operand's element type E: float, or the 2-byte __bf16 / _Float16 of a backbone under autocast, read as
// it lies and widened to fp32 in registers -- bf16 by a 16-bit shift, fp16 by v_cvt_f32_f16 (exact, subnormals included: the
// conversion makes normal fp32 numbers of them).  Everything behind the widening is the fp32 kernel's own code, so a 2-byte
// launch gives the bits of the fp32 launch on feat.float().  Weights, statistics, the mask and every output stay fp32.
// head_feat4: four consecutive elements -> fp32 (float: one 16-byte load; 2-byte E: one 8-byte load)
template <typename E>
__device__ __forceinline__ head_f4 head_feat4(const E *p)
{
    if constexpr (__is_same(E, float)) {
        return *reinterpret_cast<const head_f4 *>(p);
    } else {
        typedef unsigned head_u2 __attribute__((ext_vector_type(2)));
        const head_u2 u = *reinterpret_cast<const head_u2 *>(p);
        if constexpr (__is_same(E, __bf16)) {
            const head_f4 f = {__builtin_bit_cast(float, u.x << 16), __builtin_bit_cast(float, u.x & 0xffff0000u),
                               __builtin_bit_cast(float, u.y << 16), __builtin_bit_cast(float, u.y & 0xffff0000u)};
            return f;
        } else {
            typedef _Float16 head_h4 __attribute__((ext_vector_type(4)));
            return __builtin_convertvector(__builtin_bit_cast(head_h4, u), head_f4);
        }
    }
}

// (feat_dtype of the typed entries -> E: with_logit_elem of launch.hpp)

// What every head entry, forward and backward, asks of its two matrix-core operands: 16-byte loads of fp32 feature rows, 8-byte
// loads of 2-byte rows (strides in elements), 16-byte loads of the weight rows, K a multiple of 16.
inline bool head_operands_ok(const void *feat, int feat_dtype, int64_t stride_t, int64_t stride_b, const float *weight, int K)
{
    const uintptr_t mask = feat_dtype == CTC_AMD_F32 ? 15 : 7;
    return (K & 15) == 0 && (stride_b & 3) == 0 && (stride_t & 3) == 0 && (reinterpret_cast<uintptr_t>(feat) & mask) == 0 &&
           (reinterpret_cast<uintptr_t>(weight) & 15) == 0;
}

inline bool head_dtype_ok(int feat_dtype) { return feat_dtype == CTC_AMD_F32 || feat_dtype == CTC_AMD_BF16 || feat_dtype == CTC_AMD_F16; }

// The arguments the three forward entries share (ctc_amd_head_forward_typed, ctc_amd_head_forward_wide_typed,
// ctc_amd_lstm_forward_typed) -> CTC_AMD_ERR_BAD_ARGUMENT, or `p` filled and the operands' answer: 0 or
// CTC_AMD_ERR_UNSUPPORTED_SHAPE.  A bad argument wins over the shape, so the caller runs its own argument checks before it acts on
// the second answer, and adds what is its own to the shape: the bound on B, the scratch, the recurrence's sizes.
inline int head_forward_params(HeadParams &p, const void *feat, int feat_dtype, int64_t feat_stride_t, int64_t feat_stride_b,
                               const float *weight, const float *bias, const float *bn_weight, const float *bn_bias,
                               const float *running_mean, const float *running_var, float eps, const float *mask,
                               int T, int B, int K, int C, float *out, int64_t out_stride_t, int64_t out_stride_b,
                               float *linear_out, float *save_mean, float *save_var, float *save_invstd)
{
    if (!head_dtype_ok(feat_dtype)) return CTC_AMD_ERR_BAD_ARGUMENT;
    if (!feat || !weight || !bias || !bn_weight || !bn_bias || !out) return CTC_AMD_ERR_BAD_ARGUMENT;
    if (T < 1 || B < 1 || K < 1 || C < 1 || (running_mean == nullptr) != (running_var == nullptr)) return CTC_AMD_ERR_BAD_ARGUMENT;
    if (out_stride_b < C) return CTC_AMD_ERR_BAD_ARGUMENT;
    if (running_mean == nullptr && B < 2) return CTC_AMD_ERR_BAD_ARGUMENT;       // (torch raises too: one value per channel)
    p.feat = feat; p.fst = feat_stride_t; p.fsb = feat_stride_b;
    p.w = weight; p.bias = bias; p.gamma = bn_weight; p.beta = bn_bias;
    p.rmean = running_mean; p.rvar = running_var; p.mask = mask; p.eps = eps;
    p.T = T; p.B = B; p.K = K; p.C = C;
    p.out = out; p.ost = out_stride_t; p.osb = out_stride_b;
    p.lin = linear_out; p.smean = save_mean; p.svar = save_var; p.sinv = save_invstd;
    return head_operands_ok(feat, feat_dtype, feat_stride_t, feat_stride_b, weight, K) ? 0 : CTC_AMD_ERR_UNSUPPORTED_SHAPE;
}

// The Linear product of one tile of 16 rows with N tiles of 16 columns (head_kernel: N = 1; lstm_forward_kernel: every
// column tile of a row tile).  ap / bp[n]: this lane's feature row / weight rows, already advanced by 4 fq.  Every output
// element is ONE fmaf chain over k in the order (kb, MFMA i, q) with k = 16 kb + 4 q + i, a zero second batch when the
// count of 16-blocks is odd: whoever calls this gets the same bits for the same row, column and K.
template <int N, typename E>
__device__ __forceinline__ void head_dot(const E *ap, const float *const (&bp)[N], int KB, head_f4 (&acc)[N])
{
    const head_f4 zero = {0.f, 0.f, 0.f, 0.f};
    for (int kb = 0; kb < KB; kb += 2) {                     // two batches of four MFMAs in flight (rows are 16-byte aligned, 8-byte for a 2-byte E: checked by the host)
        const bool two = kb + 1 < KB;
        const head_f4 a0 = head_feat4(ap + 16 * kb);
        const head_f4 a1 = two ? head_feat4(ap + 16 * kb + 16) : zero;
        head_f4 b0[N], b1[N];
#pragma unroll
        for (int n = 0; n < N; ++n) {
            b0[n] = *reinterpret_cast<const head_f4 *>(bp[n] + 16 * kb);
            b1[n] = two ? *reinterpret_cast<const head_f4 *>(bp[n] + 16 * kb + 16) : zero;
        }
#pragma unroll
        for (int n = 0; n < N; ++n) acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.x, b0[n].x, acc[n], 0, 0, 0);
#pragma unroll
        for (int n = 0; n < N; ++n) acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.y, b0[n].y, acc[n], 0, 0, 0);
#pragma unroll
        for (int n = 0; n < N; ++n) acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.z, b0[n].z, acc[n], 0, 0, 0);
#pragma unroll
        for (int n = 0; n < N; ++n) acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.w, b0[n].w, acc[n], 0, 0, 0);
#pragma unroll
        for (int n = 0; n < N; ++n) acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.x, b1[n].x, acc[n], 0, 0, 0);
#pragma unroll
        for (int n = 0; n < N; ++n) acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.y, b1[n].y, acc[n], 0, 0, 0);
#pragma unroll
        for (int n = 0; n < N; ++n) acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.z, b1[n].z, acc[n], 0, 0, 0);
#pragma unroll
        for (int n = 0; n < N; ++n) acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.w, b1[n].w, acc[n], 0, 0, 0);
    }
}

// The head's epilogue, piece by piece (one definition for both kernels: the same roundings in both)
__device__ __forceinline__ float head_linear(float acc, float bias) { return acc + bias; }
__device__ __forceinline__ float head_invstd(float var, float eps) { return 1.0f / sqrtf(var + eps); }
// BatchNorm's output, the value the ReLU tests (head_bn_relu here, the gate of the backward pass in head_bwd_rows_kernel:
// one expression, so the two agree bit for bit)
__device__ __forceinline__ float head_bn_y(float x, float mean, float inv, float g, float be) { return (x - mean) * inv * g + be; }
__device__ __forceinline__ float head_bn_relu(float x, float mean, float inv, float g, float be)
{
    const float y = head_bn_y(x, mean, inv, g, be);
    return y > 0.f ? y : 0.f;
}

// Sum over the batch rows of a frame for the 16 columns of a tile; every lane of a column gets it.  Lane (fr, fq) of wave w
// brings the partial sum of its four rows; red: [wave][column of the tile].  Fixed order: the lane quarters, then the waves.
__device__ __forceinline__ float head_column_total(float v, float (*red)[16], int w, int fr, int fq, int NW)
{
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    __syncthreads();                                         // (the previous total has been read by everybody)
    if (fq == 0) red[w][fr] = v;
    __syncthreads();
    float s = 0.f;
    for (int i = 0; i < NW; ++i) s += red[i][fr];
    return s;
}

template <typename E>
__global__ __launch_bounds__(1024) void head_kernel(HeadParams p)
{
    __shared__ float red[16][16];                            // [wave][column of the tile]
    const int t = blockIdx.x, n = blockIdx.y, tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    const int fr = lane & 15, fq = lane >> 4;
    const int NW = blockDim.x >> 6;
    // operands: A row = batch row 16 w + fr, B row = output column 16 n + fr (clamped: the padding is masked out below)
    const int arow = min(16 * w + fr, p.B - 1), bcol = min(16 * n + fr, p.C - 1);
    const E *ap = static_cast<const E *>(p.feat) + (int64_t)t * p.fst + (int64_t)arow * p.fsb + 4 * fq;
    const float *bp = p.w + (int64_t)bcol * p.K + 4 * fq;
    const float *bps[1] = {bp};
    head_f4 accs[1] = {{0.f, 0.f, 0.f, 0.f}};
    head_dot<1>(ap, bps, p.K >> 4, accs);                    // K is a multiple of 16 (checked by the host)
    const head_f4 acc = accs[0];
    // acc[j] = Linear output (without bias) of batch row 16 w + 4 fq + j, column 16 n + fr
    const int col = 16 * n + fr;
    const bool colok = col < p.C;
    const float bias = colok ? p.bias[col] : 0.f;
    float x[4];
    bool rowok[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        rowok[j] = 16 * w + 4 * fq + j < p.B;
        x[j] = head_linear(acc[j], bias);
    }
    auto column_total = [&](float v) { return head_column_total(v, red, w, fr, fq, NW); };
    float mean, inv;
    if (p.rmean) {                                           // eval mode
        mean = colok ? p.rmean[col] : 0.f;
        inv = head_invstd(colok ? p.rvar[col] : 1.f, p.eps);
    } else {
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) s += rowok[j] ? x[j] : 0.f;
        mean = column_total(s) / (float)p.B;
        float q = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) q += rowok[j] ? (x[j] - mean) * (x[j] - mean) : 0.f;
        const float var = column_total(q) / (float)p.B;      // biased, what the normalisation uses
        inv = head_invstd(var, p.eps);
        if (w == 0 && fq == 0 && colok) {
            if (p.smean) p.smean[(int64_t)t * p.C + col] = mean;
            if (p.svar) p.svar[(int64_t)t * p.C + col] = var;
            if (p.sinv) p.sinv[(int64_t)t * p.C + col] = inv;
        }
    }
    const float g = colok ? p.gamma[col] : 0.f, be = colok ? p.beta[col] : 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int b = 16 * w + 4 * fq + j;
        if (!rowok[j] || !colok) continue;
        if (p.lin) p.lin[((int64_t)t * p.B + b) * p.C + col] = x[j];
        float y = head_bn_relu(x[j], mean, inv, g, be);
        if (p.mask) y *= p.mask[((int64_t)t * p.B + b) * p.C + col];
        p.out[(int64_t)t * p.ost + (int64_t)b * p.osb + col] = y;
    }
}

}  // namespace ctc

extern "C" int ctc_amd_head_forward_typed(const void *feat, int feat_dtype, int64_t feat_stride_t, int64_t feat_stride_b,
                                          const float *weight, const float *bias, const float *bn_weight, const float *bn_bias,
                                          const float *running_mean, const float *running_var, float eps, const float *mask,
                                          int T, int B, int K, int C,
                                          float *out, int64_t out_stride_t, int64_t out_stride_b,
                                          float *linear_out, float *save_mean, float *save_var, float *save_invstd, void *stream)
{
    ctc::HeadParams p;
    const int rc = ctc::head_forward_params(p, feat, feat_dtype, feat_stride_t, feat_stride_b, weight, bias, bn_weight, bn_bias,
                                            running_mean, running_var, eps, mask, T, B, K, C, out, out_stride_t, out_stride_b,
                                            linear_out, save_mean, save_var, save_invstd);
    if (rc == CTC_AMD_ERR_BAD_ARGUMENT) return rc;
    // one workgroup holds the B rows of a frame (BatchNorm's statistics)
    if (rc || B > ctc::kHeadMaxBatch) return CTC_AMD_ERR_UNSUPPORTED_SHAPE;
    return ctc::with_logit_elem(feat_dtype, [&](auto e) {
        using E = typename decltype(e)::type;
        return launch<ctc::head_kernel<E>>(dim3(T, (C + 15) / 16), dim3(64 * ((B + 15) / 16)), 0, static_cast<hipStream_t>(stream), p);
    });
}

extern "C" int ctc_amd_head_forward(const float *feat, int64_t feat_stride_t, int64_t feat_stride_b,
                                    const float *weight, const float *bias, const float *bn_weight, const float *bn_bias,
                                    const float *running_mean, const float *running_var, float eps, const float *mask,
                                    int T, int B, int K, int C,
                                    float *out, int64_t out_stride_t, int64_t out_stride_b,
                                    float *linear_out, float *save_mean, float *save_var, float *save_invstd, void *stream)
{
    return ctc_amd_head_forward_typed(feat, CTC_AMD_F32, feat_stride_t, feat_stride_b, weight, bias, bn_weight, bn_bias,
                                      running_mean, running_var, eps, mask, T, B, K, C, out, out_stride_t, out_stride_b,
                                      linear_out, save_mean, save_var, save_invstd, stream);
}

// ---------------------------------------------------------------------------------------------------------------------
// EVAL mode: head and recurrence as ONE launch (feat -> v_series).  BatchNorm on its running statistics
// makes a sample's head rows independent of every other sample, so the workgroup that walks kSeriesSamples samples
// through the T frames (lstm_series_kernel's split, unchanged) first computes the head of exactly those samples:
//   phase 1: rows (frame t, sample s) -> 16 x 16 tiles on the matrix cores, A row 4 t + s; wave w takes row tiles
//            w, w + 4, ... and every column tile of them (the feature rows are loaded once, N = ceil(C / 16) <= 3
//            independent accumulator chains); bias, BatchNorm, ReLU; the result stays in LDS as [T][4][C];
//   phase 2: lstm_series_kernel's loop, x_t read from that slice.
// head_dot / head_linear / head_invstd / head_bn_relu and series_stage / series_frame are the two-launch path's own
// code: v_series is bit-identical to ctc_amd_head_forward + ctc_amd_lstm_series.
namespace ctc {

struct LstmForwardParams {
    HeadParams h;                                            // feat, strides, Linear, BatchNorm, running statistics, eps, T, B, K, C (the rest unused)
    LstmSeriesParams s;                                      // I = H = C; x unused
};

template <int N, typename E>
__device__ __forceinline__ void forward_head_phase(const HeadParams &p, float *vall, int b0, int ns)
{
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, fr = lane & 15, fq = lane >> 4;
    const int RT = (kSeriesSamples * p.T + 15) >> 4;         // row tiles of the workgroup's [T][4] rows
    const float *bp[N];
    float bias[N], mean[N], inv[N], g[N], be[N];
#pragma unroll
    for (int n = 0; n < N; ++n) {                            // (columns past C: clamped, never stored)
        const int col = min(16 * n + fr, p.C - 1);
        bp[n] = p.w + (int64_t)col * p.K + 4 * fq;
        bias[n] = p.bias[col];
        mean[n] = p.rmean[col];
        inv[n] = head_invstd(p.rvar[col], p.eps);
        g[n] = p.gamma[col];
        be[n] = p.beta[col];
    }
    for (int rt = w; rt < RT; rt += kLstmThreads / 64) {
        // A row 16 rt + fr = (frame, sample), clamped like arow / bcol of head_kernel: rows past the count are masked below
        const int row = 16 * rt + fr;
        const int t = min(row / kSeriesSamples, p.T - 1), s = min(row % kSeriesSamples, ns - 1);
        const E *ap = static_cast<const E *>(p.feat) + (int64_t)t * p.fst + (int64_t)(b0 + s) * p.fsb + 4 * fq;
        head_f4 acc[N];
#pragma unroll
        for (int n = 0; n < N; ++n) acc[n] = head_f4{0.f, 0.f, 0.f, 0.f};
        head_dot<N>(ap, bp, p.K >> 4, acc);
        // acc[n][j] = row 16 rt + 4 fq + j = (frame 4 rt + fq, sample j), column 16 n + fr
        const int to = 4 * rt + fq;
        if (to >= p.T) continue;
#pragma unroll
        for (int n = 0; n < N; ++n) {
            const int col = 16 * n + fr;
#pragma unroll
            for (int j = 0; j < kSeriesSamples; ++j)
                if (col < p.C && j < ns)
                    vall[((size_t)to * kSeriesSamples + j) * p.C + col] =
                        head_bn_relu(head_linear(acc[n][j], bias[n]), mean[n], inv[n], g[n], be[n]);
        }
    }
}

template <typename E>
__global__ __launch_bounds__(kLstmThreads) void lstm_forward_kernel(LstmForwardParams q)
{
    static_assert(kSeriesSamples == 4, "a 16-row tile holds four frames of the workgroup's samples");
    extern __shared__ float4 forward_smem[];
    const LstmSeriesParams &p = q.s;
    float *smem = reinterpret_cast<float *>(forward_smem);
    const SeriesLane L = series_lane(p, smem);
    float *vall = smem + series_smem_floats(p.I, p.H);       // [T][kSeriesSamples][C]: this workgroup's slice of the head's output
    const int C = q.h.C, CT = (C + 15) >> 4;                 // (2 C <= kSeriesK: at most three column tiles)
    if (CT == 1) forward_head_phase<1, E>(q.h, vall, L.b0, L.ns);
    else if (CT == 2) forward_head_phase<2, E>(q.h, vall, L.b0, L.ns);
    else forward_head_phase<3, E>(q.h, vall, L.b0, L.ns);
    float wr[kSeriesK];
    float bias;
    series_gate_row(p, L, wr, bias);
    __syncthreads();                                         // the slice is complete
    series_stage(p, L, [&](int s, int k) { return vall[s * C + k]; });
    for (int t = 0; t < p.T; ++t) {
        __syncthreads();                                     // [x_t | h_{t-1}] is complete
        float xnext = 0.f;
        if (L.xmine && t + 1 < p.T) xnext = vall[((size_t)(t + 1) * kSeriesSamples + L.xs) * C + L.xk];
        series_frame(p, L, wr, bias, t, xnext);
    }
}

}  // namespace ctc

extern "C" int ctc_amd_lstm_forward_typed(const void *feat, int feat_dtype, int64_t feat_stride_t, int64_t feat_stride_b,
                                          const float *weight, const float *bias, const float *bn_weight, const float *bn_bias,
                                          const float *running_mean, const float *running_var, float eps,
                                          const float *h0, const float *c0,
                                          const float *w_ih, const float *w_hh, const float *b_ih, const float *b_hh,
                                          int T, int B, int K, int C,
                                          float *series, int64_t series_stride_t, int64_t series_stride_b, int series_cols,
                                          float pad_value, float *h_out, float *c_out, void *stream)
{
    ctc::LstmForwardParams q{};
    // the head of the launch: no mask, nothing saved, and its "out" is the LDS slice -- the series stands in for the checks
    const int rc = ctc::head_forward_params(q.h, feat, feat_dtype, feat_stride_t, feat_stride_b, weight, bias, bn_weight, bn_bias,
                                            running_mean, running_var, eps, nullptr, T, B, K, C, series, series_stride_t,
                                            series_stride_b, nullptr, nullptr, nullptr, nullptr);
    if (rc == CTC_AMD_ERR_BAD_ARGUMENT) return rc;
    if (!running_mean || !h0 || !c0 || !w_ih || !w_hh || !b_ih || !b_hh) return CTC_AMD_ERR_BAD_ARGUMENT;        // eval mode only
    if (series_cols < C || series_stride_b < series_cols) return CTC_AMD_ERR_BAD_ARGUMENT;
    // the recurrence's sizes (I = H = C)
    if (rc || 2 * C > kSeriesK || 4 * C > kLstmThreads) return CTC_AMD_ERR_UNSUPPORTED_SHAPE;
    // the workgroup's slice of the head's output, [T][4][C], next to the recurrence's staging
    const size_t smem = (series_smem_floats(C, C) + (size_t)kSeriesSamples * (size_t)T * (size_t)C) * sizeof(float);
    if (smem > kMaxLds) return CTC_AMD_ERR_UNSUPPORTED_SHAPE;
    q.s = ctc::series_params(nullptr, h0, c0, w_ih, w_hh, b_ih, b_hh, T, B, C, C, series, series_stride_t, series_stride_b,
                             series_cols, pad_value, nullptr, nullptr, h_out, c_out);
    return ctc::with_logit_elem(feat_dtype, [&](auto e) {
        using E = typename decltype(e)::type;
        return launch<lstm_forward_kernel<E>>(dim3((B + kSeriesSamples - 1) / kSeriesSamples), dim3(kLstmThreads), smem,
                                              static_cast<hipStream_t>(stream), q);
    });
}

extern "C" int ctc_amd_lstm_forward(const float *feat, int64_t feat_stride_t, int64_t feat_stride_b,
                                    const float *weight, const float *bias, const float *bn_weight, const float *bn_bias,
                                    const float *running_mean, const float *running_var, float eps,
                                    const float *h0, const float *c0,
                                    const float *w_ih, const float *w_hh, const float *b_ih, const float *b_hh,
                                    int T, int B, int K, int C,
                                    float *series, int64_t series_stride_t, int64_t series_stride_b, int series_cols, float pad_value,
                                    float *h_out, float *c_out, void *stream)
{
    return ctc_amd_lstm_forward_typed(feat, CTC_AMD_F32, feat_stride_t, feat_stride_b, weight, bias, bn_weight, bn_bias,
                                      running_mean, running_var, eps, h0, c0, w_ih, w_hh, b_ih, b_hh, T, B, K, C,
                                      series, series_stride_t, series_stride_b, series_cols, pad_value, h_out, c_out, stream);
}

// ---------------------------------------------------------------------------------------------------------------------
// The BACKWARD of the head: from the upstream gradient of the head's output and what the forward launch saved
// to the gradients of feat, the Linear layer and BatchNorm's affine parameters.  Two launches (three when the weight
// gradient splits its row range), data handed on at the kernel boundaries only:
//   rows      grid (T, ceil(C / 16)), head_kernel's tiling: lane (fr, fq) of wave w owns batch rows 16 w + 4 fq + j of
//             column 16 n + fr -- dy, xhat, the per-frame column totals (head_column_total), dlin [T B][CP] (CP = C padded
//             to a multiple of 16, the pad zero) and the per-frame partials dbeta_t, dgamma_t, sum_b dlin [3][T][CP];
//   products  one wave per task, exact fp32 on the matrix cores (an fmaf chain per output element):
//               d_weight tile [16 c x 64 k] of one row-range split, contracting over the rows (4-byte operand loads, 64
//                 contiguous bytes per 16 lanes);
//               d_feat tile [16 rows x 64 k], contracting over the padded C (16-byte loads of the dlin row);
//               tail: the [T][CP] partials summed over t ascending;
//   reduce    (S > 1 only) the S partial weight gradients added in ascending split order.
// S and the rows per split are functions of T B alone (head_bwd_splits): the same shape sums in the same order.
namespace ctc {

constexpr int64_t kHeadBwdMaxRows = (int64_t)1 << 22;        // T B beyond this: CTC_AMD_ERR_UNSUPPORTED_SHAPE
constexpr int64_t kHeadBwdMaxTasks = (int64_t)1 << 28;       // waves of the products launch
constexpr int kHeadBwdSplitRows = 128, kHeadBwdMaxSplits = 64;
constexpr size_t kHeadBwdAlign = 256;                        // every piece of the scratch starts on such a boundary

// row-range splits of the weight gradient: S = min(64, ceil(R / 128)) ranges of `chunk` rows (a multiple of 16)
__host__ __device__ inline void head_bwd_splits(int64_t R, int &S, int &chunk)
{
    int64_t s = (R + kHeadBwdSplitRows - 1) / kHeadBwdSplitRows;
    if (s > kHeadBwdMaxSplits) s = kHeadBwdMaxSplits;
    if (s < 1) s = 1;
    const int64_t c = 16 * (((R + s - 1) / s + 15) / 16);
    S = (int)((R + c - 1) / c);
    chunk = (int)c;
}

struct HeadBwdLayout {                                       // byte offsets into the (aligned) scratch
    size_t dlin, part, wpart, total;
    int CP, S, chunk;
};

// The scratch of every producer entry that takes one: the pieces start on kHeadBwdAlign boundaries of the pointer rounded up (so
// a query answers its layout's total + kHeadBwdAlign).
inline size_t scratch_up(size_t v) { return (v + kHeadBwdAlign - 1) / kHeadBwdAlign * kHeadBwdAlign; }
inline char *scratch_base(void *scratch) { return reinterpret_cast<char *>(scratch_up(reinterpret_cast<uintptr_t>(scratch))); }

// What the head's backward entries, the wide forward entry and their scratch queries take of (T, B, K, C): B up to `max_batch`
// (kHeadMaxBatch: a frame in one workgroup; kHeadWideMaxBatch: head_wide.hpp), K a multiple of 16, row and task counts inside
// the launches' index range.
inline bool head_shape_ok(int T, int B, int K, int C, int max_batch)
{
    if (B > max_batch || (K & 15) != 0) return false;
    const int64_t R = (int64_t)T * B;
    if (R > kHeadBwdMaxRows) return false;
    int S, chunk;
    head_bwd_splits(R, S, chunk);
    const int64_t CT = (C + 15) / 16, KQ = (K / 16 + 3) / 4;
    const int64_t tasks = CT * KQ * S + ((R + 15) / 16) * KQ + (3 * 16 * CT + 63) / 64;
    return CT <= 65535 && tasks <= kHeadBwdMaxTasks;
}

inline HeadBwdLayout head_bwd_layout(int T, int B, int K, int C)
{
    HeadBwdLayout L;
    const size_t R = (size_t)T * (size_t)B;
    L.CP = 16 * ((C + 15) / 16);
    head_bwd_splits((int64_t)R, L.S, L.chunk);
    L.dlin = 0;
    L.part = scratch_up(R * L.CP * sizeof(float));
    L.wpart = L.part + scratch_up((size_t)3 * T * L.CP * sizeof(float));
    L.total = L.wpart + (L.S > 1 ? scratch_up((size_t)L.S * C * K * sizeof(float)) : 0);
    return L;
}

// the answer of both scratch queries of the head's backward (0: the shape is not one the entry takes)
inline size_t head_bwd_scratch_bytes(int T, int B, int K, int C, int max_batch)
{
    if (T < 1 || B < 1 || K < 1 || C < 1 || !head_shape_ok(T, B, K, C, max_batch)) return 0;
    return head_bwd_layout(T, B, K, C).total + kHeadBwdAlign;
}

struct HeadBwdRowsParams {
    const float *dout;                                       // rows of C at (dst, dsb)
    int64_t dst, dsb;
    const float *lin, *gamma, *beta;                         // [T][B][C]; [C]
    const float *smean, *sinv;                               // train: [T][C]
    const float *rmean, *rvar;                               // eval: [C]
    const float *mask;                                       // [T][B][C] or NULL
    float eps;
    int T, B, C, CP;
    float *dlin, *part;                                      // [T B][CP]; [3][T][CP]: dbeta_t, dgamma_t, sum_b dlin
};

__global__ __launch_bounds__(1024) void head_bwd_rows_kernel(HeadBwdRowsParams p)
{
    __shared__ float red[16][16];
    const int t = blockIdx.x, n = blockIdx.y, tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    const int fr = lane & 15, fq = lane >> 4;
    const int NW = blockDim.x >> 6;
    const int col = 16 * n + fr;                             // (< CP)
    const bool colok = col < p.C, train = p.smean != nullptr;
    float mean = 0.f, inv = 0.f, g = 0.f, be = 0.f;
    if (colok) {
        mean = train ? p.smean[(int64_t)t * p.C + col] : p.rmean[col];
        inv = train ? p.sinv[(int64_t)t * p.C + col] : head_invstd(p.rvar[col], p.eps);
        g = p.gamma[col];
        be = p.beta[col];
    }
    float dy[4], xh[4];
    bool rowok[4];
    float sb = 0.f, sg = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int b = 16 * w + 4 * fq + j;
        rowok[j] = b < p.B;
        dy[j] = 0.f; xh[j] = 0.f;
        if (rowok[j] && colok) {
            const int64_t i = ((int64_t)t * p.B + b) * p.C + col;
            const float x = p.lin[i];
            float d = p.dout[(int64_t)t * p.dst + (int64_t)b * p.dsb + col];
            if (p.mask) d *= p.mask[i];
            xh[j] = (x - mean) * inv;
            dy[j] = head_bn_y(x, mean, inv, g, be) > 0.f ? d : 0.f;
        }
        sb += dy[j];
        sg += dy[j] * xh[j];
    }
    const float dbeta = head_column_total(sb, red, w, fr, fq, NW);
    const float dgamma = head_column_total(sg, red, w, fr, fq, NW);
    const float mb = dbeta / (float)p.B, mg = dgamma / (float)p.B;
    float sd = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int b = 16 * w + 4 * fq + j;
        if (!rowok[j]) continue;                             // (uniform per lane quarter; no barrier below depends on it)
        float dl = 0.f;
        if (colok) dl = train ? inv * g * (dy[j] - mb - xh[j] * mg) : dy[j] * g * inv;
        sd += dl;
        p.dlin[((int64_t)t * p.B + b) * p.CP + col] = dl;    // the pad columns get their zeros here
    }
    const float dsum = head_column_total(sd, red, w, fr, fq, NW);
    if (w == 0 && fq == 0) {
        const int64_t TC = (int64_t)p.T * p.CP, i = (int64_t)t * p.CP + col;
        p.part[i] = dbeta;
        p.part[TC + i] = dgamma;
        p.part[2 * TC + i] = dsum;
    }
}

struct HeadBwdProdParams {
    const float *dlin, *part;                                // as the rows launch left them
    const void *feat;                                        // of the kernel's element type E
    int64_t fst, fsb;
    const float *w;                                          // [C][K]
    int T, B, K, C, CP;
    int R, S, chunk;                                         // rows T B; row-range splits of the weight gradient
    float *dw;                                               // S == 1: d_weight [C][K]; else the partials [S][C][K]
    void *dfeat;                                             // of E as well, or NULL
    int64_t gst, gsb;
    float *dbias, *dgamma, *dbeta;
    int64_t nW, nF, nTail;                                   // tasks of the three roles
};

// E: the element type of feat and d_feat.  The d_weight role widens feat exactly (bf16: a shift; fp16: v_cvt_f32_f16); the d_feat
// role rounds its fp32 accumulator once, to nearest even.  float: the loads and stores as they were.
template <typename E>
__global__ __launch_bounds__(256) void head_bwd_products_kernel(HeadBwdProdParams p)
{
    const int lane = threadIdx.x & 63, fr = lane & 15, fq = lane >> 4;
    int64_t task = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int KQ = ((p.K >> 4) + 3) >> 2;
    head_f4 acc[4];
#pragma unroll
    for (int n = 0; n < 4; ++n) acc[n] = head_f4{0.f, 0.f, 0.f, 0.f};
    if (task < p.nW) {
        // d_weight[c][k] = sum_r dlin[r][c] feat[r][k]: A[c][r] = dlin, B[r][k] = feat; MFMA i of a 16-row step takes
        // rows rb + 4 i + fq.  One chain per element over r ascending within (step, i, fq).
        const int CT = p.CP >> 4;
        const int s = (int)(task / ((int64_t)CT * KQ));
        const int rem = (int)(task - (int64_t)s * CT * KQ);
        const int ct = rem / KQ, kq = rem - ct * KQ;
        const int col = 16 * ct + fr;                        // (< CP: the pad columns of dlin hold zeros)
        int kc[4];
#pragma unroll
        for (int n = 0; n < 4; ++n) kc[n] = min(64 * kq + 16 * n + fr, p.K - 1);
        const int r0 = s * p.chunk, rend = min(p.R, r0 + p.chunk);
        for (int rb = r0; rb < rend; rb += 16) {
            float a[4], b[4][4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int r = rb + 4 * i + fq;
                const bool ok = r < rend;
                const int rc = ok ? r : rend - 1;            // (an address inside the range; the value is dropped)
                const int tt = rc / p.B, bb = rc - tt * p.B;
                const float av = p.dlin[(int64_t)rc * p.CP + col];
                const E *fp = static_cast<const E *>(p.feat) + (int64_t)tt * p.fst + (int64_t)bb * p.fsb;
                a[i] = ok ? av : 0.f;
#pragma unroll
                for (int n = 0; n < 4; ++n) {
                    const float bv = (float)fp[kc[n]];
                    b[n][i] = ok ? bv : 0.f;
                }
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int n = 0; n < 4; ++n) acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[n][i], acc[n], 0, 0, 0);
        }
        // acc[n][j] = (c = 16 ct + 4 fq + j, k = 64 kq + 16 n + fr)
        float *out = p.dw + (int64_t)s * p.C * p.K;
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            const int k = 64 * kq + 16 * n + fr;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int c = 16 * ct + 4 * fq + j;
                if (c < p.C && k < p.K) out[(int64_t)c * p.K + k] = acc[n][j];
            }
        }
        return;
    }
    task -= p.nW;
    if (task < p.nF) {
        // d_feat[r][k] = sum_c dlin[r][c] W[c][k]: A[r][c] = dlin (16 bytes of the row per lane: MFMA i of a 16-column
        // block takes c = 16 cb + 4 fq + i on both operands), B[c][k] = W.
        const int rt = (int)(task / KQ), kq = (int)(task - (int64_t)rt * KQ);
        const int ra = min(16 * rt + fr, p.R - 1);
        const float *ap = p.dlin + (int64_t)ra * p.CP + 4 * fq;
        int kc[4];
#pragma unroll
        for (int n = 0; n < 4; ++n) kc[n] = min(64 * kq + 16 * n + fr, p.K - 1);
        for (int cb = 0; cb < (p.CP >> 4); ++cb) {
            const head_f4 a = *reinterpret_cast<const head_f4 *>(ap + 16 * cb);
            float b[4][4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int c = 16 * cb + 4 * fq + i;
                const bool ok = c < p.C;
                const float *wp = p.w + (int64_t)(ok ? c : p.C - 1) * p.K;
#pragma unroll
                for (int n = 0; n < 4; ++n) {
                    const float bv = wp[kc[n]];
                    b[n][i] = ok ? bv : 0.f;
                }
            }
#pragma unroll
            for (int n = 0; n < 4; ++n) acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b[n][0], acc[n], 0, 0, 0);
#pragma unroll
            for (int n = 0; n < 4; ++n) acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b[n][1], acc[n], 0, 0, 0);
#pragma unroll
            for (int n = 0; n < 4; ++n) acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b[n][2], acc[n], 0, 0, 0);
#pragma unroll
            for (int n = 0; n < 4; ++n) acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b[n][3], acc[n], 0, 0, 0);
        }
        // acc[n][j] = (r = 16 rt + 4 fq + j, k = 64 kq + 16 n + fr)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int r = 16 * rt + 4 * fq + j;
            if (r >= p.R) continue;
            const int tt = r / p.B, bb = r - tt * p.B;
            E *out = static_cast<E *>(p.dfeat) + (int64_t)tt * p.gst + (int64_t)bb * p.gsb;
#pragma unroll
            for (int n = 0; n < 4; ++n) {
                const int k = 64 * kq + 16 * n + fr;
                if (k < p.K) out[k] = (E)acc[n][j];
            }
        }
        return;
    }
    task -= p.nF;
    if (task < p.nTail) {
        // the per-frame partials summed over the frames, t ascending
        const int64_t i = task * 64 + lane;
        const int which = (int)(i / p.CP), c = (int)(i - (int64_t)which * p.CP);
        if (which < 3 && c < p.C) {
            const float *q = p.part + (int64_t)which * p.T * p.CP + c;
            float s = 0.f;
            for (int t = 0; t < p.T; ++t) s += q[(int64_t)t * p.CP];
            (which == 0 ? p.dbeta : which == 1 ? p.dgamma : p.dbias)[c] = s;
        }
    }
}

// d_weight = the S partial tiles added in ascending split order
__global__ __launch_bounds__(256) void head_bwd_reduce_kernel(const float *wpart, float *dw, int64_t n, int S)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float s = 0.f;
    for (int k = 0; k < S; ++k) s += wpart[(int64_t)k * n + i];
    dw[i] = s;
}

}  // namespace ctc

namespace ctc {

// The backward of the head behind both *_typed entries (the untyped ones forward to those with CTC_AMD_F32): the checks, the
// scratch carve-up, both parameter blocks, the task count and the products and reduce launches.  What differs comes from the
// caller: the bound on B and the rows launch, rows(grid, stream, r) -- head_bwd_rows_kernel with a frame in one workgroup or
// head_wide_bwd_rows_kernel walking the frame's row blocks.
template <typename Rows>
inline int head_backward_enqueue(int max_batch, Rows rows, const float *d_out, int64_t dout_stride_t, int64_t dout_stride_b,
                                 const void *feat, int feat_dtype, int64_t feat_stride_t, int64_t feat_stride_b,
                                 const float *weight, const float *bn_weight, const float *bn_bias, const float *linear_out,
                                 const float *save_mean, const float *save_invstd,
                                 const float *running_mean, const float *running_var, float eps, const float *mask,
                                 int T, int B, int K, int C, void *d_feat, int64_t dfeat_stride_t, int64_t dfeat_stride_b,
                                 float *d_weight, float *d_bias, float *d_bn_weight, float *d_bn_bias,
                                 void *scratch, size_t scratch_bytes, void *stream)
{
    if (!head_dtype_ok(feat_dtype)) return CTC_AMD_ERR_BAD_ARGUMENT;
    if (!d_out || !feat || !weight || !bn_weight || !bn_bias || !linear_out) return CTC_AMD_ERR_BAD_ARGUMENT;
    if (!d_weight || !d_bias || !d_bn_weight || !d_bn_bias || !scratch) return CTC_AMD_ERR_BAD_ARGUMENT;
    if (T < 1 || B < 1 || K < 1 || C < 1) return CTC_AMD_ERR_BAD_ARGUMENT;
    const bool train = save_mean && save_invstd && !running_mean && !running_var;
    const bool eval = running_mean && running_var && !save_mean && !save_invstd;
    if (!train && !eval) return CTC_AMD_ERR_BAD_ARGUMENT;
    if (train && B < 2) return CTC_AMD_ERR_BAD_ARGUMENT;
    if (dout_stride_b < C) return CTC_AMD_ERR_BAD_ARGUMENT;
    if (d_feat && dfeat_stride_b < K) return CTC_AMD_ERR_BAD_ARGUMENT;
    if (scratch_bytes < head_bwd_scratch_bytes(T, B, K, C, max_batch)) return CTC_AMD_ERR_BAD_ARGUMENT;
    // what the forward entry refuses, row counts beyond the launches' index range, and d_feat of a 2-byte element type off its
    // 2-byte boundary (written with 2-byte stores; fp32 as the untyped entries take it)
    if (!head_shape_ok(T, B, K, C, max_batch) || !head_operands_ok(feat, feat_dtype, feat_stride_t, feat_stride_b, weight, K) ||
        (d_feat && feat_dtype != CTC_AMD_F32 && (reinterpret_cast<uintptr_t>(d_feat) & 1) != 0))
        return CTC_AMD_ERR_UNSUPPORTED_SHAPE;
    const HeadBwdLayout L = head_bwd_layout(T, B, K, C);
    char *base = scratch_base(scratch);
    float *dlin = reinterpret_cast<float *>(base + L.dlin), *part = reinterpret_cast<float *>(base + L.part);
    float *wpart = reinterpret_cast<float *>(base + L.wpart);
    hipStream_t st = static_cast<hipStream_t>(stream);

    HeadBwdRowsParams r;
    r.dout = d_out; r.dst = dout_stride_t; r.dsb = dout_stride_b;
    r.lin = linear_out; r.gamma = bn_weight; r.beta = bn_bias;
    r.smean = save_mean; r.sinv = save_invstd; r.rmean = running_mean; r.rvar = running_var;
    r.mask = mask; r.eps = eps;
    r.T = T; r.B = B; r.C = C; r.CP = L.CP;
    r.dlin = dlin; r.part = part;
    int rc = rows(dim3(T, L.CP / 16), st, r);
    if (rc) return rc;

    HeadBwdProdParams q;
    q.dlin = dlin; q.part = part;
    q.feat = feat; q.fst = feat_stride_t; q.fsb = feat_stride_b; q.w = weight;
    q.T = T; q.B = B; q.K = K; q.C = C; q.CP = L.CP;
    q.R = T * B; q.S = L.S; q.chunk = L.chunk;
    q.dw = L.S > 1 ? wpart : d_weight;
    q.dfeat = d_feat; q.gst = dfeat_stride_t; q.gsb = dfeat_stride_b;
    q.dbias = d_bias; q.dgamma = d_bn_weight; q.dbeta = d_bn_bias;
    const int64_t KQ = (K / 16 + 3) / 4;
    q.nW = (int64_t)(L.CP / 16) * KQ * L.S;
    q.nF = d_feat ? (((int64_t)q.R + 15) / 16) * KQ : 0;
    q.nTail = (3 * (int64_t)L.CP + 63) / 64;
    const int64_t tasks = q.nW + q.nF + q.nTail;
    rc = with_logit_elem(feat_dtype, [&](auto e) {          // the element type of feat and d_feat
        using E = typename decltype(e)::type;
        return launch<head_bwd_products_kernel<E>>(dim3((unsigned)((tasks + 3) / 4)), dim3(256), 0, st, q);
    });
    if (rc || L.S == 1) return rc;
    const int64_t n = (int64_t)C * K;
    return launch<head_bwd_reduce_kernel>(dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const float *)wpart, d_weight, n, L.S);
}

}  // namespace ctc

extern "C" size_t ctc_amd_head_backward_scratch_bytes(int T, int B, int K, int C)
{
    return ctc::head_bwd_scratch_bytes(T, B, K, C, ctc::kHeadMaxBatch);
}

extern "C" int ctc_amd_head_backward_typed(const float *d_out, int64_t dout_stride_t, int64_t dout_stride_b,
                                           const void *feat, int feat_dtype, int64_t feat_stride_t, int64_t feat_stride_b,
                                           const float *weight, const float *bn_weight, const float *bn_bias,
                                           const float *linear_out,
                                           const float *save_mean, const float *save_invstd,
                                           const float *running_mean, const float *running_var, float eps,
                                           const float *mask,
                                           int T, int B, int K, int C,
                                           void *d_feat, int64_t dfeat_stride_t, int64_t dfeat_stride_b,
                                           float *d_weight, float *d_bias, float *d_bn_weight, float *d_bn_bias,
                                           void *scratch, size_t scratch_bytes, void *stream)
{
    auto rows = [](dim3 grid, hipStream_t st, const ctc::HeadBwdRowsParams &r) {
        return launch<ctc::head_bwd_rows_kernel>(grid, dim3(64 * ((r.B + 15) / 16)), 0, st, r);
    };
    return ctc::head_backward_enqueue(ctc::kHeadMaxBatch, rows, d_out, dout_stride_t, dout_stride_b, feat, feat_dtype,
                                      feat_stride_t, feat_stride_b, weight, bn_weight, bn_bias, linear_out, save_mean, save_invstd,
                                      running_mean, running_var, eps, mask, T, B, K, C, d_feat, dfeat_stride_t, dfeat_stride_b,
                                      d_weight, d_bias, d_bn_weight, d_bn_bias, scratch, scratch_bytes, stream);
}

extern "C" int ctc_amd_head_backward(const float *d_out, int64_t dout_stride_t, int64_t dout_stride_b,
                                     const float *feat, int64_t feat_stride_t, int64_t feat_stride_b,
                                     const float *weight, const float *bn_weight, const float *bn_bias,
                                     const float *linear_out,
                                     const float *save_mean, const float *save_invstd,
                                     const float *running_mean, const float *running_var, float eps,
                                     const float *mask,
                                     int T, int B, int K, int C,
                                     float *d_feat, int64_t dfeat_stride_t, int64_t dfeat_stride_b,
                                     float *d_weight, float *d_bias, float *d_bn_weight, float *d_bn_bias,
                                     void *scratch, size_t scratch_bytes, void *stream)
{
    return ctc_amd_head_backward_typed(d_out, dout_stride_t, dout_stride_b, feat, CTC_AMD_F32, feat_stride_t, feat_stride_b,
                                       weight, bn_weight, bn_bias, linear_out, save_mean, save_invstd, running_mean, running_var,
                                       eps, mask, T, B, K, C, d_feat, dfeat_stride_t, dfeat_stride_b,
                                       d_weight, d_bias, d_bn_weight, d_bn_bias, scratch, scratch_bytes, stream);
}

// ---------------------------------------------------------------------------------------------------------------------
// The BACKWARD of ctc_amd_lstm_series, whole: the recurrence launch above writes dpre [T B][4H] into the scratch,
// and everything that is not a recurrence follows as HIP launches on the same stream, head_bwd_products_kernel's scheme:
//   products  one wave per task, exact fp32 on the matrix cores (an fmaf chain per output element):
//               d^T x tile [16 gate rows x (I or H)] of one row-range split, contracting over the rows (4-byte operand loads);
//                 the role runs twice -- against x (d_w_ih) and against h_{t-1} (d_w_hh), which is read IN PLACE: h0 for
//                 t = 0, row t - 1 of the forward's v_series at its own pitch otherwise;
//               d W tile [16 rows x I] (d_x), contracting over the 4H gate rows (16-byte loads of the dpre row);
//               column sums: 64 gate columns of one row-range split, rows ascending (the biases);
//   reduce    (S > 1 only) the S partial [d_w_ih | d_w_hh | d_b] added in ascending split order; writes d_b_ih and d_b_hh.
// S and the rows per split are the head's rule (head_bwd_splits), with R = T B: chunk = 16 ceil(ceil(R / min(64, ceil(R / 128))) / 16)
// rows per range, S = ceil(R / chunk) ranges (9600 rows: 60 ranges of 160) -- a function of T B alone: the same shape sums
// in the same order.
namespace ctc {

struct LstmBwdLayout {                                       // byte offsets into the (aligned) scratch
    size_t dpre, wpart, total;
    int S, chunk;
    int64_t ntot;                                            // floats of one split's partials: 4H (I + H + 1)
};

inline bool lstm_bwd_shape_ok(int T, int B, int I, int H)
{
    // ctc_amd_lstm_series's own bounds, compared without arithmetic on the sizes (no int overflow for any I, H)
    if (I > kLstmThreads / kSeriesSamples || H > kLstmThreads / kSeriesSamples || H > kSeriesG / 4 || I > kSeriesK - H) return false;
    return (int64_t)T * B <= kHeadBwdMaxRows;
}

inline LstmBwdLayout lstm_bwd_layout(int T, int B, int I, int H)
{
    LstmBwdLayout L;
    const size_t R = (size_t)T * (size_t)B;
    head_bwd_splits((int64_t)R, L.S, L.chunk);
    L.ntot = (int64_t)4 * H * (I + H + 1);
    L.dpre = 0;
    L.wpart = scratch_up(R * 4 * H * sizeof(float));
    L.total = L.wpart + (L.S > 1 ? scratch_up((size_t)L.S * (size_t)L.ntot * sizeof(float)) : 0);
    return L;
}

struct LstmBwdProdParams {
    const float *dpre;                                       // [R][G] as the recurrence launch left it
    const float *x;                                          // rows of I at (xst, xsb)
    int64_t xst, xsb;
    const float *h0, *series;                                // h_{t-1}: h0 [B][H] for t = 0, row (t - 1, b) of series otherwise
    int64_t sst, ssb;
    const float *w_ih;                                       // [G][I]
    int B, I, H, G;
    int R, S, chunk;                                         // rows T B; row-range splits
    float *dwi, *dwh, *db0, *db1;                            // S == 1: the outputs; else split 0 of the partials (db1 NULL)
    int64_t pstride;                                         // floats between two splits' partials
    float *dx;                                               // or NULL
    int64_t dxst, dxsb;
    int64_t nW, nX, nB;                                      // tasks of the three roles
};

__global__ __launch_bounds__(256) void lstm_bwd_products_kernel(LstmBwdProdParams p)
{
    const int lane = threadIdx.x & 63, fr = lane & 15, fq = lane >> 4;
    int64_t task = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int G = p.G, GT = (G + 15) >> 4;
    head_f4 acc[4];
#pragma unroll
    for (int n = 0; n < 4; ++n) acc[n] = head_f4{0.f, 0.f, 0.f, 0.f};
    if (task < p.nW) {
        // d_w[g][k] = sum_r dpre[r][g] v[r][k] (v = x or h_{t-1}): A[g][r] = dpre, B[r][k] = v; MFMA i of a 16-row step takes
        // rows rb + 4 i + fq.  One chain per element over r ascending within (step, i, fq).
        const int s = (int)(task / (2 * GT));
        const int rem = (int)(task - (int64_t)s * 2 * GT);
        const int which = rem / GT, gt = rem - which * GT;   // 0: x, 1: h_{t-1}
        const int K = which ? p.H : p.I, NT = (K + 15) >> 4;
        const int col = 16 * gt + fr;
        const bool colok = col < G;
        const int colc = colok ? col : G - 1;
        int kc[4];
#pragma unroll
        for (int n = 0; n < 4; ++n) kc[n] = min(16 * n + fr, K - 1);
        const int r0 = s * p.chunk, rend = min(p.R, r0 + p.chunk);
        for (int rb = r0; rb < rend; rb += 16) {
            float a[4], b[4][4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int r = rb + 4 * i + fq;
                const bool ok = r < rend;
                const int rc = ok ? r : rend - 1;            // (an address inside the range; the value is dropped)
                const int tt = rc / p.B, bb = rc - tt * p.B;
                const float av = p.dpre[(int64_t)rc * G + colc];
                const float *vp = which == 0 ? p.x + (int64_t)tt * p.xst + (int64_t)bb * p.xsb
                                  : tt == 0  ? p.h0 + (int64_t)bb * p.H
                                             : p.series + (int64_t)(tt - 1) * p.sst + (int64_t)bb * p.ssb;
                a[i] = (ok && colok) ? av : 0.f;
#pragma unroll
                for (int n = 0; n < 4; ++n) {
                    float bv = 0.f;
                    if (n < NT) bv = vp[kc[n]];              // (uniform)
                    b[n][i] = ok ? bv : 0.f;
                }
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int n = 0; n < 4; ++n)
                    if (n < NT) acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[n][i], acc[n], 0, 0, 0);
        }
        // acc[n][j] = (g = 16 gt + 4 fq + j, k = 16 n + fr)
        float *out = (which ? p.dwh : p.dwi) + (int64_t)s * p.pstride;
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            const int k = 16 * n + fr;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int g = 16 * gt + 4 * fq + j;
                if (g < G && k < K) out[(int64_t)g * K + k] = acc[n][j];
            }
        }
        return;
    }
    task -= p.nW;
    if (task < p.nX) {
        // d_x[r][k] = sum_g dpre[r][g] W_ih[g][k]: A[r][g] = dpre (16 bytes of the row per lane: MFMA i of a 16-column block
        // takes g = 16 gb + 4 fq + i on both operands; G is a multiple of 4, so a lane's four are inside G or all outside).
        const int rt = (int)task, NT = (p.I + 15) >> 4;
        const int ra = min(16 * rt + fr, p.R - 1);
        const float *ap = p.dpre + (int64_t)ra * G + 4 * fq;
        int kc[4];
#pragma unroll
        for (int n = 0; n < 4; ++n) kc[n] = min(16 * n + fr, p.I - 1);
        for (int gb = 0; gb < GT; ++gb) {
            const int g0 = 16 * gb + 4 * fq;
            const bool ok = g0 < G;
            head_f4 a = {0.f, 0.f, 0.f, 0.f};
            if (ok) a = *reinterpret_cast<const head_f4 *>(ap + 16 * gb);
            const float *wp = p.w_ih + (int64_t)(ok ? g0 : 0) * p.I;
            float b[4][4];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int n = 0; n < 4; ++n) {
                    float bv = 0.f;
                    if (n < NT) bv = wp[(int64_t)i * p.I + kc[n]];      // (uniform)
                    b[n][i] = ok ? bv : 0.f;
                }
#pragma unroll
            for (int n = 0; n < 4; ++n) if (n < NT) acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b[n][0], acc[n], 0, 0, 0);
#pragma unroll
            for (int n = 0; n < 4; ++n) if (n < NT) acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b[n][1], acc[n], 0, 0, 0);
#pragma unroll
            for (int n = 0; n < 4; ++n) if (n < NT) acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b[n][2], acc[n], 0, 0, 0);
#pragma unroll
            for (int n = 0; n < 4; ++n) if (n < NT) acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b[n][3], acc[n], 0, 0, 0);
        }
        // acc[n][j] = (r = 16 rt + 4 fq + j, k = 16 n + fr)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int r = 16 * rt + 4 * fq + j;
            if (r >= p.R) continue;
            const int tt = r / p.B, bb = r - tt * p.B;
            float *out = p.dx + (int64_t)tt * p.dxst + (int64_t)bb * p.dxsb;
#pragma unroll
            for (int n = 0; n < 4; ++n) {
                const int k = 16 * n + fr;
                if (k < p.I) out[k] = acc[n][j];
            }
        }
        return;
    }
    task -= p.nX;
    if (task < p.nB) {
        // the column sums of one row range, rows ascending (sixteen loads in flight, added in row order)
        const int CG = (G + 63) >> 6;
        const int s = (int)(task / CG), c = 64 * (int)(task - (int64_t)s * CG) + lane;
        if (c >= G) return;
        const int r0 = s * p.chunk, rend = min(p.R, r0 + p.chunk);
        const float *q = p.dpre + c;
        float sum = 0.f;
        int r = r0;
        for (; r + 16 <= rend; r += 16) {
            float v[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) v[u] = q[(int64_t)(r + u) * G];
#pragma unroll
            for (int u = 0; u < 16; ++u) sum += v[u];
        }
        for (; r < rend; ++r) sum += q[(int64_t)r * G];
        p.db0[(int64_t)s * p.pstride + c] = sum;
        if (p.db1) p.db1[c] = sum;
    }
}

// [d_w_ih | d_w_hh | d_b] = the S partials added in ascending split order; the bias sums go to both bias gradients
__global__ __launch_bounds__(256) void lstm_bwd_reduce_kernel(const float *part, int64_t ntot, int S, int64_t nwi, int64_t nwh,
                                                              float *dwi, float *dwh, float *db0, float *db1)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= ntot) return;
    float s = 0.f;
    for (int k = 0; k < S; ++k) s += part[(int64_t)k * ntot + i];
    if (i < nwi) dwi[i] = s;
    else if (i < nwi + nwh) dwh[i - nwi] = s;
    else {
        db0[i - nwi - nwh] = s;
        db1[i - nwi - nwh] = s;
    }
}

}  // namespace ctc

extern "C" size_t ctc_amd_lstm_backward_scratch_bytes(int T, int B, int I, int H)
{
    if (T < 1 || B < 1 || I < 1 || H < 1 || !ctc::lstm_bwd_shape_ok(T, B, I, H)) return 0;
    return ctc::lstm_bwd_layout(T, B, I, H).total + ctc::kHeadBwdAlign;           // (the entry aligns the pointer itself)
}

extern "C" int ctc_amd_lstm_backward(const float *d_series, int64_t ds_stride_t, int64_t ds_stride_b,
                                     const float *gates, const float *cells,
                                     const float *x, int64_t x_stride_t, int64_t x_stride_b,
                                     const float *h0,
                                     const float *series, int64_t series_stride_t, int64_t series_stride_b,
                                     const float *w_ih, const float *w_hh,
                                     int T, int B, int I, int H,
                                     float *d_x, int64_t dx_stride_t, int64_t dx_stride_b,
                                     float *dh0, float *dc0,
                                     float *d_w_ih, float *d_w_hh, float *d_b_ih, float *d_b_hh,
                                     void *scratch, size_t scratch_bytes, void *stream)
{
    if (!d_series || !gates || !cells || !x || !h0 || !series || !w_ih || !w_hh) return CTC_AMD_ERR_BAD_ARGUMENT;
    if (!dh0 || !dc0 || !d_w_ih || !d_w_hh || !d_b_ih || !d_b_hh || !scratch) return CTC_AMD_ERR_BAD_ARGUMENT;
    if (T < 1 || B < 1 || I < 1 || H < 1) return CTC_AMD_ERR_BAD_ARGUMENT;
    if (ds_stride_b < H || series_stride_b < H || x_stride_b < I) return CTC_AMD_ERR_BAD_ARGUMENT;
    if (d_x && dx_stride_b < I) return CTC_AMD_ERR_BAD_ARGUMENT;
    if (scratch_bytes < ctc_amd_lstm_backward_scratch_bytes(T, B, I, H)) return CTC_AMD_ERR_BAD_ARGUMENT;
    // what ctc_amd_lstm_series refuses (the saved gates and cells can only come from it), and row counts beyond the index range
    if (!ctc::lstm_bwd_shape_ok(T, B, I, H)) return CTC_AMD_ERR_UNSUPPORTED_SHAPE;
    const ctc::LstmBwdLayout L = ctc::lstm_bwd_layout(T, B, I, H);
    char *base = ctc::scratch_base(scratch);
    float *dpre = reinterpret_cast<float *>(base + L.dpre), *wpart = reinterpret_cast<float *>(base + L.wpart);
    hipStream_t st = static_cast<hipStream_t>(stream);

    int rc = enqueue_series_backward(series_bwd_params(d_series, ds_stride_t, ds_stride_b, gates, cells, w_hh, T, B, H, dpre, dh0, dc0), st);
    if (rc) return rc;

    const int G = 4 * H;
    const int64_t nwi = (int64_t)G * I, nwh = (int64_t)G * H;
    ctc::LstmBwdProdParams q;
    q.dpre = dpre;
    q.x = x; q.xst = x_stride_t; q.xsb = x_stride_b;
    q.h0 = h0; q.series = series; q.sst = series_stride_t; q.ssb = series_stride_b;
    q.w_ih = w_ih;
    q.B = B; q.I = I; q.H = H; q.G = G;
    q.R = T * B; q.S = L.S; q.chunk = L.chunk;
    if (L.S > 1) {
        q.dwi = wpart; q.dwh = wpart + nwi; q.db0 = wpart + nwi + nwh; q.db1 = nullptr; q.pstride = L.ntot;
    } else {
        q.dwi = d_w_ih; q.dwh = d_w_hh; q.db0 = d_b_ih; q.db1 = d_b_hh; q.pstride = 0;
    }
    q.dx = d_x; q.dxst = dx_stride_t; q.dxsb = dx_stride_b;
    q.nW = (int64_t)2 * ((G + 15) / 16) * L.S;
    q.nX = d_x ? ((int64_t)q.R + 15) / 16 : 0;
    q.nB = (int64_t)((G + 63) / 64) * L.S;
    const int64_t tasks = q.nW + q.nX + q.nB;
    rc = launch<ctc::lstm_bwd_products_kernel>(dim3((unsigned)((tasks + 3) / 4)), dim3(256), 0, st, q);
    if (rc || L.S == 1) return rc;
    return launch<ctc::lstm_bwd_reduce_kernel>(dim3((unsigned)((L.ntot + 255) / 256)), dim3(256), 0, st,
                                               (const float *)wpart, L.ntot, L.S, nwi, nwh, d_w_ih, d_w_hh, d_b_ih, d_b_hh);
}

#include "lstm_wide.hpp"
#include "head_wide.hpp"
