// The recurrence of LSTM_cell beyond the reference's class counts: 1 <= I, H <= kWideMax = 160, which takes
// the benchmark's C = 158.  Included at the end of producer.hip (sigmoid_f, LstmSeriesParams, LstmSeriesBwdParams and their
// fillers series_params / series_bwd_params, scratch_base / scratch_up and the row bound of the head's backward are that file's).
//
// [W_ih | W_hh] at H = 158 is 800 KB: neither the LDS (160 KiB) nor a workgroup's registers hold it, so the narrow kernels'
// "gate row in registers for the whole launch" does not carry over.  The weights stay in L2 and are STREAMED every frame;
// what the layout buys is that every such read is coalesced and shared by all samples of the workgroup:
//   forward   thread r owns gate row r (up to 640 threads).  It needs W[r][k] for k ascending, so the launch reads a
//             TRANSPOSED copy wt [I + H][4H] (lanes over r: 256 contiguous bytes per wave and k), made once per call in
//             the scratch.  The x part of the pre-activations is no recurrence: a launch of its own computes it for all
//             T B rows (16 rows per workgroup, the same k-ascending fmaf chain from 0) into the scratch, and the
//             recurrence picks it up as the starting value of the W_hh chain -- an fp32 store and load is exact, so the
//             chain is the chain of lstm_cell_step_kernel: W_ih part, W_hh part, then the bias sum.  Bit for bit.
//   backward  dh_{t-1}(s, j) = sum_r W_hh[r][j] dpre(s, r): lanes over j read row-major W_hh coalesced as it lies.  Thread
//             (q, j) sums gate chunk q (H rows) for the four samples, the four partial sums meet in LDS and are added in
//             ascending q: a fixed order, no atomics.
//   bias      d_b = the column sums of dpre: a launch of its own (lstm_wide_colsum_kernel), fixed order, no scratch, nothing to
//             clear -- a captured training step replays to the eager bits.
// The staged vectors lie sample-minor in LDS ([k][4]): one 16-byte broadcast read serves four fmaf.  Only __syncthreads()
// in control flow uniform over the T loop; no workgroup waits on another.
#pragma once

namespace ctc {

constexpr int kWideMax = 160;                                // the bound on I and on H
constexpr int kWideSamples = 4;                              // samples per workgroup of the two recurrences
constexpr int kWideGates = 4;                                // gate chunks (i, f, g, o) of H rows each
constexpr int kWideThreads = kWideGates * kWideMax;          // one thread per gate row
static_assert(kWideSamples == kWideGates, "a thread is (sample, unit) of the cell update and (gate chunk, column) of the products");
constexpr int kWideXRows = 16;                               // (t, b) rows per workgroup of the x-part launch

struct LstmWideLayout {                                      // byte offsets into the (aligned) scratch
    size_t wt, xpre, total;
};

inline bool lstm_wide_shape_ok(int T, int B, int I, int H)
{
    return I <= kWideMax && H <= kWideMax && (int64_t)T * B <= kHeadBwdMaxRows;
}

inline LstmWideLayout lstm_wide_layout(int T, int B, int I, int H)
{
    LstmWideLayout L;
    const size_t R = (size_t)T * (size_t)B, G = 4 * (size_t)H;
    L.wt = 0;
    L.xpre = scratch_up(((size_t)I + H) * G * sizeof(float));
    L.total = L.xpre + scratch_up(R * G * sizeof(float));
    return L;
}

__host__ __device__ inline unsigned wide_block(int G) { return 64u * (unsigned)((G + 63) / 64); }

// wt [I + H][4H]: row k < I is column k of W_ih, row I + k column k of W_hh
__global__ __launch_bounds__(256) void lstm_wide_transpose_kernel(const float *w_ih, const float *w_hh, int I, int H, float *wt)
{
    const int G = 4 * H, n = (I + H) * G;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int k = i / G, r = i - k * G;
    wt[i] = k < I ? w_ih[(size_t)r * I + k] : w_hh[(size_t)r * H + (k - I)];
}

struct LstmWideXParams {
    const float *x, *wt;                                     // [R][I]; [I + H][G] (the first I rows are read)
    int64_t R;
    int I, G;
    float *xpre;                                             // [R][G]: sum_k W_ih[r][k] x[k], one fmaf chain from 0, k ascending
};

__global__ __launch_bounds__(kWideThreads) void lstm_wide_xpart_kernel(LstmWideXParams p)
{
    __shared__ float4 xs4[kWideMax * kWideXRows / 4];        // [k][kWideXRows]
    float *xs = reinterpret_cast<float *>(xs4);
    const int tid = threadIdx.x;
    const int64_t r0 = (int64_t)blockIdx.x * kWideXRows;
    const int nr = (int)min((int64_t)kWideXRows, p.R - r0);
    for (int i = tid; i < kWideXRows * p.I; i += blockDim.x) {
        const int row = i / p.I, k = i - row * p.I;
        xs[k * kWideXRows + row] = row < nr ? p.x[(r0 + row) * p.I + k] : 0.f;
    }
    __syncthreads();
    if (tid >= p.G) return;
    float acc[kWideXRows];
#pragma unroll
    for (int s = 0; s < kWideXRows; ++s) acc[s] = 0.f;
    const float *w = p.wt + tid;
#pragma unroll 4
    for (int k = 0; k < p.I; ++k) {
        const float wv = w[(size_t)k * p.G];
#pragma unroll
        for (int q = 0; q < kWideXRows / 4; ++q) {
            const float4 v = xs4[k * (kWideXRows / 4) + q];
            acc[4 * q] = __builtin_fmaf(wv, v.x, acc[4 * q]);
            acc[4 * q + 1] = __builtin_fmaf(wv, v.y, acc[4 * q + 1]);
            acc[4 * q + 2] = __builtin_fmaf(wv, v.z, acc[4 * q + 2]);
            acc[4 * q + 3] = __builtin_fmaf(wv, v.w, acc[4 * q + 3]);
        }
    }
#pragma unroll
    for (int s = 0; s < kWideXRows; ++s)
        if (s < nr) p.xpre[(r0 + s) * p.G + tid] = acc[s];
}

struct LstmWideParams {
    LstmSeriesParams s;                                      // the narrow launch's parameter block (x, w_ih, w_hh: not read by the kernel)
    const float *wht, *xpre;                                 // [H][G]: the W_hh rows of wt; [T B][G]
};

__global__ __launch_bounds__(kWideThreads) void lstm_series_wide_kernel(LstmWideParams q)
{
    static_assert(kWideSamples == 4, "the staged vectors are one float4 per k");
    extern __shared__ float4 wide_smem[];
    const LstmSeriesParams &p = q.s;
    const int H = p.H, G = 4 * H, tid = threadIdx.x;
    float *hb = reinterpret_cast<float *>(wide_smem);        // [H][4]: h_{t-1} of the workgroup's samples
    float *pre = hb + 4 * H;                                 // [4][G]
    const float4 *hb4 = wide_smem;
    const int b0 = blockIdx.x * kWideSamples, ns = min(kWideSamples, p.B - b0);
    const bool row = tid < G;                                // gate row tid; also (sample cs, unit cj) of the cell update
    const int cs = tid / H, cj = tid - cs * H;
    const bool cmine = row && cs < ns;
    const int cb = b0 + (cmine ? cs : 0);
    float c = 0.f;                                           // the cell state of (cs, cj), in a register for the whole launch
    if (row) hb[cj * 4 + cs] = cmine ? p.h0[(size_t)cb * H + cj] : 0.f;
    if (cmine) {
        c = p.c0[(size_t)cb * H + cj];
        if (p.cells) p.cells[(size_t)cb * H + cj] = c;
    }
    const float bias = row ? p.b_ih[tid] + p.b_hh[tid] : 0.f;
    auto fetch = [&](int t, float (&v)[kWideSamples]) {      // the x part of gate row tid, frame t: where the W_hh chain starts
#pragma unroll
        for (int s = 0; s < kWideSamples; ++s)
            v[s] = (row && s < ns) ? q.xpre[((size_t)t * p.B + b0 + s) * G + tid] : 0.f;
    };
    float xc[kWideSamples];
    fetch(0, xc);
    const float *w = q.wht + tid;
    for (int t = 0; t < p.T; ++t) {
        __syncthreads();                                     // h_{t-1} is complete; pre is free
        float xn[kWideSamples] = {0.f, 0.f, 0.f, 0.f};
        if (t + 1 < p.T) fetch(t + 1, xn);
        if (row) {
            float a0 = xc[0], a1 = xc[1], a2 = xc[2], a3 = xc[3];
#pragma unroll 8
            for (int k = 0; k < H; ++k) {
                const float wv = w[(size_t)k * G];
                const float4 v = hb4[k];
                a0 = __builtin_fmaf(wv, v.x, a0);
                a1 = __builtin_fmaf(wv, v.y, a1);
                a2 = __builtin_fmaf(wv, v.z, a2);
                a3 = __builtin_fmaf(wv, v.w, a3);
            }
            pre[tid] = a0 + bias; pre[G + tid] = a1 + bias; pre[2 * G + tid] = a2 + bias; pre[3 * G + tid] = a3 + bias;
        }
        __syncthreads();                                     // the pre-activations are there; h_{t-1} is free
        if (cmine) {
            const float *g4 = pre + cs * G;
            const float gi = sigmoid_f(g4[cj]), gf = sigmoid_f(g4[H + cj]), gg = tanhf(g4[2 * H + cj]), go = sigmoid_f(g4[3 * H + cj]);
            const float cn = __builtin_fmaf(gf, c, gi * gg);
            const float hn = go * tanhf(cn);
            c = cn;
            hb[cj * 4 + cs] = hn;
            p.series[t * p.series_stride_t + cb * p.series_stride_b + cj] = hn;
            if (p.gates) {
                float *o = p.gates + ((size_t)t * p.B + cb) * G;
                o[cj] = gi; o[H + cj] = gf; o[2 * H + cj] = gg; o[3 * H + cj] = go;
            }
            if (p.cells) p.cells[((size_t)(t + 1) * p.B + cb) * H + cj] = cn;
            if (t == p.T - 1) {
                if (p.h_out) p.h_out[(size_t)cb * H + cj] = hn;
                if (p.c_out) p.c_out[(size_t)cb * H + cj] = cn;
            }
        }
        if (p.series_cols > H) {
            const int np = p.series_cols - H;
            for (int i = tid; i < ns * np; i += blockDim.x) {
                const int s = i / np, j = H + (i - s * np);
                p.series[t * p.series_stride_t + (b0 + s) * p.series_stride_b + j] = p.pad_value;
            }
        }
#pragma unroll
        for (int s = 0; s < kWideSamples; ++s) xc[s] = xn[s];
    }
}

// The backward recurrence, lstm_series_bwd_kernel's formulas: thread (s, j) owns hidden unit j of sample s for all T frames
// (dh, dc in registers) and turns (dh_t, dc_t) into the unit's four pre-activation gradients; between two frames the same
// thread, as (gate chunk q = s, column j), sums W_hh[q H + rr][j] dpre(., q H + rr) over rr ascending for the four samples.
__global__ __launch_bounds__(kWideThreads) void lstm_series_bwd_wide_kernel(LstmSeriesBwdParams p)
{
    extern __shared__ float4 bwd_wide_smem[];
    const int H = p.H, G = 4 * H, tid = threadIdx.x;
    float *dp = reinterpret_cast<float *>(bwd_wide_smem);    // [G][4]: the frame's pre-activation gradients, sample-minor
    float *part = dp + kWideSamples * G;                     // [kWideGates chunks][kWideSamples][H]
    const int b0 = blockIdx.x * kWideSamples, ns = min(kWideSamples, p.B - b0);
    const int s = tid / H, j = tid - s * H;
    const bool act = tid < G, mine = act && s < ns;
    const int b = b0 + (mine ? s : 0);
    for (int i = tid; i < kWideSamples * G; i += blockDim.x) dp[i] = 0.f;         // (the columns of samples past the batch stay zero)
    __syncthreads();
    float dh = 0.f, dc = 0.f;                                // gradient arriving from frame t + 1
    auto fetch = [&](int t, float (&g)[4], float &ct, float &cp, float &ds) {
        const float *gp = p.gates + ((size_t)t * p.B + b) * G;
        g[0] = gp[j]; g[1] = gp[H + j]; g[2] = gp[2 * H + j]; g[3] = gp[3 * H + j];
        ct = p.cells[((size_t)(t + 1) * p.B + b) * H + j];
        cp = p.cells[((size_t)t * p.B + b) * H + j];
        ds = p.d_series[t * p.ds_stride_t + b * p.ds_stride_b + j];
    };
    float g[4] = {0.f, 0.f, 0.f, 0.f}, ct = 0.f, cp = 0.f, ds = 0.f;
    if (mine) fetch(p.T - 1, g, ct, cp, ds);
    const float *w = p.w_hh + (act ? (size_t)s * H * H + j : 0);         // row s H of W_hh, column j
    const float4 *d4 = bwd_wide_smem + (act ? s * H : 0);
    for (int t = p.T - 1; t >= 0; --t) {
        float gn[4] = {0.f, 0.f, 0.f, 0.f}, ctn = 0.f, cpn = 0.f, dsn = 0.f;
        if (mine && t > 0) fetch(t - 1, gn, ctn, cpn, dsn);
        if (mine) {
            const float gi = g[0], gf = g[1], gg = g[2], go = g[3];
            const float dht = dh + ds;
            const float tc = tanhf(ct);
            const float dct = __builtin_fmaf(dht * go, 1.0f - tc * tc, dc);
            const float d_i = dct * gg * gi * (1.0f - gi);
            const float d_f = dct * cp * gf * (1.0f - gf);
            const float d_g = dct * gi * (1.0f - gg * gg);
            const float d_o = dht * tc * go * (1.0f - go);
            dp[j * 4 + s] = d_i; dp[(H + j) * 4 + s] = d_f; dp[(2 * H + j) * 4 + s] = d_g; dp[(3 * H + j) * 4 + s] = d_o;
            float *o = p.dpre + ((size_t)t * p.B + b) * G;
            o[j] = d_i; o[H + j] = d_f; o[2 * H + j] = d_g; o[3 * H + j] = d_o;
            dc = dct * gf;
        }
        __syncthreads();                                     // the frame's gradients of every sample are in LDS; part is free
        if (act) {
            float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll 8
            for (int rr = 0; rr < H; ++rr) {
                const float wv = w[(size_t)rr * H];
                const float4 v = d4[rr];
                a0 = __builtin_fmaf(wv, v.x, a0);
                a1 = __builtin_fmaf(wv, v.y, a1);
                a2 = __builtin_fmaf(wv, v.z, a2);
                a3 = __builtin_fmaf(wv, v.w, a3);
            }
            float *o = part + (size_t)s * kWideSamples * H + j;
            o[0] = a0; o[H] = a1; o[2 * H] = a2; o[3 * H] = a3;
        }
        __syncthreads();                                     // the partial sums are there; dp is free
        if (mine) {                                          // the chunks' sums of sample s, ascending
            float acc = part[s * H + j];
#pragma unroll
            for (int c = 1; c < kWideGates; ++c) acc += part[(c * kWideSamples + s) * H + j];
            dh = acc;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) g[k] = gn[k];
        ct = ctn; cp = cpn; ds = dsn;
    }
    if (mine) {
        p.dh0[(size_t)b * H + j] = dh;
        p.dc0[(size_t)b * H + j] = dc;
    }
}

// The bias gradients behind the backward recurrence: out0[c] = out1[c] = sum_r dpre[r][c].  One workgroup per 64 columns, lanes
// over the columns (coalesced rows); wave w adds rows w, w + 16, ... ascending (sixteen loads in flight, added in row order), the
// sixteen partial sums meet in LDS and are added in ascending wave order: a fixed order, no atomics, no scratch, nothing to clear.
constexpr int kColSumWaves = 16;

__global__ __launch_bounds__(64 * kColSumWaves) void lstm_wide_colsum_kernel(const float *dpre, int64_t R, int G, float *out0, float *out1)
{
    __shared__ float red[kColSumWaves][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, c = blockIdx.x * 64 + lane;
    float sum = 0.f;
    if (c < G) {
        const float *q = dpre + c;
        int64_t r = w;
        for (; r + 15 * kColSumWaves < R; r += 16 * kColSumWaves) {
            float v[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) v[u] = q[(r + (int64_t)u * kColSumWaves) * G];
#pragma unroll
            for (int u = 0; u < 16; ++u) sum += v[u];
        }
        for (; r < R; r += kColSumWaves) sum += q[r * G];
    }
    red[w][lane] = sum;
    __syncthreads();
    if (w == 0 && c < G) {
        float s = red[0][lane];
#pragma unroll
        for (int i = 1; i < kColSumWaves; ++i) s += red[i][lane];
        out0[c] = s;
        out1[c] = s;
    }
}

}  // namespace ctc

extern "C" size_t ctc_amd_lstm_series_wide_scratch_bytes(int T, int B, int I, int H)
{
    if (T < 1 || B < 1 || I < 1 || H < 1 || !ctc::lstm_wide_shape_ok(T, B, I, H)) return 0;
    return ctc::lstm_wide_layout(T, B, I, H).total + ctc::kHeadBwdAlign;          // (the entry aligns the pointer itself)
}

// ctc_amd_lstm_series for 1 <= I, H <= 160: three launches on `stream` (the transposed weights, the x part of every row, the
// recurrence), bit for bit what T calls of ctc_amd_lstm_cell_step give.
extern "C" int ctc_amd_lstm_series_wide(const float *x, const float *h0, const float *c0,
                                        const float *w_ih, const float *w_hh, const float *b_ih, const float *b_hh,
                                        int T, int B, int I, int H,
                                        float *series, int64_t series_stride_t, int64_t series_stride_b, int series_cols, float pad_value,
                                        float *gates_out, float *cells_out, float *h_out, float *c_out,
                                        void *scratch, size_t scratch_bytes, void *stream)
{
    if (!x || !h0 || !c0 || !w_ih || !w_hh || !b_ih || !b_hh || !series || !scratch) return CTC_AMD_ERR_BAD_ARGUMENT;
    if (T < 1 || B < 1 || I < 1 || H < 1) return CTC_AMD_ERR_BAD_ARGUMENT;
    if (series_cols < H || series_stride_b < series_cols) return CTC_AMD_ERR_BAD_ARGUMENT;
    if (scratch_bytes < ctc_amd_lstm_series_wide_scratch_bytes(T, B, I, H)) return CTC_AMD_ERR_BAD_ARGUMENT;
    if (!ctc::lstm_wide_shape_ok(T, B, I, H)) return CTC_AMD_ERR_UNSUPPORTED_SHAPE;
    const ctc::LstmWideLayout L = ctc::lstm_wide_layout(T, B, I, H);
    char *base = ctc::scratch_base(scratch);
    float *wt = reinterpret_cast<float *>(base + L.wt), *xpre = reinterpret_cast<float *>(base + L.xpre);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int G = 4 * H;

    int rc = launch<ctc::lstm_wide_transpose_kernel>(dim3((unsigned)(((I + H) * G + 255) / 256)), dim3(256), 0, st, w_ih, w_hh, I, H, wt);
    if (rc) return rc;
    ctc::LstmWideXParams xp;
    xp.x = x; xp.wt = wt; xp.R = (int64_t)T * B; xp.I = I; xp.G = G; xp.xpre = xpre;
    rc = launch<ctc::lstm_wide_xpart_kernel>(dim3((unsigned)((xp.R + ctc::kWideXRows - 1) / ctc::kWideXRows)), dim3(ctc::wide_block(G)),
                                             0, st, xp);
    if (rc) return rc;
    ctc::LstmWideParams q;
    q.s = ctc::series_params(x, h0, c0, w_ih, w_hh, b_ih, b_hh, T, B, I, H, series, series_stride_t, series_stride_b, series_cols,
                             pad_value, gates_out, cells_out, h_out, c_out);
    q.wht = wt + (size_t)I * G; q.xpre = xpre;
    const size_t smem = ((size_t)ctc::kWideSamples * H + (size_t)ctc::kWideSamples * G) * sizeof(float);
    return launch<ctc::lstm_series_wide_kernel>(dim3((unsigned)((B + ctc::kWideSamples - 1) / ctc::kWideSamples)),
                                                dim3(ctc::wide_block(G)), smem, st, q);
}

// ctc_amd_lstm_series_backward for 1 <= H <= 160: one launch, no scratch.  Deterministic (fixed sum order, no atomics).
extern "C" int ctc_amd_lstm_series_backward_wide(const float *d_series, int64_t ds_stride_t, int64_t ds_stride_b,
                                                 const float *gates, const float *cells, const float *w_hh,
                                                 int T, int B, int H, float *dpre_out, float *dh0_out, float *dc0_out, void *stream)
{
    if (!d_series || !gates || !cells || !w_hh || !dpre_out || !dh0_out || !dc0_out) return CTC_AMD_ERR_BAD_ARGUMENT;
    if (T < 1 || B < 1 || H < 1) return CTC_AMD_ERR_BAD_ARGUMENT;
    if (H > ctc::kWideMax) return CTC_AMD_ERR_UNSUPPORTED_SHAPE;
    const ctc::LstmSeriesBwdParams p = ctc::series_bwd_params(d_series, ds_stride_t, ds_stride_b, gates, cells, w_hh, T, B, H,
                                                              dpre_out, dh0_out, dc0_out);
    const int G = 4 * H;
    const size_t smem = ((size_t)ctc::kWideSamples * G + (size_t)ctc::kWideGates * ctc::kWideSamples * H) * sizeof(float);
    return launch<ctc::lstm_series_bwd_wide_kernel>(dim3((unsigned)((B + ctc::kWideSamples - 1) / ctc::kWideSamples)),
                                                    dim3(ctc::wide_block(G)), smem, static_cast<hipStream_t>(stream), p);
}

// d_b_ih = d_b_hh = the column sums of dpre [rows][4H] (what ctc_amd_lstm_series_backward_wide wrote): one launch, deterministic.
extern "C" int ctc_amd_lstm_bias_grad_wide(const float *dpre, int64_t rows, int H, float *d_b_ih, float *d_b_hh, void *stream)
{
    if (!dpre || !d_b_ih || !d_b_hh) return CTC_AMD_ERR_BAD_ARGUMENT;
    if (rows < 1 || H < 1) return CTC_AMD_ERR_BAD_ARGUMENT;
    if (H > ctc::kWideMax) return CTC_AMD_ERR_UNSUPPORTED_SHAPE;
    const int G = 4 * H;
    return launch<ctc::lstm_wide_colsum_kernel>(dim3((unsigned)((G + 63) / 64)), dim3(64 * ctc::kColSumWaves), 0,
                                                static_cast<hipStream_t>(stream), dpre, rows, G, d_b_ih, d_b_hh);
}
