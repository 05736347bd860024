// CTC evaluation on the device, gfx950: per-frame decisions -> tokens with frame spans
// (ctc_amd_collapse_frames), tokens against the reference transcript (ctc_amd_edit_distance).  Both are integer-exact;
// neither allocates, synchronises, uses atomics or lets one workgroup wait for another: safe under stream capture,
// deterministic.  Every global store is a plain C++ store.
//
//   collapse_frames_kernel    one 256-thread workgroup per sample.  All waves stage the sample's T_b labels in LDS (the
//                             only read of `frames`: any strides, nothing at t >= T_b).  Wave 0 scans them in 64-frame
//                             chunks: a frame opens a run when it differs from the frame before it and closes one when it
//                             differs from the frame behind it; the token index of a kept opening / closing is the
//                             number of kept openings / closings in front of it -- a ballot and a prefix count inside
//                             the chunk, a running count across chunks (a run may open in one chunk and close in a later
//                             one: two counts).  The first min(W, T) tokens' first and last frames go to LDS.  Then one
//                             thread per output column writes tokens / start / end / conf of that column -- the token's
//                             record, or the padding -- so every element is written exactly once; the lane of a token
//                             adds its own frames' confidences in ascending t (the order is the contract).
//   edit_distance_kernel<K>   one wave per sample, four samples per workgroup.  The DP row over the reference positions
//                             j = 1..M lives in registers, K consecutive cells per lane (64 K >= M).  Per hypothesis
//                             token: t[j] = min(up + 1, diag + cost) in every cell at once, then the dependency inside
//                             the row, d[j] = min(t[j], d[j-1] + 1), in closed form: d[j] = j + min_{j' <= j} (t[j'] - j')
//                             with t[0] = i -- a running minimum inside the lane, an exclusive DPP prefix minimum over
//                             the 64 lane totals.  The hypothesis is read 64 tokens at a time (one per lane) and handed
//                             out with v_readlane.
#include "common.hpp"
#include "launch.hpp"

namespace ctc {

constexpr int kCollapseThreads = 256;
constexpr int kEditWaves = 4;                   // samples (waves) per workgroup of the edit distance
constexpr int kEditMaxRef = 1023;               // M: the project's one limit on target widths
constexpr int kSpanLoadsAhead = 4;              // frame confidences a token's lane loads ahead of its sum

struct CollapseParams {
    const void *frames;                         // [B][T] labels through (stride_b, stride_t), int32 or the low words of int64
    int frames64;
    int64_t sb, st;
    const int64_t *in_len;
    const float *frame_conf;                    // through (csb, cst), or nullptr (then conf is nullptr too)
    int64_t csb, cst;
    int T, B, blank, W, WC;                     // WC = min(W, T): tokens whose spans are kept
    int32_t *tokens;                            // [B][W]
    int64_t *out_len;                           // [B]
    int32_t *start, *end;                       // [B][W]
    float *conf;                                // [B][W] or nullptr
};

__global__ __launch_bounds__(kCollapseThreads) void collapse_frames_kernel(CollapseParams p)
{
    extern __shared__ float4 smem_raw[];
    int *lab = reinterpret_cast<int *>(smem_raw);               // [T]
    int *tfirst = lab + p.T;                                    // [WC]
    int *tlast = tfirst + p.WC;                                 // [WC]
    int *count = tlast + p.WC;                                  // [1]
    const int b = blockIdx.x, tid = threadIdx.x;
    const int64_t Tb64 = p.in_len[b];
    const int Tb = Tb64 < 0 ? 0 : (Tb64 > p.T ? p.T : (int)Tb64);       // (memory safety: never beyond the tensor)

    for (int t = tid; t < Tb; t += kCollapseThreads) lab[t] = load_label(p.frames, p.frames64, (int64_t)b * p.sb + (int64_t)t * p.st);
    __syncthreads();

    if (wave_id() == 0) {
        const int lane = lane_id();
        const unsigned long long below = (1ull << lane) - 1ull;
        int opened = 0, closed = 0;                             // kept runs opened / closed in front of this chunk
        for (int t0 = 0; t0 < Tb; t0 += kWave) {
            const int t = t0 + lane;
            bool open = false, close = false;
            if (t < Tb) {
                const int cur = lab[t];
                const bool keep = p.blank < 0 || cur != p.blank;
                open = keep && (t == 0 || lab[t - 1] != cur);
                close = keep && (t == Tb - 1 || lab[t + 1] != cur);
            }
            const unsigned long long mo = __ballot(open), mc = __ballot(close);
            const int io = opened + __popcll(mo & below), ic = closed + __popcll(mc & below);
            if (open && io < p.WC) tfirst[io] = t;
            if (close && ic < p.WC) tlast[ic] = t;
            opened += __popcll(mo);
            closed += __popcll(mc);
        }
        if (lane == 0) {
            count[0] = opened;
            p.out_len[b] = opened;                              // the true count, also beyond W
        }
    }
    __syncthreads();

    const int n = min(count[0], p.WC);
    for (int i = tid; i < p.W; i += kCollapseThreads) {
        int tok = -1, t0 = -1, t1 = -1;
        float c = 0.f;
        if (i < n) {
            t0 = tfirst[i];
            t1 = tlast[i];
            tok = lab[t0];
            if (p.conf) {
                const float *fc = p.frame_conf + (int64_t)b * p.csb;
                float acc = 0.0f;
                for (int t = t0; t <= t1; t += kSpanLoadsAhead) {           // loads in flight, added in ascending t
                    float v[kSpanLoadsAhead];
#pragma unroll
                    for (int k = 0; k < kSpanLoadsAhead; ++k) v[k] = fc[(int64_t)min(t + k, t1) * p.cst];
#pragma unroll
                    for (int k = 0; k < kSpanLoadsAhead; ++k)
                        if (t + k <= t1) acc += v[k];
                }
                c = __fdiv_rn(acc, (float)(t1 - t0 + 1));
            }
        }
        const int64_t o = (int64_t)b * p.W + i;
        p.tokens[o] = tok;
        p.start[o] = t0;
        p.end[o] = t1;
        if (p.conf) p.conf[o] = c;
    }
}

// DPP on integers: lanes selected by CTRL / ROW_MASK read `v` of their source lane, the others get `ident`
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ int dpp_i(int v, int ident)
{
    return __builtin_amdgcn_update_dpp(ident, v, CTRL, ROW_MASK, 0xf, false);
}
constexpr int kRowShr1 = 0x111, kRowShr2 = 0x112, kRowShr4 = 0x114, kRowShr8 = 0x118, kWaveShr1 = 0x138;

// lane i <- min over lanes 0..i-1, `first` in lane 0 and folded into every lane: shifts inside the 16-lane rows, then the
// rows' last lanes handed to the rows behind them
__device__ __forceinline__ int wave_prefix_min_excl(int v, int first)
{
    constexpr int top = 0x7fffffff;
    v = min(v, dpp_i<kRowShr1, 0xf>(v, top));
    v = min(v, dpp_i<kRowShr2, 0xf>(v, top));
    v = min(v, dpp_i<kRowShr4, 0xf>(v, top));
    v = min(v, dpp_i<kRowShr8, 0xf>(v, top));
    v = min(v, dpp_i<kRowBcast15, 0xa>(v, top));
    v = min(v, dpp_i<kRowBcast31, 0xc>(v, top));
    return min(dpp_i<kWaveShr1, 0xf>(v, top), first);
}

struct EditParams {
    const void *hyp, *ref;                      // [B][N], [B][M] through their batch strides, unit stride inside a row
    int hyp64, ref64;
    int64_t hsb, rsb;
    const int64_t *hyp_len, *ref_len;
    int B, N, M;
    int32_t *dist;                              // [B]
};

template <int K>
__global__ __launch_bounds__(kEditWaves * kWave) void edit_distance_kernel(EditParams p)
{
    const int b = blockIdx.x * kEditWaves + wave_id(), lane = lane_id();
    if (b >= p.B) return;                                       // (whole waves; the kernel has no barrier)
    const int64_t N64 = p.hyp_len[b], M64 = p.ref_len[b];
    const int Nb = N64 < 0 ? 0 : (N64 > p.N ? p.N : (int)N64);  // (memory safety: never beyond the tensors)
    const int Mb = M64 < 0 ? 0 : (M64 > p.M ? p.M : (int)M64);
    const int j0 = lane * K + 1;                                // this lane's cells: j0 .. j0 + K - 1
    int r[K], d[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        r[k] = j0 + k <= Mb ? load_label(p.ref, p.ref64, (int64_t)b * p.rsb + (j0 + k - 1)) : 0;
        d[k] = j0 + k;                                          // row 0: d[0][j] = j
    }
    for (int i0 = 0; i0 < Nb; i0 += kWave) {
        const int mine = i0 + lane < Nb ? load_label(p.hyp, p.hyp64, (int64_t)b * p.hsb + i0 + lane) : 0;
        const int steps = min(kWave, Nb - i0);
        for (int s = 0; s < steps; ++s) {
            const int h = __builtin_amdgcn_readlane(mine, s);
            const int i = i0 + s + 1;                           // the row being formed; d[i][0] = i
            int diag = dpp_i<kWaveShr1, 0xf>(d[K - 1], i - 1);  // d[i-1][j0-1]; lane 0: d[i-1][0]
            int u[K];
            int run = 0x7fffffff;
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const int t = min(d[k] + 1, diag + (r[k] != h ? 1 : 0));
                diag = d[k];
                run = min(run, t - (j0 + k));
                u[k] = run;
            }
            const int before = wave_prefix_min_excl(run, i);
#pragma unroll
            for (int k = 0; k < K; ++k) d[k] = min(u[k], before) + (j0 + k);
        }
    }
    if (Mb == 0) {
        if (lane == 0) p.dist[b] = Nb;
    } else if (lane == (Mb - 1) / K) {
        int v = 0;
#pragma unroll
        for (int k = 0; k < K; ++k) v = (k == (Mb - 1) % K) ? d[k] : v;
        p.dist[b] = v;
    }
}

}  // namespace ctc

using namespace ctc;

extern "C" int ctc_amd_collapse_frames(const void *frames, int frames_i64, int64_t stride_b, int64_t stride_t,
                                       const int64_t *in_len,
                                       const float *frame_conf, int64_t conf_stride_b, int64_t conf_stride_t,
                                       int T, int B, int blank, int W,
                                       int32_t *tokens, int64_t *out_len, int32_t *start, int32_t *end, float *conf,
                                       void *stream)
{
    if (!frames || !in_len || !tokens || !out_len || !start || !end) return CTC_AMD_ERR_BAD_ARGUMENT;
    if ((frame_conf == nullptr) != (conf == nullptr)) return CTC_AMD_ERR_BAD_ARGUMENT;
    if (T < 1 || B < 1 || W < 1) return CTC_AMD_ERR_BAD_ARGUMENT;
    CollapseParams p;
    p.frames = frames; p.frames64 = frames_i64 != 0;
    p.sb = stride_b; p.st = stride_t;
    p.in_len = in_len;
    p.frame_conf = frame_conf; p.csb = conf_stride_b; p.cst = conf_stride_t;
    p.T = T; p.B = B; p.blank = blank; p.W = W; p.WC = W < T ? W : T;
    p.tokens = tokens; p.out_len = out_len; p.start = start; p.end = end; p.conf = conf;
    const size_t smem = ((size_t)T + 2 * (size_t)p.WC + 1) * 4;
    if (smem > kMaxLds) return CTC_AMD_ERR_UNSUPPORTED_SHAPE;
    return launch<collapse_frames_kernel>(dim3(B), dim3(kCollapseThreads), smem, static_cast<hipStream_t>(stream), p);
}

extern "C" int ctc_amd_edit_distance(const void *hyp, int hyp_i64, int64_t hyp_stride_b, const int64_t *hyp_len,
                                     const void *ref, int ref_i64, int64_t ref_stride_b, const int64_t *ref_len,
                                     int B, int N, int M, int32_t *dist, void *stream)
{
    if (!hyp_len || !ref_len || !dist) return CTC_AMD_ERR_BAD_ARGUMENT;
    if (B < 1 || N < 0 || M < 0) return CTC_AMD_ERR_BAD_ARGUMENT;
    if ((!hyp && N > 0) || (!ref && M > 0)) return CTC_AMD_ERR_BAD_ARGUMENT;     // (an empty tensor has no address)
    if (M > kEditMaxRef) return CTC_AMD_ERR_UNSUPPORTED_SHAPE;
    EditParams p;
    p.hyp = hyp; p.hyp64 = hyp_i64 != 0; p.hsb = hyp_stride_b; p.hyp_len = hyp_len;
    p.ref = ref; p.ref64 = ref_i64 != 0; p.rsb = ref_stride_b; p.ref_len = ref_len;
    p.B = B; p.N = N; p.M = M;
    p.dist = dist;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid((B + kEditWaves - 1) / kEditWaves), block(kEditWaves * kWave);
    if (M <= 1 * kWave) return launch<edit_distance_kernel<1>>(grid, block, 0, s, p);
    if (M <= 2 * kWave) return launch<edit_distance_kernel<2>>(grid, block, 0, s, p);
    if (M <= 4 * kWave) return launch<edit_distance_kernel<4>>(grid, block, 0, s, p);
    if (M <= 8 * kWave) return launch<edit_distance_kernel<8>>(grid, block, 0, s, p);
    return launch<edit_distance_kernel<16>>(grid, block, 0, s, p);
}
