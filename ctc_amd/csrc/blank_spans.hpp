// One record per target label from the best path and the posteriors of the blank-CTC lattice
// (ctc_amd_blank_token_spans): where label j starts, where it ends, and the mean posterior of the frames
// the best path gives it.  Included by blank_align.hip behind the narrow and the wide read-outs, whose launches it
// strings together on one stream:
//   the best path             blank_table_gather_kernel + blank_align_kernel<K> (S <= 255) or blank_align_wide_kernel:
//                             path and score go to the caller's buffers, the back-pointers are dead afterwards
//   the posteriors' chains    blank_post_chain_kernel<K> on the SAME table (narrow: one gather serves both stages, see
//                             run_blank_spans) or the gather again, with c_t, + blank_post_wide_chain_kernel:
//                             alpha' / beta' rows where the back-pointers were, nll to the caller
//   blank_post_conf_kernel<K> blank_post_gamma_kernel's grid and row arithmetic (post_row_terms, post_row_inv), but of
//                             each row only gamma[b, t, path[b, t]] is stored: frame_conf [B,T].  gamma itself is
//                             never written.
//   blank_span_kernel         one workgroup per sample: span boundaries from the path, then one lane per label sums its
//                             frames in ascending t and divides once.
// Launch order is the only synchronisation: no workgroup waits on another, nothing polls, no status bit.
#pragma once

namespace ctc {

constexpr int kSpanThreads = 512;
constexpr int kSpanMaxLabels = 1024;            // label columns a sample's boundaries take in LDS (S <= 1023)
constexpr int kSpanAhead = 4;                   // frame confidences a label's lane loads ahead of its sum

struct SpanParams {
    PostParams p;                               // p.a: inputs, shape, path, score; al / be; nll
    float *frame_conf;                          // [B][T]
    int32_t *start, *end;                       // [B][S]
    float *conf;                                // [B][S]
};

// grid (ceil(T / (4 * kPostRows)), B), as blank_post_gamma_kernel: wave w of block x takes rows t0 .. t0 + kPostRows - 1,
// state s = lane + 64 k.  frame_conf[b, t] = z * inv of state path[b, t]: the value blank_post_gamma_kernel stores
// there (the same masked loads, the same post_row_terms and post_row_inv); 0 where path is -1.  Every (b, t < T) is written.
template <int K>
__global__ __launch_bounds__(kPostThreads) void blank_post_conf_kernel(PostParams p, float *frame_conf)
{
    const int b = blockIdx.y, lane = lane_id(), T = p.a.T;
    const int t0 = (blockIdx.x * (kPostThreads / kWave) + wave_id()) * kPostRows;
    if (t0 >= T) return;
    int Tb, L;
    const bool ok = align_sample(p.a, b, Tb, L);
    const bool feasible = ok && p.nll[b] < __builtin_inff();     // (+inf: no alignment, bad lengths included)
    const int n = 2 * L + 1;
    const int64_t r0 = (int64_t)b * T + t0;
    int st[kPostRows];                                            // the path's states of the four rows (wave-uniform)
#pragma unroll
    for (int r = 0; r < kPostRows; ++r) st[r] = p.a.path[r0 + min(r, T - 1 - t0)];
    const float *al = p.al + r0 * p.NSP, *be = p.be + r0 * p.NSP;
    float z[kPostRows][K], m[kPostRows];
#pragma unroll
    for (int r = 0; r < kPostRows; ++r) {
        const bool live = feasible && t0 + r < Tb;
        m[r] = -__builtin_inff();
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int s = lane + kWave * k;
            z[r][k] = live && s < n ? al[r * p.NSP + s] + be[r * p.NSP + s] : -__builtin_inff();
            m[r] = fmaxf(m[r], z[r][k]);
        }
    }
    float sum[kPostRows];
    post_row_terms<K>(z, m, sum);
    float *out = frame_conf + r0;
#pragma unroll
    for (int r = 0; r < kPostRows; ++r) {
        if (t0 + r >= T) break;
        const float inv = post_row_inv(sum[r]);
        // state st sits in lane st % 64 at k = st / 64; a select over the registers on a wave-uniform k (an indexed
        // access would go through a stack copy of z[]); st = -1 matches no k
        float v = 0.f;
#pragma unroll
        for (int k = 0; k < K; ++k) v = (st[r] >> 6) == k ? z[r][k] : v;
        if (lane == (st[r] & (kWave - 1))) out[r] = st[r] >= 0 ? v * inv : 0.f;
    }
}

// grid B, block kSpanThreads.  Pass 1, one lane per frame: frame t opens the span of label (s - 1) / 2 when its state s is
// odd and differs from the state of frame t - 1, and closes it when s differs from the state of frame t + 1 or t is the
// last frame.  The path is monotone, so a label's frames are contiguous and each boundary has one writer.  Pass 2, one
// lane per label: conf = (sum of frame_conf over start .. end - 1, from 0.0f, ascending t, fp32) / float(end - start),
// one correctly rounded division.  Labels the path does not visit (j >= L_b, samples without an alignment or with lengths
// out of contract: their path is all -1) get -1 / -1 / 0.  Every (b, j < S) is written.
__global__ __launch_bounds__(kSpanThreads) void blank_span_kernel(AlignParams p, const float *frame_conf, int32_t *start,
                                                                  int32_t *end, float *conf)
{
    __shared__ int s_start[kSpanMaxLabels], s_end[kSpanMaxLabels];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int S = min(p.S, kSpanMaxLabels);                       // (the entry has checked: memory safety)
    int Tb, L;
    align_sample(p, b, Tb, L);                                    // lengths out of contract: Tb = 0, nothing opens
    for (int j = tid; j < S; j += kSpanThreads) {
        s_start[j] = -1;
        s_end[j] = -1;
    }
    __syncthreads();
    const int32_t *path = p.path + (int64_t)b * p.T;
    for (int t = tid; t < Tb; t += kSpanThreads) {
        const int s = path[t];
        const int j = (s - 1) >> 1;
        if (s > 0 && (s & 1) && j < S) {
            if (t == 0 || path[t - 1] != s) s_start[j] = t;
            if (t == Tb - 1 || path[t + 1] != s) s_end[j] = t + 1;
        }
    }
    __syncthreads();
    const float *fc = frame_conf + (int64_t)b * p.T;
    for (int j = tid; j < S; j += kSpanThreads) {
        int t0 = s_start[j], t1 = s_end[j];
        float c = 0.f;
        if (t0 >= 0 && t1 > t0) {
            float acc = 0.0f;
            for (int t = t0; t < t1; t += kSpanAhead) {          // kSpanAhead loads in flight, added in ascending t
                float v[kSpanAhead];
#pragma unroll
                for (int i = 0; i < kSpanAhead; ++i) v[i] = fc[min(t + i, t1 - 1)];
#pragma unroll
                for (int i = 0; i < kSpanAhead; ++i)
                    if (t + i < t1) acc += v[i];
            }
            c = __fdiv_rn(acc, (float)(t1 - t0));
        } else {
            t0 = t1 = -1;
        }
        const int64_t o = (int64_t)b * p.S + j;
        start[o] = t0;
        end[o] = t1;
        conf[o] = c;
    }
}

// the two launches behind the chains
template <int K>
static int launch_blank_conf_spans(const SpanParams &q, hipStream_t s)
{
    const AlignParams &p = q.p.a;
    const int rows = (kPostThreads / kWave) * kPostRows;
    const int rc = launch<blank_post_conf_kernel<K>>(dim3((p.T + rows - 1) / rows, p.B), dim3(kPostThreads), 0, s, q.p,
                                                     q.frame_conf);
    if (rc) return rc;
    return launch<blank_span_kernel>(dim3(p.B), dim3(kSpanThreads), 0, s, p, q.frame_conf, q.start, q.end, q.conf);
}

// S <= 255.  ONE gather serves both stages: run_blank_align<K> and blank_post_layout<K> put the table at the same
// address with the same pitch (workspace + 256, align_row_pitch(K)), both stages would fill it with
// the same blank_table_gather_kernel from the same AlignParams, and blank_align_kernel<K> only reads it -- its back-pointers
// are in LDS and, beyond, in `spill` BEHIND the table.  The alpha' rows start where `spill` started: the back-pointers
// are dead once the path is out, and the stream orders the chains behind the walk back.
template <int K>
static int run_blank_spans(SpanParams &q, hipStream_t s)
{
    AlignParams &p = q.p.a;
    int rc = run_blank_align<K>(p, s);                            // gather + scan and walk back: path, score
    if (rc) return rc;
    const float *table = p.em;
    rc = blank_post_layout<K>(q.p);
    if (rc) return rc;
    if (p.em != table) return CTC_AMD_ERR_UNSUPPORTED_SHAPE;      // (the two layouts have drifted apart)
    rc = launch<blank_post_chain_kernel<K>>(dim3(p.B), dim3(2 * kWave), 0, s, q.p);
    if (rc) return rc;
    return launch_blank_conf_spans<K>(q, s);
}

// 256 <= S <= 1023.  Two gathers: the posteriors' table carries the row maximum c_t in a padding column that the best
// path's gather (CMAX = false) fills with -inf.  The second
// gather rewrites the table in place; the alpha' / beta' rows then cover the best path's back-pointer words.
static int run_blank_spans_wide(SpanParams &q, hipStream_t s)
{
    int rc = run_blank_align_wide(q.p.a, s);                      // gather + scan and walk back: path, score
    if (rc) return rc;
    PostWideParams w;
    rc = blank_post_wide_layout(q.p, w);
    if (rc) return rc;
    return with_constant<2, 3, 4>(w.W, [&](auto n) {
        constexpr int W = decltype(n)::value;
        const int crc = launch_blank_post_wide_chains<W>(w, s);
        return crc ? crc : launch_blank_conf_spans<W * kWideAlignK>(q, s);
    });
}

}  // namespace ctc
