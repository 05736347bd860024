// The HEAD of the producer for batches beyond one workgroup's 256 rows: ctc_amd_head_forward_wide and
// ctc_amd_head_backward_wide.  Included at the end of producer.hip (HeadParams, head_dot / head_linear / head_invstd /
// head_bn_y / head_bn_relu / head_column_total, HeadBwdRowsParams, the layout and the products / reduce launches of the head's
// backward are that file's, unchanged: every rounding of an element is the narrow path's own).  So is the host code the two
// widths share: head_forward_params (the forward entries' checks and HeadParams), head_shape_ok (one shape rule, the bound on B
// its argument), head_backward_enqueue (the whole backward entry but the rows launch), scratch_base / scratch_up.
//
// BatchNorm's batch statistics are taken over the B rows of ONE frame, and B rows no longer fit one workgroup, so the sums over
// a frame's rows cross workgroups -- at a kernel boundary, never inside a launch:
//   forward, eval   ONE launch.  grid (frame, row block of 256, group of N <= 3 column tiles): wave w of a block owns rows
//                   256 rb + 16 w .. + 15 and all N column tiles of its group (head_dot<N>: the feature row is read once per
//                   group, not once per 16 columns), then head_kernel's epilogue on the running statistics.  No cross-row term.
//   forward, train  TWO launches.  The product launch (same grid) writes lin [T][B][C] (to linear_out, else to the scratch) and
//                   the column sums of its 256 rows, psum [T][NB][CP] (head_column_total: lane quarters, then waves).  The
//                   statistics launch, grid (frame, column tile), walks the frame: mean = (psum added over the row blocks
//                   ascending) / B; the centred second moment over lin (per lane: row blocks ascending, then its four rows;
//                   then head_column_total); var = moment / B (biased), invstd = head_invstd; BatchNorm, ReLU, mask, out.
//                   At B <= 256 (one row block) these are head_kernel's own sums in head_kernel's own order.
//   backward        head_bwd_rows_kernel's row pass with the frame's rows walked by one workgroup per (frame, column tile):
//                   pass 1 sums dy and dy xhat per lane over the row blocks ascending (then head_column_total), pass 2 (train
//                   mode only: eval has no cross-row term and writes dlin in pass 1) writes dlin and sums it.  ONE launch,
//                   no partials in memory; it leaves dlin [T B][CP] and part [3][T][CP] as head_bwd_rows_kernel does, and
//                   head_bwd_products_kernel / head_bwd_reduce_kernel follow as they are: two launches in all, three when the
//                   weight gradient splits its rows (T B > 128).
// No atomics; every order is fixed by (T, B, K, C) alone.  Only __syncthreads() in block-uniform control flow.
#pragma once

namespace ctc {

constexpr int kHeadWideRows = 256;                           // rows of a row block: 16 waves of 16 rows
constexpr int kHeadWideMaxBatch = 65536;                     // B beyond this: CTC_AMD_ERR_UNSUPPORTED_SHAPE (256 row blocks in grid.y)
constexpr int kHeadWideMaxTiles = 3;                         // column tiles a wave takes (lstm_forward_kernel's bound on N)

// column tiles per wave and groups of them: NG = ceil(CT / 3), N = ceil(CT / NG) (CT = 10: 4 groups of 3, 3, 3, 1)
inline void head_wide_groups(int C, int &N, int &NG)
{
    const int CT = (C + 15) / 16;
    NG = (CT + kHeadWideMaxTiles - 1) / kHeadWideMaxTiles;
    N = (CT + NG - 1) / NG;
}

// (what the entries take of (T, B, K, C): head_shape_ok, the narrow entries' rule, with kHeadWideMaxBatch for the bound on B)

struct HeadWideLayout {                                      // byte offsets into the (aligned) scratch of the forward
    size_t lin, psum, total;
    int CP, NB;
};

inline HeadWideLayout head_wide_layout(int T, int B, int C)
{
    HeadWideLayout L;
    L.CP = 16 * ((C + 15) / 16);
    L.NB = (B + kHeadWideRows - 1) / kHeadWideRows;
    L.lin = 0;
    L.psum = scratch_up((size_t)T * B * C * sizeof(float));
    L.total = L.psum + scratch_up((size_t)T * L.NB * L.CP * sizeof(float));
    return L;
}

inline unsigned head_wide_block(int B) { return 64u * (unsigned)((B < kHeadWideRows ? B + 15 : kHeadWideRows) / 16); }

// The product of one row block with one group of N column tiles.  Eval mode (p.rmean): head_kernel's epilogue, the whole head.
// Train mode: lin and the block's column sums psum [T][NB][CP] (a pad column gets 0).
template <int N, typename E>
__global__ __launch_bounds__(1024) void head_wide_product_kernel(HeadParams p, float *psum, int CP)
{
    __shared__ float red[16][16];                            // [wave][column of the tile]
    const int t = blockIdx.x, rb = blockIdx.y, grp = blockIdx.z, tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    const int fr = lane & 15, fq = lane >> 4;
    const int NW = blockDim.x >> 6, NB = gridDim.y;
    const int row0 = kHeadWideRows * rb + 16 * w;            // operands clamped like head_kernel's: the padding is masked out below
    const int arow = min(row0 + fr, p.B - 1);
    const E *ap = static_cast<const E *>(p.feat) + (int64_t)t * p.fst + (int64_t)arow * p.fsb + 4 * fq;
    const float *bp[N];
    head_f4 acc[N];
#pragma unroll
    for (int n = 0; n < N; ++n) {
        const int bcol = min(16 * (N * grp + n) + fr, p.C - 1);
        bp[n] = p.w + (int64_t)bcol * p.K + 4 * fq;
        acc[n] = head_f4{0.f, 0.f, 0.f, 0.f};
    }
    head_dot<N>(ap, bp, p.K >> 4, acc);                      // K is a multiple of 16 (checked by the host)
    bool rowok[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) rowok[j] = row0 + 4 * fq + j < p.B;
#pragma unroll
    for (int n = 0; n < N; ++n) {
        // acc[n][j] = Linear output (without bias) of batch row row0 + 4 fq + j, column 16 (N grp + n) + fr
        const int col = 16 * (N * grp + n) + fr;
        if (col - fr >= p.C) continue;                       // a tile past the last one (uniform over the workgroup)
        const bool colok = col < p.C;
        const float bias = colok ? p.bias[col] : 0.f;
        float x[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) x[j] = head_linear(acc[n][j], bias);
        if (p.rmean) {                                       // eval mode
            const float mean = colok ? p.rmean[col] : 0.f, inv = head_invstd(colok ? p.rvar[col] : 1.f, p.eps);
            const float g = colok ? p.gamma[col] : 0.f, be = colok ? p.beta[col] : 0.f;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int b = row0 + 4 * fq + j;
                if (!rowok[j] || !colok) continue;
                const int64_t i = ((int64_t)t * p.B + b) * p.C + col;
                if (p.lin) p.lin[i] = x[j];
                float y = head_bn_relu(x[j], mean, inv, g, be);
                if (p.mask) y *= p.mask[i];
                p.out[(int64_t)t * p.ost + (int64_t)b * p.osb + col] = y;
            }
            continue;
        }
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) s += rowok[j] ? x[j] : 0.f;
        const float tot = head_column_total(s, red, w, fr, fq, NW);
        if (w == 0 && fq == 0) psum[((int64_t)t * NB + rb) * CP + col] = colok ? tot : 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int b = row0 + 4 * fq + j;
            if (rowok[j] && colok) p.lin[((int64_t)t * p.B + b) * p.C + col] = x[j];
        }
    }
}

// Train mode behind the product launch: the statistics of (frame, column) over all B rows and the epilogue.  p.lin is what the
// product launch wrote (linear_out or the scratch).
__global__ __launch_bounds__(1024) void head_wide_stats_kernel(HeadParams p, const float *psum, int CP, int NB)
{
    __shared__ float red[16][16];
    const int t = blockIdx.x, n = blockIdx.y, tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    const int fr = lane & 15, fq = lane >> 4;
    const int NW = blockDim.x >> 6;
    const int col = 16 * n + fr;                             // (< CP)
    const bool colok = col < p.C;
    float s = 0.f;
    for (int rb = 0; rb < NB; ++rb) s += psum[((int64_t)t * NB + rb) * CP + col];
    const float mean = s / (float)p.B;
    const float *lin = p.lin + (int64_t)t * p.B * p.C + col;
    float q = 0.f;
    for (int rb = 0; rb < NB; ++rb) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int b = kHeadWideRows * rb + 16 * w + 4 * fq + j;
            if (b < p.B && colok) {
                const float x = lin[(int64_t)b * p.C];
                q += (x - mean) * (x - mean);
            }
        }
    }
    const float var = head_column_total(q, red, w, fr, fq, NW) / (float)p.B;     // biased, what the normalisation uses
    const float inv = head_invstd(var, p.eps);
    if (!colok) return;                                      // (no barrier below)
    if (w == 0 && fq == 0) {
        if (p.smean) p.smean[(int64_t)t * p.C + col] = mean;
        if (p.svar) p.svar[(int64_t)t * p.C + col] = var;
        if (p.sinv) p.sinv[(int64_t)t * p.C + col] = inv;
    }
    const float g = p.gamma[col], be = p.beta[col];
    for (int rb = 0; rb < NB; ++rb) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int b = kHeadWideRows * rb + 16 * w + 4 * fq + j;
            if (b >= p.B) continue;
            float y = head_bn_relu(lin[(int64_t)b * p.C], mean, inv, g, be);
            if (p.mask) y *= p.mask[((int64_t)t * p.B + b) * p.C + col];
            p.out[(int64_t)t * p.ost + (int64_t)b * p.osb + col] = y;
        }
    }
}

// head_bwd_rows_kernel for any B: one workgroup per (frame, column tile) walks the frame's row blocks.
__global__ __launch_bounds__(1024) void head_wide_bwd_rows_kernel(HeadBwdRowsParams p)
{
    __shared__ float red[16][16];
    const int t = blockIdx.x, n = blockIdx.y, tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    const int fr = lane & 15, fq = lane >> 4;
    const int NW = blockDim.x >> 6, NB = (p.B + kHeadWideRows - 1) / kHeadWideRows;
    const int col = 16 * n + fr;                             // (< CP)
    const bool colok = col < p.C, train = p.smean != nullptr;
    float mean = 0.f, inv = 0.f, g = 0.f, be = 0.f;
    if (colok) {
        mean = train ? p.smean[(int64_t)t * p.C + col] : p.rmean[col];
        inv = train ? p.sinv[(int64_t)t * p.C + col] : head_invstd(p.rvar[col], p.eps);
        g = p.gamma[col];
        be = p.beta[col];
    }
    // dy and xhat of batch row b of this lane's column (zero in a pad column)
    auto row = [&](int b, float &dy, float &xh) {
        dy = 0.f; xh = 0.f;
        if (!colok) return;
        const int64_t i = ((int64_t)t * p.B + b) * p.C + col;
        const float x = p.lin[i];
        float d = p.dout[(int64_t)t * p.dst + (int64_t)b * p.dsb + col];
        if (p.mask) d *= p.mask[i];
        xh = (x - mean) * inv;
        dy = head_bn_y(x, mean, inv, g, be) > 0.f ? d : 0.f;
    };
    float sb = 0.f, sg = 0.f, sd = 0.f;
    for (int rb = 0; rb < NB; ++rb) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int b = kHeadWideRows * rb + 16 * w + 4 * fq + j;
            if (b >= p.B) continue;
            float dy, xh;
            row(b, dy, xh);
            sb += dy;
            sg += dy * xh;
            if (!train) {                                    // eval mode: no cross-row term
                const float dl = colok ? dy * g * inv : 0.f;
                sd += dl;
                p.dlin[((int64_t)t * p.B + b) * p.CP + col] = dl;    // the pad columns get their zeros here
            }
        }
    }
    const float dbeta = head_column_total(sb, red, w, fr, fq, NW);
    const float dgamma = head_column_total(sg, red, w, fr, fq, NW);
    if (train) {
        const float mb = dbeta / (float)p.B, mg = dgamma / (float)p.B;
        for (int rb = 0; rb < NB; ++rb) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int b = kHeadWideRows * rb + 16 * w + 4 * fq + j;
                if (b >= p.B) continue;
                float dy, xh;
                row(b, dy, xh);
                const float dl = colok ? inv * g * (dy - mb - xh * mg) : 0.f;
                sd += dl;
                p.dlin[((int64_t)t * p.B + b) * p.CP + col] = dl;
            }
        }
    }
    const float dsum = head_column_total(sd, red, w, fr, fq, NW);
    if (w == 0 && fq == 0) {
        const int64_t TC = (int64_t)p.T * p.CP, i = (int64_t)t * p.CP + col;
        p.part[i] = dbeta;
        p.part[TC + i] = dgamma;
        p.part[2 * TC + i] = dsum;
    }
}

template <int N, typename E>
inline int head_wide_launch_product(const HeadParams &p, float *psum, const HeadWideLayout &L, int NG, hipStream_t st)
{
    return launch<head_wide_product_kernel<N, E>>(dim3(p.T, L.NB, NG), dim3(head_wide_block(p.B)), 0, st, p, psum, L.CP);
}

}  // namespace ctc

extern "C" size_t ctc_amd_head_forward_wide_scratch_bytes(int T, int B, int K, int C)
{
    if (T < 1 || B < 1 || K < 1 || C < 1 || !ctc::head_shape_ok(T, B, K, C, ctc::kHeadWideMaxBatch)) return 0;
    return ctc::head_wide_layout(T, B, C).total + ctc::kHeadBwdAlign;             // (the entry aligns the pointer itself)
}

// ctc_amd_head_forward(_typed) for any batch up to kHeadWideMaxBatch: ONE launch in eval mode, TWO in train mode (see the top).
// Only the product launch reads feat: it carries the element type, the statistics launch is one kernel for all three.
extern "C" int ctc_amd_head_forward_wide_typed(const void *feat, int feat_dtype, int64_t feat_stride_t, int64_t feat_stride_b,
                                               const float *weight, const float *bias, const float *bn_weight, const float *bn_bias,
                                               const float *running_mean, const float *running_var, float eps, const float *mask,
                                               int T, int B, int K, int C,
                                               float *out, int64_t out_stride_t, int64_t out_stride_b,
                                               float *linear_out, float *save_mean, float *save_var, float *save_invstd,
                                               void *scratch, size_t scratch_bytes, void *stream)
{
    ctc::HeadParams p;
    int rc = ctc::head_forward_params(p, feat, feat_dtype, feat_stride_t, feat_stride_b, weight, bias, bn_weight, bn_bias,
                                      running_mean, running_var, eps, mask, T, B, K, C, out, out_stride_t, out_stride_b,
                                      linear_out, save_mean, save_var, save_invstd);
    if (rc == CTC_AMD_ERR_BAD_ARGUMENT) return rc;
    if (!scratch || scratch_bytes < ctc_amd_head_forward_wide_scratch_bytes(T, B, K, C)) return CTC_AMD_ERR_BAD_ARGUMENT;
    if (rc || !ctc::head_shape_ok(T, B, K, C, ctc::kHeadWideMaxBatch)) return CTC_AMD_ERR_UNSUPPORTED_SHAPE;
    const ctc::HeadWideLayout L = ctc::head_wide_layout(T, B, C);
    char *base = ctc::scratch_base(scratch);
    float *psum = reinterpret_cast<float *>(base + L.psum);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const bool train = running_mean == nullptr;
    if (train && !linear_out) p.lin = reinterpret_cast<float *>(base + L.lin);   // the statistics launch reads it
    int N, NG;
    ctc::head_wide_groups(C, N, NG);
    rc = ctc::with_logit_elem(feat_dtype, [&](auto e) {
        using E = typename decltype(e)::type;
        return N == 1   ? ctc::head_wide_launch_product<1, E>(p, psum, L, NG, st)
               : N == 2 ? ctc::head_wide_launch_product<2, E>(p, psum, L, NG, st)
                        : ctc::head_wide_launch_product<3, E>(p, psum, L, NG, st);
    });
    if (rc || !train) return rc;
    return launch<ctc::head_wide_stats_kernel>(dim3(T, L.CP / 16), dim3(ctc::head_wide_block(B)), 0, st, p,
                                               (const float *)psum, L.CP, L.NB);
}

extern "C" int ctc_amd_head_forward_wide(const float *feat, int64_t feat_stride_t, int64_t feat_stride_b,
                                         const float *weight, const float *bias, const float *bn_weight, const float *bn_bias,
                                         const float *running_mean, const float *running_var, float eps, const float *mask,
                                         int T, int B, int K, int C,
                                         float *out, int64_t out_stride_t, int64_t out_stride_b,
                                         float *linear_out, float *save_mean, float *save_var, float *save_invstd,
                                         void *scratch, size_t scratch_bytes, void *stream)
{
    return ctc_amd_head_forward_wide_typed(feat, CTC_AMD_F32, feat_stride_t, feat_stride_b, weight, bias, bn_weight, bn_bias,
                                           running_mean, running_var, eps, mask, T, B, K, C, out, out_stride_t, out_stride_b,
                                           linear_out, save_mean, save_var, save_invstd, scratch, scratch_bytes, stream);
}

extern "C" size_t ctc_amd_head_backward_wide_scratch_bytes(int T, int B, int K, int C)
{
    return ctc::head_bwd_scratch_bytes(T, B, K, C, ctc::kHeadWideMaxBatch);
}

// ctc_amd_head_backward(_typed) for any batch up to kHeadWideMaxBatch: the walking row pass, then the narrow entry's products and
// reduce launches on the same scratch layout -- two launches, three when T B > 128.
extern "C" int ctc_amd_head_backward_wide_typed(const float *d_out, int64_t dout_stride_t, int64_t dout_stride_b,
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
        return launch<ctc::head_wide_bwd_rows_kernel>(grid, dim3(ctc::head_wide_block(r.B)), 0, st, r);
    };
    return ctc::head_backward_enqueue(ctc::kHeadWideMaxBatch, rows, d_out, dout_stride_t, dout_stride_b, feat, feat_dtype,
                                      feat_stride_t, feat_stride_b, weight, bn_weight, bn_bias, linear_out, save_mean, save_invstd,
                                      running_mean, running_var, eps, mask, T, B, K, C, d_feat, dfeat_stride_t, dfeat_stride_b,
                                      d_weight, d_bias, d_bn_weight, d_bn_bias, scratch, scratch_bytes, stream);
}

extern "C" int ctc_amd_head_backward_wide(const float *d_out, int64_t dout_stride_t, int64_t dout_stride_b,
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
    return ctc_amd_head_backward_wide_typed(d_out, dout_stride_t, dout_stride_b, feat, CTC_AMD_F32, feat_stride_t, feat_stride_b,
                                            weight, bn_weight, bn_bias, linear_out, save_mean, save_invstd, running_mean,
                                            running_var, eps, mask, T, B, K, C, d_feat, dfeat_stride_t, dfeat_stride_b,
                                            d_weight, d_bias, d_bn_weight, d_bn_bias, scratch, scratch_bytes, stream);
}
