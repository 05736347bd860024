// Per-frame state posteriors on blank-CTC lattices wider than one wave: 256 <= S <= 1023 labels, 513 <= 2S+1 <= 2047
// states.  Included by blank_align.hip behind blank_align_wide.hpp: the arithmetic is PostChain<8>'s
// (pre / add_store / state_max / subtract, post_lse2, kPostNeg / kPostLive), the input rules are align_sample and
// align_label, the transition rule is align_skip_flag.  Three launches:
//   blank_table_gather_kernel         the table of blank_align.hip with NL = 256 W label columns and CMAX: the row's
//                                     emission maximum c_t in column NL + 1.  One wave has the whole row there, so
//                                     every wave of the chains reads the SAME c_t and no step reduces across waves.
//   blank_post_wide_chain_kernel      grid (B, 2), W = ceil((2S+1)/512) waves per workgroup: workgroup (b, 0) runs alpha
//                                     forward, (b, 1) runs beta' backward; wave w owns states [512 w, 512 w + 512), K = 8
//                                     per lane.  What crosses a wave goes through LDS, double-buffered by step parity, ONE
//                                     workgroup barrier per step and nothing polled (the hand-off of
//                                     blank_align_wide_kernel): alpha takes the last state of the wave below, beta' the
//                                     first two states of the wave above (its state 0 and, summed by the receiver with the
//                                     sender's own operations, state 0's two-term sum).  Every kPostRescale steps each
//                                     wave leaves its state maximum in LDS with that step's hand-off; in front of the
//                                     next step (where the narrow rescale() sits: the same arithmetic) every wave reads
//                                     all of them and subtracts their maximum from its states and from
//                                     the operands it was handed: one value per direction and sample, so the offsets of
//                                     neighbouring waves agree and alpha' + beta' has no seam.  alpha sums what it
//                                     subtracted (and the c_t) in double for nll.  Each wave stores its slice of the
//                                     alpha' / beta' rows [B][T][512 W].
//   blank_post_gamma_kernel<8 W>      the narrow combine launch with 8 W states per lane and row.
#pragma once

namespace ctc {

struct PostWideParams {
    PostParams p;                    // p.a: inputs, shape, em (the table); al / be with NSP = 512 W; nll, gamma
    int W;                           // waves per lattice row
};

// the emissions of one step of a wave's slice: el = the lane's four labels, bc = (blank, c_t)
struct PostWideRow {
    float4 el;
    float2 bc;
};

template <bool FWD>
__device__ __forceinline__ void post_wide_chain(const PostWideParams &q, int b, int Tb, int L)
{
    // operands on their way to the neighbouring wave: [step parity][value][slot].  alpha: wave w writes its last state
    // to slot w + 1 and reads slot w; beta': wave w writes its first two states to slot w and reads slot w + 1.  The
    // slot nobody writes (0 / W) stays at kPostNeg: no branch on the wave's place in the step.  (Plain LDS declared
    // here, as in blank_align_wide_kernel.)
    __shared__ float xch[2][2][kWideAlignMaxWaves + 1];
    // the waves' state maxima of a rescale step, read by every wave at the step behind it (the next rescale step
    // writes kPostRescale barriers later: one buffer); the slots of waves that do not exist stay at kPostNeg
    __shared__ __attribute__((aligned(16))) float xmx[kWideAlignMaxWaves];
    __shared__ float s_fin[2];                                    // alpha(2L), alpha(2L-1) from the waves that hold them
    constexpr int K = kWideAlignK, D = kPostAhead, G = kPostRescale;
    static_assert(D % G == 0, "rescale points are compile-time positions in the unrolled body");
    static_assert(kWideAlignMaxWaves == 4, "the maxima are one 16-byte LDS read");
    const PostParams &p = q.p;
    const int W = q.W, RW = align_row_pitch(K * W), NSP = p.NSP, T = p.a.T;
    const int tid = threadIdx.x, w = wave_id(), lane = lane_id();
    const int s0 = w * kWideAlignSpan + lane * K, n = 2 * L + 1;

    if (tid < 2 * 2 * (kWideAlignMaxWaves + 1)) (&xch[0][0][0])[tid] = kPostNeg;
    if (tid < kWideAlignMaxWaves) xmx[tid] = kPostNeg;
    __syncthreads();                                              // (the hand-off of step 0 writes behind it)

    PostChain<K, FWD> c;
    c.off = 0.0;
    c.coff = 0.0;
#pragma unroll
    for (int k = 0; k < K; ++k) c.skip[k] = align_skip_flag<FWD>(p.a, b, L, s0 + k, k);
    // the lane's labels of a row, and (blank, c_t) through a per-lane address: vector loads, counted with the rows (a
    // scalar load would be waited for with the LDS hand-off at every barrier)
    const float *em = p.a.em + (int64_t)b * T * RW + (w * kWave + lane) * (K / 2);
    const int boff = 256 * W - (w * kWave + lane) * (K / 2) + opaque_v(0);
    auto fetch = [&](PostWideRow &r, int i) {
        const int ii = i < Tb ? i : Tb - 1;
        const float *row = em + (int64_t)(FWD ? ii : Tb - 1 - ii) * RW;
        r.el = *reinterpret_cast<const float4 *>(row);
        r.bc = *reinterpret_cast<const float2 *>(row + boff);
    };
    const bool st = s0 < n;                                       // lanes wholly beyond the lattice store nothing
    const int64_t dir = FWD ? NSP : -(int64_t)NSP;
    float *dst = (FWD ? p.al : p.be) + ((int64_t)b * T + (FWD ? 0 : Tb - 1)) * NSP + s0;
    const int rslot = FWD ? w : w + 1, wslot = FWD ? w + 1 : w;
    // this wave's edge goes to the buffer step i + 1 reads; one barrier (lgkmcnt only: the rows in flight stay in
    // flight).  The states are operands of the barrier, as in blank_align_wide_kernel: the step's adds are done in front
    // of it and the refill behind it can land in the registers of the row the step has read.
    auto hand_on = [&](int i) {
        if (FWD) {
            if (lane == kWave - 1) xch[(i + 1) & 1][0][wslot] = c.a[K - 1];
        } else if (lane == 0) {
            xch[(i + 1) & 1][0][wslot] = c.a[0];
            xch[(i + 1) & 1][1][wslot] = c.a[1];
        }
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier"
                     : "+v"(c.a[0]), "+v"(c.a[1]), "+v"(c.a[2]), "+v"(c.a[3]), "+v"(c.a[4]), "+v"(c.a[5]), "+v"(c.a[6]),
                       "+v"(c.a[7])
                     :
                     : "memory");
    };
    auto add_store = [&](const float (&pre)[K], const PostWideRow &r) {
        AlignRow<K> e;
        e.el[0] = r.el.x; e.el[1] = r.el.y; e.el[2] = r.el.z; e.el[3] = r.el.w;
        e.eb = r.bc.x;
        c.add_store(pre, e, r.bc.y, dst, st);
        dst += dir;
    };
    // one step.  `apply`: the step behind a rescale step -- the maximum measured there over all waves leaves the states
    // and the operands handed on at that step (between that step's add_store and this step's pre: where the narrow
    // rescale() sits, the same arithmetic); `measure`: a rescale step
    auto step = [&](int i, const PostWideRow &r, bool apply, bool measure) {
        float in0 = xch[i & 1][0][rslot];                         // (wave-uniform)
        float in1 = FWD ? 0.f : xch[i & 1][1][rslot];
        if (apply) {
            const float4 mw = *reinterpret_cast<const float4 *>(xmx);
            float m = fmaxf(fmaxf(mw.x, mw.y), fmaxf(mw.z, mw.w));    // waves without a reachable state: kPostNeg
            m = m > kPostLive ? m : 0.f;
            c.subtract(m);
            in0 = vmax(in0 - m, kPostNeg);
            if (!FWD) in1 = vmax(in1 - m, kPostNeg);
        }
        float pre[K];
        if (FWD) c.pre(pre, in0);
        else c.pre(pre, in0, post_lse2(in0, in1));                // (the sum the wave above forms for its own state 0)
        add_store(pre, r);
        if (measure) {
            const float mx = c.state_max();
            if (lane == 0) xmx[w] = mx;
        }
        hand_on(i);
    };

    PostWideRow ring[D];
    {
        PostWideRow r0;
        fetch(r0, 0);
        float pre[K];
        const int sa = FWD ? 0 : 2 * L, sb = FWD ? 1 : 2 * L - 1;        // entry states (may sit in two waves)
#pragma unroll
        for (int k = 0; k < K; ++k) pre[k] = (s0 + k == sa || s0 + k == sb) ? 0.f : kPostNeg;
        add_store(pre, r0);
        hand_on(0);
    }
    int i = 1;
#pragma unroll
    for (int j = 0; j < D; ++j) fetch(ring[j], i + j);
    for (; i + D <= Tb; i += D) {
#pragma unroll
        for (int j = 0; j < D; ++j) {
            step(i + j, ring[j], j % G == 0, j % G == G - 1);     // (step first, refill afterwards: the load can land in
            fetch(ring[j], i + j + D);                            // the registers the step has just read)
        }
    }
#pragma unroll
    for (int j = 0; j < D; ++j)
        if (i + j < Tb) step(i + j, ring[j], j % G == 0, j % G == G - 1);    // (uniform over the workgroup)

    if (FWD) {
        wide_final_states(c.a, L, s_fin);
        __syncthreads();
        if (w == 0 && lane == 0) {                                // (off and coff are the same in every wave)
            const float v = post_lse2(s_fin[0], L > 0 ? s_fin[1] : kPostNeg);
            p.nll[b] = v > kPostLive ? (float)(-((double)v + c.off) * (double)kLn2 - c.coff) : __builtin_inff();
        }
    }
}

// grid (B, 2), block 64 W: blockIdx.y = 0 alpha, 1 beta'
__global__ __launch_bounds__(kWideAlignMaxWaves * kWave) void blank_post_wide_chain_kernel(PostWideParams q)
{
    const int b = blockIdx.x;
    int Tb, L;
    if (!align_sample(q.p.a, b, Tb, L)) {                        // lengths outside the tensor: no alignment (+inf, gamma rows 0)
        if (blockIdx.y == 0 && threadIdx.x == 0) q.p.nll[b] = __builtin_inff();
        return;                                                   // (uniform over the workgroup)
    }
    if (blockIdx.y == 0) post_wide_chain<true>(q, b, Tb, L);
    else post_wide_chain<false>(q, b, Tb, L);
}

// the gather and the chains: the alpha' / beta' rows and nll are out when these two have run
template <int W>
static int launch_blank_post_wide_chains(PostWideParams &q, hipStream_t s)
{
    static_assert(kWideAlignGatherRows == kPostRows, "the table's c_t column: one wave_max4 for the rows of a wave");
    const AlignParams &p = q.p.a;
    const int rc = launch_blank_table_gather<256 * W, kWideAlignGatherRows, true>(p, s);
    return rc ? rc : launch<blank_post_wide_chain_kernel>(dim3(p.B, 2), dim3(W * kWave), 0, s, q);
}

// the table, then the alpha' and the beta' rows: (256 W + 4) + 2 * 512 W floats per (b, t) of 1536 W
static int blank_post_wide_layout(PostParams &pp, PostWideParams &q)
{
    AlignParams &p = pp.a;
    size_t rest;
    const int rc = blank_wide_layout(p, q.W, rest);
    if (rc) return rc;
    pp.NSP = q.W * kWideAlignSpan;
    pp.NS = 2 * p.S + 1;
    const size_t cells = (size_t)p.B * p.T;
    if (2 * cells * pp.NSP * sizeof(float) > rest) return CTC_AMD_ERR_UNSUPPORTED_SHAPE;
    pp.al = p.em + cells * p.RW;
    pp.be = pp.al + cells * pp.NSP;
    q.p = pp;
    return 0;
}

static int run_blank_post_wide(PostParams &pp, hipStream_t s)
{
    PostWideParams q;
    const int rc = blank_post_wide_layout(pp, q);
    if (rc) return rc;
    return with_constant<2, 3, 4>(q.W, [&](auto w) {
        constexpr int W = decltype(w)::value;
        const AlignParams &p = q.p.a;
        const int crc = launch_blank_post_wide_chains<W>(q, s);
        if (crc) return crc;
        const int rows = (kPostThreads / kWave) * kPostRows;
        return launch<blank_post_gamma_kernel<kWideAlignK * W>>(dim3((p.T + rows - 1) / rows, p.B), dim3(kPostThreads), 0, s, q.p);
    });
}

}  // namespace ctc
