// Blank-CTC lattices wider than one wave: 256 <= S <= 1023 labels, 513 <= 2S+1 <= 2047 states.
// Included by blank.hip, which owns the arithmetic (lse2_2, kNegB, BlankParams, the log2-domain lattice): this is the
// same loss, wider.  Three launches, as the narrow path's three-launch schedule:
//   gather  em[b,t,s] = lp[t,b,l'_s] and the state tables, the tables' states dealt over the sample's row blocks
//   chains  one workgroup per (sample, direction) of W = ceil((2S+1)/512) waves, each wave with the narrow path's
//           K = 8 states per lane, so a lane's serial work per step is what it is at S = 255.  K is even: the only
//           operands that cross a wave are v(s-1) and v(s-2) of a wave's first two states (alpha: both come from the
//           previous wave's LAST state of the step before; beta, mirrored: the next wave's FIRST state and that
//           blank's pre-emission sum).  They go through LDS, double-buffered, one workgroup barrier per step: step i
//           reads buffer i & 1 and writes buffer (i + 1) & 1, so a wave that runs ahead after the barrier of step i
//           writes the buffer everybody has finished reading BEFORE that barrier.  No polling: nothing can starve.
//   grad    one wave per (t,b) row, the row's states in W passes of 64 x 8 held in registers
// The padded state count is 512 W (1024, 1536, 2048), not a power of two.
#pragma once

namespace ctc {

constexpr int kWideK = 8;                            // states per lane
constexpr int kWideSpan = kWave * kWideK;            // states per wave / per pass of a gradient wave
static_assert(kWideSpan == kWave * 8, "blank_padded_states pads to this");
constexpr int kWideMaxWaves = 4;                     // 2047 states
constexpr int kWideNxtBits = 12;                     // packed state table of a gradient wave: class << 12 | next + 1

// ---- gather + state tables ------------------------------------------------------------------------------
// Grid: (row blocks, B); block x takes rows [x rpb, (x+1) rpb) and every gridDim.x-th slice of 256 states of the tables
// (one block doing all of them walks 8 x 1023 labels per thread at S = 1023).
__global__ __launch_bounds__(256) void blank_wide_gather_kernel(BlankParams p, int rows_per_block)
{
    extern __shared__ int s_cls[];                           // [NSP] classes + [1] adjacent repeats
    const int b = blockIdx.y, tid = threadIdx.x;
    int Tb, L;
    blank_sample_ok(p, b, Tb, L);
    const int n = 2 * L + 1;
    if (tid == 0) s_cls[p.NSP] = 0;
    blank_classes(p, b, n, s_cls);
    for (int s = blockIdx.x * blockDim.x + tid; s < p.NSP; s += gridDim.x * blockDim.x) blank_table_entry(p, b, n, s, s_cls);
    if (blockIdx.x == 0) {                                   // an alignment needs one step per label plus a blank
        int rep = 0;                                         // between every two equal neighbours
        for (int l = 1 + tid; l < L; l += blockDim.x) rep += s_cls[2 * l + 1] == s_cls[2 * l - 1] ? 1 : 0;
        if (rep) atomicAdd(&s_cls[p.NSP], rep);
        __syncthreads();
        if (tid == 0) p.meta[b] = make_int2(Tb >= L + s_cls[p.NSP] ? Tb : 0, L);
    }
    const int t_begin = blockIdx.x * rows_per_block;
    const int t_end = min(t_begin + rows_per_block, Tb);
    for (int t = t_begin; t < t_end; ++t) {
        const float *row = p.lp + (int64_t)t * p.st + (int64_t)b * p.sb;
        float *out = p.em + ((int64_t)b * p.T + t) * p.NSP;
        for (int s = tid; s < p.NSP; s += blockDim.x) out[s] = s < n ? blank_emission(row[s_cls[s]]) : kNegB;
    }
}

// ---- chains ---------------------------------------------------------------------------------------------
// One time step of a wave's 512 states; blank_step<8, FWD> of the narrow path, operation for operation, with the
// wave's outer neighbour coming in from the wave beside it instead of the kNegB fill.
//   alpha: in0 = the previous wave's last (label) state
//   beta:  in0 = the next wave's first (blank) state, in1 = what that blank comes from (its pre-emission sum);
//          pb0 carries this lane's own first blank's sum from the end of one step to the next, where the narrow
//          step computes it at the start: the same operation on the same operands, and the value a neighbour needs
template <bool FWD>
__device__ __forceinline__ void blank_wide_step(float (&a)[kWideK], const float (&e)[kWideK], const bool (&skip)[kWideK],
                                                float in0, float in1, float &pb0)
{
    constexpr int K = kWideK;
    float pre[K];
    if (FWD) {
        const float n1 = wave_shr1(a[K - 1], in0);
#pragma unroll
        for (int k = 0; k < K; k += 2) pre[k] = lse2_2(a[k], k >= 1 ? a[k - 1] : n1);
#pragma unroll
        for (int k = 1; k < K; k += 2) pre[k] = lse2_2(a[k], skip[k] ? pre[k - 1] : a[k - 1]);
    } else {
        const float n1 = wave_shl1(a[0], in0);
        pre[0] = pb0;
#pragma unroll
        for (int k = 2; k < K; k += 2) pre[k] = lse2_2(a[k], a[k + 1]);
        const float nb = wave_shl1(pre[0], in1);
#pragma unroll
        for (int k = 1; k < K; k += 2) pre[k] = lse2_2(a[k], skip[k] ? (k + 1 < K ? pre[k + 1] : nb) : (k + 1 < K ? a[k + 1] : n1));
    }
#pragma unroll
    for (int k = 0; k < K; ++k) a[k] = pre[k] + e[k];
    if (!FWD) pb0 = lse2_2(a[0], a[1]);
}

// wave w of the W of a chain: states [512 w, 512 w + 512).  Every wave of the workgroup makes the same T_b barriers.
template <bool FWD>
__device__ __forceinline__ void blank_wide_chain(const BlankParams &p, int b, int Tb, int L, int w, int W, float (&a)[kWideK])
{
    // the edges on their way to the neighbour wave: [step parity][wave][value].  (Declared here, accessed as plain LDS:
    // through a volatile pointer argument the accesses became flat instructions that each drained the vector-memory
    // counter, and with it the emission rows in flight.  The barrier below is the compiler's fence.)
    __shared__ float xch[2][kWideMaxWaves][2];
    constexpr int K = kWideK, D = kRingRegs / K;             // emission rows in flight
    const int lane = lane_id(), s0 = (w * kWave + lane) * K, n = 2 * L + 1;
    const float *em = p.em + (int64_t)b * p.T * p.NSP + s0;
    float *out = (FWD ? p.al : p.be) + (int64_t)b * p.T * p.NSP + s0;
    bool skip[K];
    blank_state_flags<K, FWD>(p, b, n, s0, skip);
    const int from = FWD ? w - 1 : w + 1;                    // the wave whose edge this one needs, and the one that
    const bool hears = from >= 0 && from < W;                // needs this one's
    const bool tells = FWD ? w + 1 < W : w > 0;
    float pb0 = kNegB;
    auto row_of = [&](int i) { return FWD ? i : Tb - 1 - i; };
    auto fetch = [&](float (&dst)[K], int i) {
        const float *r = em + (int64_t)row_of(i < Tb ? i : Tb - 1) * p.NSP;
#pragma unroll
        for (int k = 0; k < K; ++k) dst[k] = r[k];
    };
    // the row of step i goes to the workspace; this wave's edge goes to the buffer step i + 1 reads; one barrier.
    // (lgkmcnt only: the emission rows in flight stay in flight across the barrier)
    auto hand_on = [&](int i) {
        float *r = out + (int64_t)row_of(i) * p.NSP;
#pragma unroll
        for (int k = 0; k < K; ++k) r[k] = a[k];
        if (tells && lane == (FWD ? kWave - 1 : 0)) {
            xch[(i + 1) & 1][w][0] = FWD ? a[K - 1] : a[0];
            if (!FWD) xch[(i + 1) & 1][w][1] = pb0;
        }
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    };
    auto step = [&](int i, const float (&e)[K]) {
        float in0 = kNegB, in1 = kNegB;
        if (hears) {                                         // (wave-uniform)
            in0 = xch[i & 1][from][0];
            if (!FWD) in1 = xch[i & 1][from][1];
        }
        blank_wide_step<FWD>(a, e, skip, in0, in1, pb0);
        hand_on(i);
    };
    float ring[D][K];
    {
        float e0[K];
        fetch(e0, 0);
        blank_first<K, FWD>(a, e0, n, s0);
        if (!FWD) pb0 = lse2_2(a[0], a[1]);
        hand_on(0);
    }
    int i = 1;
#pragma unroll
    for (int j = 0; j < D; ++j) fetch(ring[j], i + j);
    for (; i + D <= Tb; i += D) {
#pragma unroll
        for (int j = 0; j < D; ++j) {
            step(i + j, ring[j]);                            // (the refill AFTER the step has used the row: the load can
            fetch(ring[j], i + j + D);                       // land in the same registers, nothing to rotate at the loop's end)
        }
    }
#pragma unroll
    for (int j = 0; j < D; ++j)
        if (i + j < Tb) step(i + j, ring[j]);                // (uniform over the workgroup)
}

// Grid: (B, 2 with a gradient / 1 without); y = 0 alpha (+ likelihood and batch mean), y = 1 beta.  Block: 64 W.
__global__ __launch_bounds__(kWideMaxWaves * kWave) void blank_wide_chain_kernel(BlankParams p)
{
    __shared__ float s_fin[kWideMaxWaves][2];
    constexpr int K = kWideK;
    const int b = blockIdx.x, w = wave_id(), W = blockDim.x >> 6, lane = lane_id();
    int Tb, L;
    const bool ok = blank_sample_ok(p, b, Tb, L);
    const bool run = ok && Tb > 0;                           // uniform over the workgroup
    float a[K];
    if (blockIdx.y == 1) {
        if (run) blank_wide_chain<false>(p, b, Tb, L, w, W, a);
        return;
    }
    float nll = __builtin_inff();
    if (run) {
        blank_wide_chain<true>(p, b, Tb, L, w, W, a);
        // alpha_{T-1}(n-1) and (n-2): in one wave or in two neighbours; every other wave adds an exact 0
        const int n = 2 * L + 1;
        float v1 = 0.f, v2 = 0.f;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int s = (w * kWave + lane) * K + k;
            if (s == n - 1) v1 = a[k];
            if (s == n - 2) v2 = a[k];
        }
        v1 = wave_sum(v1);
        v2 = wave_sum(v2);
        if (lane == 0) { s_fin[w][0] = v1; s_fin[w][1] = v2; }
        __syncthreads();
        if (w != 0) return;
        v1 = 0.f; v2 = 0.f;
        for (int q = 0; q < W; ++q) { v1 += s_fin[q][0]; v2 += s_fin[q][1]; }
        const float ll2 = lse2_2(v1, n >= 2 ? v2 : kNegB);
        nll = ll2 < -1.0e29f ? __builtin_inff() : -ll2 * kLn2;
    } else {
        if (w != 0) return;
        if (ok && L == 0) nll = 0.f;                         // empty input, empty target
    }
    publish_and_reduce(nll, b, p.B, p.nll, p.loss, p.loss_scale, p.counter,
                       [&](float v, int i) {
                           const int64_t Li = p.tgt_len[i];
                           return v / (float)(Li > 1 ? Li : 1);
                       });
}

// ---- gamma -> gradient rows -----------------------------------------------------------------------------
// blank_row_emit of the narrow path with the row's states in W passes of 64 x 8 (the zero rows and the dense row
// are the narrow path's own: blank_row_fill, blank_row_dense).  Per wave in LDS: occ[C4],
// gam[NSP] and the sample's packed state table tab[NSP] (class << 12 | next state of that class + 1; 0 ends the
// chain); which of a lane's 8 W states are the first of their class is a bit mask in a register.
template <int W, bool VEC4>
__global__ __launch_bounds__(kGradWaves * kWave) void blank_wide_grad_kernel(BlankParams p, int total_rows)
{
    extern __shared__ float4 s_buf4[];
    constexpr int K = kWideK;
    const int w = wave_id(), lane = lane_id();
    const int C4 = (p.C + 3) & ~3;
    float *occ = reinterpret_cast<float *>(s_buf4) + (size_t)w * (C4 + 2 * p.NSP);
    float *gam = occ + C4;
    int *tab = reinterpret_cast<int *>(gam + p.NSP);
    for (int c = lane; c < C4; c += kWave) occ[c] = 0.f;
    int tab_b = -1;
    unsigned first_mask = 0;
    for (int idx = blockIdx.x * kGradWaves + w; idx < total_rows; idx += gridDim.x * kGradWaves) {
        const int t = idx / p.B;
        const int b = __builtin_amdgcn_readfirstlane(idx - t * p.B);
        const int2 meta = p.meta[b];
        const int Te = __builtin_amdgcn_readfirstlane(meta.x), L = __builtin_amdgcn_readfirstlane(meta.y);
        if (t >= Te) {                                       // beyond T_b, or no alignment: a zero row
            blank_row_fill<VEC4>(p, t, b, 0.f);
            continue;
        }
        const int n = 2 * L + 1;
        const int64_t o = ((int64_t)b * p.T + t) * p.NSP;
        float v[W][K];
        float4 xr[kMaxV4];
#pragma unroll
        for (int q = 0; q < W; ++q) {
            const int s0 = q * kWideSpan + lane * K;
            float al[K], be[K], em[K];
#pragma unroll
            for (int k = 0; k < K; ++k) al[k] = be[k] = em[k] = 0.f;
            if (s0 < n) {                                    // (lanes beyond the sample's states load nothing)
#pragma unroll
                for (int k = 0; k < K; ++k) { al[k] = p.al[o + s0 + k]; be[k] = p.be[o + s0 + k]; em[k] = p.em[o + s0 + k]; }
            }
#pragma unroll
            for (int k = 0; k < K; ++k) v[q][k] = s0 + k < n ? al[k] + be[k] - em[k] : kNegB;
        }
        if (VEC4) {
            const float4 *row = reinterpret_cast<const float4 *>(p.lp + (int64_t)t * p.st + (int64_t)b * p.sb);
            const int c4 = p.C >> 2;
#pragma unroll
            for (int i = 0; i < kMaxV4; ++i) xr[i] = row[min(lane + kWave * i, c4 - 1)];   // (past the row: its last float4 again)
        }
        if (tab_b != b) {                                    // (wave-uniform) the sample's tables: once per sample change
            tab_b = b;
            first_mask = 0;
#pragma unroll
            for (int q = 0; q < W; ++q) {
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    const int s = q * kWideSpan + lane * K + k;
                    tab[s] = (p.cls[b * p.NSP + s] << kWideNxtBits) | (p.nxt[b * p.NSP + s] + 1);
                    if (p.first[b * p.NSP + s] != 0) first_mask |= 1u << (q * K + k);
                }
            }
        }
        float m = kNegB;
#pragma unroll
        for (int q = 0; q < W; ++q)
#pragma unroll
            for (int k = 0; k < K; ++k) m = fmaxf(m, v[q][k]);
        m = wave_max(m);
        if (m < -1.0e29f) {                                  // no alignment through the emissions: as blank_row_emit
            blank_row_fill<VEC4>(p, t, b, 0.f);
            continue;
        }
        float ssum = 0.f, blank_part = 0.f;
#pragma unroll
        for (int q = 0; q < W; ++q) {
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const int s = q * kWideSpan + lane * K + k;
                v[q][k] = s < n ? __builtin_amdgcn_exp2f(v[q][k] - m) : 0.f;   // lattice is in log2 units
                ssum += v[q][k];
                if ((k & 1) == 0) blank_part += v[q][k];
            }
        }
        ssum = wave_sum(ssum);
        blank_part = wave_sum(blank_part);
        const float inv = 1.0f / ssum;
#pragma unroll
        for (int q = 0; q < W; ++q)
#pragma unroll
            for (int k = 0; k < K; ++k) gam[q * kWideSpan + lane * K + k] = v[q][k] * inv;   // wave-local LDS, in order
        // occupancy per class: labels folded along the repeat chain, then the blank from the reduction, added to its
        // entry as in blank_row_emit (a bad label clamped onto the blank's class has left its share there)
#pragma unroll
        for (int q = 0; q < W; ++q) {
#pragma unroll
            for (int k = 1; k < K; k += 2) {
                if (first_mask >> (q * K + k) & 1) {         // label states only; repeats are chained
                    const int s = q * kWideSpan + lane * K + k;
                    const int e = tab[s];
                    float tot = gam[s];
                    for (int nx = e & ((1 << kWideNxtBits) - 1); nx != 0; nx = tab[nx - 1] & ((1 << kWideNxtBits) - 1)) tot += gam[nx - 1];
                    occ[e >> kWideNxtBits] = tot;
                }
            }
        }
        if (lane == 0) occ[p.blank] += blank_part * inv;
        blank_row_dense<VEC4>(p, t, b, xr, occ, p.grad_scale / (float)(L > 1 ? L : 1));
        // un-set only what this row touched
        if (lane == 0) occ[p.blank] = 0.f;
#pragma unroll
        for (int q = 0; q < W; ++q) {
#pragma unroll
            for (int k = 1; k < K; k += 2) {
                const int s = q * kWideSpan + lane * K + k;
                if (s < n) occ[tab[s] >> kWideNxtBits] = 0.f;
            }
        }
    }
}

// the launches; p.S > 255 (the caller has checked 2S+1 <= 2047 and the LDS of a gradient wave, and laid out the
// workspace: p.NSP = 512 W; the hand-off state in it stays unused, the persistent launch is not taken)
static int run_blank_wide(BlankParams &p, hipStream_t s)
{
    const int W = p.NSP / kWideSpan;
    const bool vec4 = blank_rows_vec4(p);
    const int rows_per_block = 8;
    const dim3 ggrid((p.T + rows_per_block - 1) / rows_per_block, p.B);
    int rc = launch<blank_wide_gather_kernel>(ggrid, dim3(256), (p.NSP + 1) * sizeof(int), s, p, rows_per_block);
    if (rc) return rc;
    rc = launch<blank_wide_chain_kernel>(dim3(p.B, p.grad ? 2 : 1), dim3(W * kWave), 0, s, p);
    if (rc || !p.grad) return rc;
    if (W == 2) return blank_launch_grad<blank_wide_grad_kernel<2, true>, blank_wide_grad_kernel<2, false>>(p, vec4, s);
    if (W == 3) return blank_launch_grad<blank_wide_grad_kernel<3, true>, blank_wide_grad_kernel<3, false>>(p, vec4, s);
    return blank_launch_grad<blank_wide_grad_kernel<4, true>, blank_wide_grad_kernel<4, false>>(p, vec4, s);
}

}  // namespace ctc
