// Best path (Viterbi forced alignment) on blank-CTC lattices wider than one wave: 256 <= S <= 1023 labels,
// 513 <= 2S+1 <= 2047 states.  Included by blank_align.hip, which owns the arithmetic and the
// input rules (AlignParams, align_sample, align_label, align_state_value): the same select chain, wider.
// Two launches:
//   blank_align_wide_gather_kernel<W>  (bandwidth, every CU)  em[b,t,:] = lp[t,b,{l_0 .. l_{256W-1}, blank}] (labels
//                                      j >= L -> -inf): the narrow gather's layout with a row of 256 W + 4 floats.
//   blank_align_wide_kernel            (latency, one workgroup of W = ceil((2S+1)/512) waves per sample)  wave w owns
//                                      states [512 w, 512 w + 512), K = 8 per lane.  K is even, so the only operand
//                                      that crosses a wave is the previous wave's LAST state of step t-1 (v(s-1) of a
//                                      wave's state 0, v(s-2) of its state 1): through LDS, double-buffered by step
//                                      parity, one workgroup barrier per step -- the hand-off of blank_wide_chain
//                                      (blank_wide.hpp).  Nothing polls: no bounded wait, no status bit.  Every wave
//                                      loads its own slice of the emission rows kWideAlignAhead rows ahead into
//                                      registers.  Back-pointers: 2 bits per state and step, 16 bits per lane and
//                                      step, two steps per 32-bit word, stored as whole 256-byte rows [T/2][W][64]
//                                      behind the table in the workspace.  Wave 0 walks them back: 16 word rows of
//                                      two wave slices fetched ahead, one readlane per step, 64 path entries per store.
#pragma once

namespace ctc {

constexpr int kWideAlignK = 8;                          // states per lane
constexpr int kWideAlignSpan = kWave * kWideAlignK;     // states per wave
constexpr int kWideAlignMaxWaves = 4;                   // 2047 states
constexpr int kWideAlignAhead = 16;                     // emission rows in flight per wave (even: see the scan loop)
constexpr int kWideAlignGatherRows = 4;                 // rows per wave of the gather launch
static_assert(kWideAlignK == 8 && 16 / kWideAlignK == 2, "two steps per back-pointer word");
static_assert(kWideAlignAhead % 2 == 0, "a step's half of its back-pointer word is a compile-time position");
// two blocks of the walk back move the state by at most 4 * 2 * kAlignWalkWords < 512: they stay within two waves
static_assert(8 * kAlignWalkWords < kWideAlignSpan, "the walk's two fetched slices cover two blocks");

__host__ __device__ constexpr int align_wide_row_pitch(int W) { return 256 * W + 4; }

struct AlignWideParams {
    AlignParams a;                   // inputs, shape, outputs, em (the table), spill (the back-pointer words)
    int W, NW;                       // waves per sample, back-pointer word rows per sample ((T + 1) / 2)
};

// ---- launch 1: the compact emission rows ---------------------------------------------------------
// grid (ceil(T / (4 * kWideAlignGatherRows)), B); a wave takes kWideAlignGatherRows rows, a row's 256 W + 1 columns dealt
// over its lanes in M passes, all loads in flight at once.  (blank_post_wide_gather_kernel in blank_post_wide.hpp is a
// copy of this body plus the row maximum: a change to the table's layout goes into both.)
template <int W>
__global__ __launch_bounds__(kAlignGatherThreads) void blank_align_wide_gather_kernel(AlignWideParams q)
{
    constexpr int RW = align_wide_row_pitch(W), M = (RW + kWave - 1) / kWave, NL = 256 * W;
    const AlignParams &p = q.a;
    const int b = blockIdx.y, lane = lane_id();
    int Tb, L;
    if (!align_sample(p, b, Tb, L)) return;
    const int t0 = (blockIdx.x * (kAlignGatherThreads / kWave) + wave_id()) * kWideAlignGatherRows;
    if (t0 >= Tb) return;
    int col[M];
#pragma unroll
    for (int m = 0; m < M; ++m) {
        const int j = lane + kWave * m;
        col[m] = j < L ? align_label(p, b, j) : (j == NL ? p.blank : -1);
    }
    const float *__restrict__ lp = p.lp + (int64_t)b * p.sb;
    float v[kWideAlignGatherRows][M];
#pragma unroll
    for (int r = 0; r < kWideAlignGatherRows; ++r) {
        const int t = min(t0 + r, Tb - 1);
#pragma unroll
        for (int m = 0; m < M; ++m) v[r][m] = lp[(int64_t)t * p.st + (col[m] >= 0 ? col[m] : p.blank)];
    }
    float *__restrict__ out = p.em + ((int64_t)b * p.T + t0) * RW;
#pragma unroll
    for (int r = 0; r < kWideAlignGatherRows; ++r) {
        if (t0 + r >= Tb) break;
#pragma unroll
        for (int m = 0; m < M; ++m) {
            const int j = lane + kWave * m;
            if (j < RW) out[r * RW + j] = col[m] >= 0 ? v[r][m] : -__builtin_inff();
        }
    }
}

// ---- launch 2: scan + walk back ------------------------------------------------------------------
// the emissions of one step of a wave's slice: el = the lane's four labels (one 16-byte load), eb = the blank
struct AlignWideRow {
    float4 el;
    float eb;
};

// from state `s` at step Tb-1 down to step 0 (wave 0); path[t] = s_t, stored 64 steps at a time.  The words of a block
// of 2 * kAlignWalkWords steps are fetched for two wave slices, `base` and `base - 1`, one block ahead: base is the
// wave of the state at the START of the block before (the state falls by at most 2 per step, so by less than 512 over two
// blocks: it cannot leave the two slices).
__device__ __forceinline__ void align_wide_walk(const unsigned *bp, int W, int Tb, int s, int32_t *out)
{
    constexpr int K = kWideAlignK, NWW = kAlignWalkWords;
    const int lane = lane_id();
    unsigned chi[NWW], clo[NWW], nhi[NWW], nlo[NWW];
    auto load_words = [&](unsigned (&hi)[NWW], unsigned (&lo)[NWW], int wtop, int base) {
#pragma unroll
        for (int i = 0; i < NWW; ++i) {
            const int r = wtop - i;
            hi[i] = r < 0 ? 0u : bp[((int64_t)r * W + base) * kWave + lane];
            lo[i] = (r < 0 || base == 0) ? 0u : bp[((int64_t)r * W + base - 1) * kWave + lane];
        }
    };
    int outv = -1;
    const int wtop = (Tb - 1) >> 1;
    int base_n = s / kWideAlignSpan;
    load_words(nhi, nlo, wtop, base_n);
    for (int w0 = wtop; w0 >= 0; w0 -= NWW) {
#pragma unroll
        for (int i = 0; i < NWW; ++i) { chi[i] = nhi[i]; clo[i] = nlo[i]; }
        const int base = base_n;
        base_n = s / kWideAlignSpan;
        if (w0 >= NWW) load_words(nhi, nlo, w0 - NWW, base_n);
#pragma unroll
        for (int i = 0; i < NWW; ++i) {
#pragma unroll
            for (int sub = 1; sub >= 0; --sub) {
                const int t = (w0 - i) * 2 + sub;                 // (t < 0 only below the last block: nothing to do)
                if (t >= 0 && t < Tb) {
                    outv = lane == (t & (kWave - 1)) ? s : outv;
                    if ((t & (kWave - 1)) == 0 && t + lane < Tb) out[t + lane] = outv;
                    const int word = (int)(s / kWideAlignSpan == base ? chi[i] : clo[i]);
                    const unsigned x = (unsigned)__builtin_amdgcn_readlane(word, (s & (kWideAlignSpan - 1)) / K);
                    if (t >= 1) s -= (int)((x >> (2 * K * sub + 2 * (s & (K - 1)))) & 3u);
                }
            }
        }
    }
}

// grid B, block 64 W
__global__ __launch_bounds__(kWideAlignMaxWaves * kWave) void blank_align_wide_kernel(AlignWideParams q)
{
    // the last state of every wave on its way to the wave above: [step parity][reader]; wave w reads slot w and writes
    // slot w + 1, slot 0 stays at -inf (wave 0 has no lower neighbour) and slot W is read by nobody: no branch on the
    // wave's place in the step.  (Plain LDS declared here, as in blank_wide_chain: through a volatile pointer the
    // accesses become flat instructions that drain the row loads.)
    __shared__ float xch[2][kWideAlignMaxWaves + 1];
    __shared__ float s_fin[2];                                    // v(2L), v(2L-1) from the waves that hold them
    constexpr int K = kWideAlignK, D = kWideAlignAhead;
    const AlignParams &p = q.a;
    const int W = q.W, RW = align_wide_row_pitch(W);
    const int b = blockIdx.x, tid = threadIdx.x, w = wave_id(), lane = lane_id();
    const int nthreads = W * kWave;
    int32_t *out = p.path + (int64_t)b * p.T;
    int Tb, L;
    if (!align_sample(p, b, Tb, L)) {                             // (uniform over the workgroup)
        for (int t = tid; t < p.T; t += nthreads) out[t] = -1;
        if (tid == 0) p.score[b] = -__builtin_inff();
        return;
    }
    for (int t = Tb + tid; t < p.T; t += nthreads) out[t] = -1;

    const int s0 = w * kWideAlignSpan + lane * K;                 // the lane's first state: a blank
    bool skip[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int s = s0 + k;
        // a label state s >= 3 may come from s - 2 when its class is no blank and differs from that of s - 2
        bool sk = false;
        if ((k & 1) && s >= 3 && s <= 2 * L - 1) {
            const int c = align_label(p, b, (s - 1) >> 1), c2 = align_label(p, b, (s - 3) >> 1);
            sk = c != p.blank && c != c2;
        }
        skip[k] = sk;
    }
    if (tid < 2) xch[tid][0] = -__builtin_inff();                 // (before the first barrier)
    // the lane's labels of a row, and the blank through a per-lane address: a vector load, counted with the rows
    // (a scalar load would be waited for with the LDS hand-off at every barrier)
    const float *em = p.em + (int64_t)b * p.T * RW + (w * kWave + lane) * (K / 2);
    const int boff = 256 * W - (w * kWave + lane) * (K / 2) + opaque_v(0);
    unsigned *bp = p.spill + ((int64_t)b * q.NW * W + w) * kWave + lane;
    auto fetch = [&](AlignWideRow &r, int i) {
        const float *row = em + (int64_t)(i < Tb ? i : Tb - 1) * RW;
        r.el = *reinterpret_cast<const float4 *>(row);
        r.eb = row[boff];
    };
    float a[K];
    unsigned word = 0;
    // this wave's edge goes to the buffer step i + 1 reads; one barrier (lgkmcnt only: the rows in flight stay in flight).
    // The states are operands of the barrier: the step's adds are done in front of it, the row they read is dead, and the
    // refill behind the barrier can land in the row's registers (left to the scheduler, the adds drift behind the
    // refill, the ring is rotated through copies at the loop's end and waits vmcnt(2) there: drained every D steps).
    auto hand_on = [&](int i) {
        if (lane == kWave - 1) xch[(i + 1) & 1][w + 1] = a[K - 1];
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier"
                     : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "+v"(a[4]), "+v"(a[5]), "+v"(a[6]), "+v"(a[7])
                     :
                     : "memory");
    };
    // one step: the select chain stay -> advance -> skip, one add (AlignScan<8>::step with the neighbour wave's edge as
    // the fill of the shift); 2-bit codes into half `sub` of the word
    auto step = [&](int i, const AlignWideRow &e, int sub) {
        const float in0 = xch[i & 1][w];                          // (wave-uniform)
        const float nb = wave_shr1(a[K - 1], in0);
        const float el[K / 2] = {e.el.x, e.el.y, e.el.z, e.el.w};
        float n[K];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const float adv = k == 0 ? nb : a[k - 1];
            float best = a[k];
            unsigned c = 0;
            if (adv > best) { best = adv; c = 1; }
            if (k & 1) {
                const float sk = k == 1 ? nb : a[k - 2];
                if (skip[k] && sk > best) { best = sk; c = 2; }
            }
            n[k] = best + ((k & 1) ? el[k / 2] : e.eb);
            word |= c << (2 * K * sub + 2 * k);
        }
#pragma unroll
        for (int k = 0; k < K; ++k) a[k] = n[k];
        if (sub == 1) {                                           // the word of steps i - 1, i is complete
            bp[(int64_t)(i >> 1) * W * kWave] = word;
            word = 0;
        }
        hand_on(i);
    };
    AlignWideRow ring[D];
    {
        AlignWideRow e0;
        fetch(e0, 0);
#pragma unroll
        for (int k = 0; k < K; ++k) a[k] = s0 + k == 0 ? e0.eb : (s0 + k == 1 ? e0.el.x : -__builtin_inff());
        hand_on(0);                                               // (step 0 leaves its half of word 0 at code 0)
    }
    int i = 1;
#pragma unroll
    for (int j = 0; j < D; ++j) fetch(ring[j], i + j);
    for (; i + D <= Tb; i += D) {                                 // i is odd: step i + j fills half (j + 1) & 1
#pragma unroll
        for (int j = 0; j < D; ++j) {
            step(i + j, ring[j], (j + 1) & 1);                    // (step first, refill afterwards: the load can land in
            fetch(ring[j], i + j + D);                            // the registers the step has just read)
        }
    }
#pragma unroll
    for (int j = 0; j < D; ++j)
        if (i + j < Tb) step(i + j, ring[j], (j + 1) & 1);        // (uniform over the workgroup)
    if (((Tb - 1) & 1) == 0) bp[(int64_t)((Tb - 1) >> 1) * W * kWave] = word;   // a last word with its lower half only

    // v(2L) and v(2L-1) may sit in two waves (2L = 512 w: the first state of wave w, 2L-1 the last of wave w-1)
    const int sa = 2 * L, sb = L > 0 ? 2 * L - 1 : 0;
    if (sa / kWideAlignSpan == w) {
        const float x = align_state_value<K>(a, sa & (kWideAlignSpan - 1));
        if (lane == 0) s_fin[0] = x;
    }
    if (sb / kWideAlignSpan == w) {
        const float x = align_state_value<K>(a, sb & (kWideAlignSpan - 1));
        if (lane == 0) s_fin[1] = x;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");              // this wave's back-pointer words have left it
    __syncthreads();
    if (w != 0) return;
    int sfin = 0;
    if (L > 0) sfin = s_fin[0] > s_fin[1] ? sa : sb;
    const float score = sfin == sa ? s_fin[0] : s_fin[1];
    if (lane == 0) p.score[b] = score;
    if (!(score > -__builtin_inff())) {                           // no alignment
        for (int t = lane; t < Tb; t += kWave) out[t] = -1;
        return;
    }
    align_wide_walk(p.spill + (int64_t)b * q.NW * W * kWave, W, Tb, __builtin_amdgcn_readfirstlane(sfin), out);
}

// 256 <= p.S <= 1023 (the caller has checked); the table and the back-pointer words lie in the three lattice areas of
// ctc_amd_workspace_bytes(CTC_AMD_BLANK, ...): (256 W + 4) + 32 W words per (b, t) (+ 32 W per sample at odd T) of 1536 W
static int run_blank_align_wide(AlignParams &p, hipStream_t s)
{
    AlignWideParams q;
    q.W = (2 * p.S + 1 + kWideAlignSpan - 1) / kWideAlignSpan;
    q.NW = (p.T + 1) / 2;
    const int RW = align_wide_row_pitch(q.W);
    p.RW = RW;
    p.R = p.WL = 0;
    p.NWS = q.NW;
    char *ws = reinterpret_cast<char *>(p.counter) + 256;
    const size_t table = (size_t)p.B * p.T * RW * sizeof(float);
    const size_t words = (size_t)p.B * q.NW * q.W * kWave * sizeof(unsigned);
    p.em = reinterpret_cast<float *>(ws);
    p.spill = reinterpret_cast<unsigned *>(ws + table);
    const size_t areas = 3 * (size_t)p.B * p.T * q.W * kWideAlignSpan * sizeof(float);
    if (table + words > areas || 256 + areas > ctc_amd_workspace_bytes(CTC_AMD_BLANK, p.T, p.B, p.C, p.S))
        return CTC_AMD_ERR_UNSUPPORTED_SHAPE;
    q.a = p;
    const int rows_per_block = (kAlignGatherThreads / kWave) * kWideAlignGatherRows;
    const dim3 ggrid((p.T + rows_per_block - 1) / rows_per_block, p.B), gblock(kAlignGatherThreads);
    int rc;
    if (q.W == 2) rc = launch<blank_align_wide_gather_kernel<2>>(ggrid, gblock, 0, s, q);
    else if (q.W == 3) rc = launch<blank_align_wide_gather_kernel<3>>(ggrid, gblock, 0, s, q);
    else rc = launch<blank_align_wide_gather_kernel<4>>(ggrid, gblock, 0, s, q);
    if (rc) return rc;
    return launch<blank_align_wide_kernel>(dim3(p.B), dim3(q.W * kWave), 0, s, q);
}

}  // namespace ctc
