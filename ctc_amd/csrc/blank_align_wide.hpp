// Best path (Viterbi forced alignment) on blank-CTC lattices wider than one wave: 256 <= S <= 1023 labels,
// 513 <= 2S+1 <= 2047 states.  Included by blank_align.hip, which owns the arithmetic and the
// input rules (AlignParams, align_sample, align_label, align_state_value), the transition rule (align_skip_flag) and
// the step (align_select_step): the same select chain, wider.
// Two launches:
//   blank_table_gather_kernel          (bandwidth, every CU)  the table of blank_align.hip with NL = 256 W label columns.
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

struct AlignWideParams {
    AlignParams a;                   // inputs, shape, outputs, em (the table), spill (the back-pointer words)
    int W, NW;                       // waves per sample, back-pointer word rows per sample ((T + 1) / 2)
};

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

// The last two states of a sample, 2L and 2L-1 (state 0 twice when L = 0), may sit in two waves (2L = 512 w: the first
// state of wave w, 2L-1 the last of wave w-1): s_fin[0] = a(2L), s_fin[1] = a(2L-1), each from lane 0 of the wave that
// holds it.  The caller's barrier makes them visible.
__device__ __forceinline__ void wide_final_states(const float (&a)[kWideAlignK], int L, float (&s_fin)[2])
{
    const int sa = 2 * L, sb = L > 0 ? 2 * L - 1 : 0;
    if (sa / kWideAlignSpan == wave_id()) {
        const float x = align_state_value<kWideAlignK>(a, sa & (kWideAlignSpan - 1));
        if (lane_id() == 0) s_fin[0] = x;
    }
    if (sb / kWideAlignSpan == wave_id()) {
        const float x = align_state_value<kWideAlignK>(a, sb & (kWideAlignSpan - 1));
        if (lane_id() == 0) s_fin[1] = x;
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
    const int W = q.W, RW = align_row_pitch(K * W);
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
    for (int k = 0; k < K; ++k) skip[k] = align_skip_flag<true>(p, b, L, s0 + k, k);
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
    // one step (align_select_step with the edge of the wave below as the fill of the shift) into half `sub` of the word
    auto step = [&](int i, const AlignWideRow &e, int sub) {
        const float el[K / 2] = {e.el.x, e.el.y, e.el.z, e.el.w};
        align_select_step<K>(a, skip, el, e.eb, xch[i & 1][w], sub, word);    // (the fill is wave-uniform)
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

    wide_final_states(a, L, s_fin);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");              // this wave's back-pointer words have left it
    __syncthreads();
    if (w != 0) return;
    const int sa = 2 * L, sb = L > 0 ? 2 * L - 1 : 0;
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

// Where the wide read-outs' workspace lies (256 <= p.S <= 1023: the caller has checked).  W waves per sample; behind the
// 256-byte header the table em [B][T][256 W + 4], and behind the table `rest` bytes for the caller's rows: what is left
// of the three lattice areas of ctc_amd_workspace_bytes(CTC_AMD_BLANK, ...), 1536 W floats per (b, t).  Nothing is
// written to the header or behind the areas.
static int blank_wide_layout(AlignParams &p, int &W, size_t &rest)
{
    W = (2 * p.S + 1 + kWideAlignSpan - 1) / kWideAlignSpan;
    p.RW = align_row_pitch(kWideAlignK * W);
    p.em = reinterpret_cast<float *>(reinterpret_cast<char *>(p.counter) + 256);
    const size_t cells = (size_t)p.B * p.T;
    const size_t areas = 3 * cells * W * kWideAlignSpan * sizeof(float);
    if (256 + areas > ctc_amd_workspace_bytes(CTC_AMD_BLANK, p.T, p.B, p.C, p.S)) return CTC_AMD_ERR_UNSUPPORTED_SHAPE;
    rest = areas - cells * p.RW * sizeof(float);
    return 0;
}

// the table, then the back-pointer words: (256 W + 4) + 32 W words per (b, t) (+ 32 W per sample at odd T) of 1536 W
static int run_blank_align_wide(AlignParams &p, hipStream_t s)
{
    AlignWideParams q;
    size_t rest;
    const int rc = blank_wide_layout(p, q.W, rest);
    if (rc) return rc;
    q.NW = (p.T + 1) / 2;
    p.R = p.WL = 0;
    p.NWS = q.NW;
    p.spill = reinterpret_cast<unsigned *>(p.em + (size_t)p.B * p.T * p.RW);
    if ((size_t)p.B * q.NW * q.W * kWave * sizeof(unsigned) > rest) return CTC_AMD_ERR_UNSUPPORTED_SHAPE;
    q.a = p;
    return with_constant<2, 3, 4>(q.W, [&](auto w) {
        const int grc = launch_blank_table_gather<256 * decltype(w)::value, kWideAlignGatherRows, false>(p, s);
        return grc ? grc : launch<blank_align_wide_kernel>(dim3(p.B), dim3(q.W * kWave), 0, s, q);
    });
}

}  // namespace ctc
