// Scores of candidate label sequences, gfx950: scores[b, n] = log P(sequence n | sample b), summed over
// ALL alignments of the first T_b frames, for N candidates per sample in one launch -- on the blank lattice (x holds
// log-probabilities; torch.nn.CTCLoss's lattice) and on the no-blank lattice (blank < 0: x holds raw logits, the kernel
// subtracts each row's log-sum-exp; the loss's stay / advance lattice).  A forward pass only: no gradient, no workspace,
// no atomics, nothing between workgroups; every loop has a bound known at entry; every global store is a plain C++ store.
// It allocates nothing and never synchronises the host: safe under stream capture, deterministic.
//
// One workgroup per (sample, group of kSeqGroup candidates): kSeqLoaders loader waves and one chain wave per candidate,
// which meet at one __syncthreads() per tile of F frames.
//   loader waves   bring tile k + 1 (F frames x C columns, a quarter of the rows to each wave, every dword of a wave's
//                  share in flight at once) into the LDS buffer the chains are NOT reading, and on the no-blank
//                  lattice reduce each of their rows' log2-sum-exp2 there, once for all candidates.
//   chain waves    hold their candidate's lattice in registers, 1 / 2 / 4 / 8 consecutive states per lane (S <= 64 / 128 /
//                  256 / 511 states: S = len on the no-blank lattice, 2 len + 1 on the blank one), the column of every
//                  state beside it.  A frame: one LDS gather per state (the blank states of a lane share one broadcast
//                  read), the neighbour states of the lane below by DPP wave_shr, the skip transition masked where the
//                  labels two states apart are equal, log2-sum-exp2 of the two or three predecessors plus the emission.
// Arithmetic: log2-domain fp32.  Every kSeqRenorm frames a chain subtracts floor(max state) from its states and adds it to
// a double, a sum of integers (exact).  The maximum is over the candidate's OWN states: the states beyond S that a lane
// holds are kept at -inf (their emission is), or they would sum paths that are no alignments, outgrow the real states
// without bound and drag the offset after them.  So the largest state stays within 8 frames' emissions of 0, and a state d
// below it is rounded at the size of d: one that still reaches the read-out makes a score of magnitude >= d ln 2, which
// is what the tolerance is relative to.  The read-out is ln 2 (offset + log2-sum-exp2 of the last state(s)), in double.
//
// C > kSeqStagedMaxC (a wave's share of one row no longer fits a loader lane's registers, two rows hardly fit the LDS): the
// same kernel without the staging -- chains gather from global memory, loaders reduce the rows' log-sum-exp straight from
// it.  Correct for any C; slow, and said so in DESIGN.md.
//
// This header holds the kernel and its launch plan; sequence_scores.hip has the forward entry.  sequence_scores_grad.hip
//  launches the same kernel with a row sink: the chain then stores its states, their emissions and the
// offset in force after every frame -- the same instructions in the same order in front of the stores, so the scores are
// the forward entry's bits.
#pragma once
#include <limits.h>

#include "common.hpp"
#include "launch.hpp"

namespace ctc {

constexpr int kSeqLoaders = 4;                                  // loader waves
constexpr int kSeqGroup = 8;                                    // G: chain waves = candidates of a workgroup
constexpr int kSeqThreads = (kSeqLoaders + kSeqGroup) * kWave;
constexpr int kSeqMaxL = 255;                                   // labels of a candidate: 511 blank-lattice states, 8 per lane
constexpr int kSeqLoadRegs = 64;                                // dwords a loader lane has in flight per tile
constexpr int kSeqStagedMaxC = kSeqLoadRegs * kWave;            // 4096: one row is at most a wave's whole share
constexpr int kSeqMaxFrames = 32;                               // F <= this (and a multiple of kSeqLoaders)
constexpr int kSeqDirectFrames = 16;                            // F of the unstaged kernel
constexpr size_t kSeqLdsBudget = 152 * 1024;
constexpr int kSeqRenorm = 8;                                   // frames between two renormalisations (a power of two)
constexpr int kSeqLseRegs = 16;                                 // columns per lane and pass of the row reduction

struct SeqParams {
    const float *x;                             // [T][B][C] through (st, sb), unit class stride
    int64_t st, sb;
    const int64_t *in_len;
    int T, B, C, blank;
    const void *seq;                            // labels at [b seq_sb + n seq_sn + i], int32 or int64
    int is64;
    int64_t seq_sb, seq_sn;
    int L;
    const int64_t *len;                         // at [b len_sb + n]
    int64_t len_sb;
    const int32_t *count;                       // [B] or NULL
    int N, groups, F;
    float *scores;                              // [B][N]
    // the row sink of the gradient entry (unused by the forward one): per candidate b N + n, [T] offsets and [T][SL] rows
    double *sink_off = nullptr;
    float *sink_a = nullptr, *sink_e = nullptr;
    int SL = 0;
};

// What a chain does with the row it has just finished.  The forward entry: nothing.
struct SeqNoSink {
    template <int K>
    __device__ __forceinline__ void row(int, const float (&)[K], const float (&)[K], double) const {}
};
// The gradient entry: states s < S of frame t (log2 domain, after the frame's renormalisation), their emissions, and the
// offset the states are relative to.  State s = lane K + j lies at [t SL + s]: a lane's K floats are consecutive.
struct SeqRowSink {
    float *a, *e;
    double *off;
    int S, SL;
    template <int K>
    __device__ __forceinline__ void row(int t, const float (&av)[K], const float (&ev)[K], double offset) const
    {
        const int lane = lane_id();
        float *ra = a + (int64_t)t * SL, *re = e + (int64_t)t * SL;
#pragma unroll
        for (int j = 0; j < K; ++j) {
            const int s = lane * K + j;
            if (s < S) { ra[s] = av[j]; re[s] = ev[j]; }
        }
        if (lane == 0) off[t] = offset;
    }
};

__device__ __forceinline__ int64_t seq_label(const void *q, int is64, int i)
{
    return is64 ? static_cast<const int64_t *>(q)[i] : (int64_t) static_cast<const int32_t *>(q)[i];
}

// log2(2^a + 2^b [+ 2^c]); -inf where all are
__device__ __forceinline__ float seq_lse2(float a, float b)
{
    const float m = fmaxf(a, b), mm = m == -__builtin_inff() ? 0.0f : m;
    return mm + __builtin_amdgcn_logf(__builtin_amdgcn_exp2f(a - mm) + __builtin_amdgcn_exp2f(b - mm));
}
__device__ __forceinline__ float seq_lse3(float a, float b, float c)
{
    const float m = fmaxf(fmaxf(a, b), c), mm = m == -__builtin_inff() ? 0.0f : m;
    return mm + __builtin_amdgcn_logf(__builtin_amdgcn_exp2f(a - mm) + __builtin_amdgcn_exp2f(b - mm) +
                                      __builtin_amdgcn_exp2f(c - mm));
}

// State j - d (d = 1, 2) of a lane that holds a[0 .. K): its own register, or what came from the lane below -- `last`
// that lane's state K - 1, `last2` its state K - 2 (needed by K = 1 alone, where it is the lane two below).
template <int K>
__device__ __forceinline__ float seq_below(const float (&a)[K], int j, int d, float last, float last2)
{
    if (j >= d) return a[j - d];
    return j - d == -1 ? last : last2;
}

// log2 of the sum of exp over row[0 .. C) (LDS or global), by one wave: 1024 columns per pass, a running (max, sum) between
// passes as in beam_search.hip.  Wave-uniform.
__device__ __forceinline__ float seq_row_lse2(const float *row, int C, int lane)
{
    const float ninf = -__builtin_inff();
    float wmax = ninf, wsum = 0.0f;
    for (int c0 = 0; c0 < C; c0 += kSeqLseRegs * kWave) {
        float u[kSeqLseRegs];
        float m = ninf;
#pragma unroll
        for (int i = 0; i < kSeqLseRegs; ++i) {
            const int c = c0 + i * kWave + lane;
            u[i] = c < C ? row[c] : ninf;
            m = fmaxf(m, u[i]);
        }
        m = fmaxf(wave_max(m), wmax);
        if (m > ninf) {
            float s = 0.0f;
#pragma unroll
            for (int i = 0; i < kSeqLseRegs; ++i) s += fast_exp(u[i] - m);
            wsum = wsum * fast_exp(wmax - m) + wave_sum(s);
            wmax = m;
        }
    }
    return __builtin_fmaf(wmax, kLog2e, __builtin_amdgcn_logf(wsum));
}

// Tile k of the sample: frames [k F, k F + rows) into tile[(k & 1) F C ...] (STAGED), their log2-sum-exp2 into
// lse[(k & 1) F ...] (the no-blank lattice).  Loader wave lw takes rows [lw F / 4, (lw + 1) F / 4) of the tile.
template <int STAGE, bool BLANK>
__device__ __forceinline__ void seq_load_tile(const SeqParams &p, const float *xb, int Tb, float *tile, float *lse, int k,
                                              int lw, int lane)
{
    constexpr bool STAGED = STAGE != 0;
    constexpr int VEC = STAGE == 4 ? 4 : 1;
    const int F = p.F, C = p.C, t0 = k * F, rows = min(F, Tb - t0), RW = F / kSeqLoaders;
    const int r0 = lw * RW, r1 = min(r0 + RW, rows);            // this wave's rows of the tile: [r0, r1)
    float *tl = tile + (k & 1) * F * C;
    if (STAGED && r0 < r1) {
        // The share is RW C consecutive floats of the tile (RW C <= 64 kSeqLoadRegs: the entry chose F so): piece e, of
        // VEC floats, is columns [e % C, e % C + VEC) of row r0 + e / C -- VEC = 4 only where C, the strides and the base
        // are multiples of 4 floats, so a piece never straddles two rows.  kPass pieces per lane are in flight at once.
        // No predicates: a piece beyond the share repeats the last one (the same bytes to the same place), a row beyond
        // T_b repeats frame T_b - 1 into a row nobody reads.
        typedef float piece_t __attribute__((ext_vector_type(VEC)));
        constexpr int kPass = VEC == 4 ? kSeqLoadRegs / 4 : kSeqLoadRegs / 2;   // 16 x 16 bytes (the whole share), or 32 dwords
        const int share = RW * C;
        const float inv_c = 1.0f / (float)C;
        float *dst = tl + r0 * C;
        const float *src = xb + (int64_t)(t0 + r0) * p.st;
        const int last_row = Tb - 1 - (t0 + r0);
        for (int base = 0; base < share; base += kPass * kWave * VEC) {
            piece_t v[kPass];
#pragma unroll
            for (int q = 0; q < kPass; ++q) {
                const int e = min(base + (q * kWave + lane) * VEC, share - VEC);
                const int rr = (int)(((float)e + 0.5f) * inv_c);        // e / C, exact for e < 2^21
                const int c = e - rr * C;
                v[q] = *reinterpret_cast<const piece_t *>(src + (int64_t)min(rr, last_row) * p.st + c);
            }
#pragma unroll
            for (int q = 0; q < kPass; ++q)
                *reinterpret_cast<piece_t *>(dst + min(base + (q * kWave + lane) * VEC, share - VEC)) = v[q];
        }
    }
    if constexpr (!BLANK) {
        for (int r = r0; r < r1; ++r) {
            lds_order();                                        // (this wave's own row, written above: LDS is in order)
            const float l2 = STAGED ? seq_row_lse2(tl + r * C, C, lane)
                                    : seq_row_lse2(xb + (int64_t)(t0 + r) * p.st, C, lane);
            if (lane == 0) lse[(k & 1) * F + r] = l2;
        }
    }
}

template <int STAGE, bool BLANK>
__device__ __forceinline__ void seq_loader(const SeqParams &p, const float *xb, int Tb, float *tile, float *lse, int lw)
{
    const int ntiles = (Tb + p.F - 1) / p.F, lane = lane_id();
    if (ntiles > 0) seq_load_tile<STAGE, BLANK>(p, xb, Tb, tile, lse, 0, lw, lane);
    __syncthreads();
    for (int k = 0; k < ntiles; ++k) {
        if (k + 1 < ntiles) seq_load_tile<STAGE, BLANK>(p, xb, Tb, tile, lse, k + 1, lw, lane);
        __syncthreads();
    }
}

// a wave without a candidate keeps the workgroup's barriers company
__device__ __forceinline__ void seq_idle(int Tb, int F)
{
    const int ntiles = (Tb + F - 1) / F;
    for (int k = 0; k <= ntiles; ++k) __syncthreads();
}

// The forward chain of one candidate (labels q[0 .. len), 0 <= len <= L), K states per lane: state s = lane K + j.
// -> log P in natural log (-inf: no alignment); `bad`: a label outside [0, C) or equal to the blank (wave-uniform).
// T_b >= 1 is the caller's business; the barriers are executed whatever the candidate is.
template <int STAGE, bool BLANK, int K, class Sink>
__device__ __forceinline__ float seq_chain(const SeqParams &p, const float *xb, int Tb, const float *tile, const float *lse,
                                           const void *q, int len, bool &bad, const Sink &sink)
{
    constexpr bool STAGED = STAGE != 0;
    const float ninf = -__builtin_inff();
    const int lane = lane_id(), C = p.C, F = p.F, S = BLANK ? 2 * len + 1 : len;
    int col[K];
    bool skip[K];
    float dead[K];                                              // 0, or -inf for a state beyond S: added to its emission
    bool wrong = false;
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const int s = lane * K + j;
        const bool is_label = BLANK ? (s & 1) != 0 : true;
        const int i = BLANK ? (s - 1) >> 1 : s;
        int c = BLANK ? p.blank : 0;                            // (states beyond S: any column inside the row)
        skip[j] = false;
        dead[j] = s < S ? 0.0f : ninf;
        if (is_label && i < len) {
            const int64_t lab = seq_label(q, p.is64, i);
            if (BLANK && i >= 1) skip[j] = seq_label(q, p.is64, i - 1) != lab;
            if (lab < 0 || lab >= C || lab == p.blank) wrong = true;
            else c = (int)lab;                                  // (memory safety: a gather never leaves the row)
        }
        col[j] = c;
    }
    bad = __any(wrong) != 0;

    float a[K], e[K], en[K];
#pragma unroll
    for (int j = 0; j < K; ++j) { a[j] = ninf; en[j] = ninf; }
    double offset = 0.0;

    // emissions of frame f of the tile, log2 domain
    auto gather = [&](float (&o)[K], const float *tl, const float *ls, int t, int f) {
        const float *row = STAGED ? tl + f * C : xb + (int64_t)t * p.st;
        float shared_blank = 0.0f, l2 = 0.0f;
        if constexpr (BLANK && K >= 2) shared_blank = row[p.blank];
        if constexpr (!BLANK) l2 = ls[f];
#pragma unroll
        for (int j = 0; j < K; ++j) {
            float raw;
            if (BLANK && K >= 2 && (j & 1) == 0) raw = shared_blank;
            else raw = row[col[j]];
            // a state beyond S is held at -inf: it would be fed from the last state and sum paths that are no alignments,
            // and the renormalisation below must follow the candidate's own states alone
            o[j] = BLANK ? __builtin_fmaf(raw, kLog2e, dead[j]) : __builtin_fmaf(raw, kLog2e, -l2) + dead[j];
        }
    };

    const int ntiles = (Tb + F - 1) / F;
    __syncthreads();                                            // tile 0 is there
    for (int k = 0; k < ntiles; ++k) {
        const int t0 = k * F, nf = min(F, Tb - t0);
        const float *tl = tile + (k & 1) * F * C, *ls = lse + (k & 1) * F;
        gather(en, tl, ls, t0, 0);
        for (int f = 0; f < nf; ++f) {
            const int t = t0 + f;
#pragma unroll
            for (int j = 0; j < K; ++j) e[j] = en[j];
            if (f + 1 < nf) gather(en, tl, ls, t + 1, f + 1);   // in flight across this frame's step
            if (t == 0) {
#pragma unroll
                for (int j = 0; j < K; ++j) {
                    const int s = lane * K + j;
                    a[j] = (s == 0 || (BLANK && s == 1)) ? e[j] : ninf;
                }
            } else {
                // state s - 1 and s - 2 of the lane's state j: its own registers, or the last ones of the lane below
                const float p1 = wave_shr1(a[K - 1], ninf);     // state lane K - 1
                float p2 = ninf;                                // state lane K - 2: K = 1 alone skips across two lanes
                if constexpr (BLANK && K == 1) p2 = wave_shr1(p1, ninf);
                float nw[K];
#pragma unroll
                for (int j = 0; j < K; ++j) {
                    const float x1 = seq_below<K>(a, j, 1, p1, p2);
                    if (BLANK && (K == 1 || (j & 1) != 0)) {    // (K >= 2: the even states of a lane are blanks, no skip)
                        const float x2 = seq_below<K>(a, j, 2, p1, p2);
                        nw[j] = seq_lse3(a[j], x1, skip[j] ? x2 : ninf) + e[j];
                    } else {
                        nw[j] = seq_lse2(a[j], x1) + e[j];
                    }
                }
#pragma unroll
                for (int j = 0; j < K; ++j) a[j] = nw[j];
            }
            if ((t & (kSeqRenorm - 1)) == kSeqRenorm - 1) {
                float m = a[0];
#pragma unroll
                for (int j = 1; j < K; ++j) m = fmaxf(m, a[j]);
                m = wave_max(m);
                if (m > ninf) {
                    const float fl = floorf(m);
#pragma unroll
                    for (int j = 0; j < K; ++j) a[j] -= fl;
                    offset += (double)fl;
                }
            }
            sink.row(t, a, e, offset);
        }
        __syncthreads();                                        // the other buffer is full, this one is free
    }

    // read-out: the last state, on the blank lattice the last two
    float v = ninf;
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const int s = lane * K + j;
        if (s == S - 1 || (BLANK && s == S - 2)) v = fmaxf(v, a[j]);
    }
    const float M = wave_max(v);
    if (!(M > ninf)) return ninf;
    float sum = 0.0f;
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const int s = lane * K + j;
        if (s == S - 1 || (BLANK && s == S - 2)) sum += __builtin_amdgcn_exp2f(a[j] - M);
    }
    sum = wave_sum(sum);
    const double l2 = offset + (double)M + (double)__builtin_amdgcn_logf(sum);
    return (float)(l2 * 0.69314718055994530942);
}

template <int STAGE, bool BLANK, int K, bool STORE>
__device__ __forceinline__ float seq_chain_of(const SeqParams &p, const float *xb, int Tb, const float *tile,
                                              const float *lse, const void *q, int len, bool &bad, int64_t cand)
{
    if constexpr (STORE) {
        const int64_t rows = cand * p.T;
        const SeqRowSink sink{p.sink_a + rows * p.SL, p.sink_e + rows * p.SL, p.sink_off + rows, BLANK ? 2 * len + 1 : len,
                              p.SL};
        return seq_chain<STAGE, BLANK, K>(p, xb, Tb, tile, lse, q, len, bad, sink);
    } else {
        return seq_chain<STAGE, BLANK, K>(p, xb, Tb, tile, lse, q, len, bad, SeqNoSink{});
    }
}

template <int STAGE, bool BLANK, bool STORE = false>
__global__ __launch_bounds__(kSeqThreads) void sequence_scores_kernel(SeqParams p)
{
    extern __shared__ float4 smem_raw[];
    float *tile = reinterpret_cast<float *>(smem_raw);          // staged: [2][F][C]
    float *lse = tile + (STAGE != 0 ? 2 * p.F * p.C : 0);       // [2][F]
    const int wave = wave_id();
    const int g = blockIdx.x % p.groups, b = blockIdx.x / p.groups;
    const int64_t Tb64 = p.in_len[b];
    const int Tb = Tb64 < 0 ? 0 : (Tb64 > p.T ? p.T : (int)Tb64);       // (memory safety: never beyond the tensor)
    const float *xb = p.x + (int64_t)b * p.sb;

    if (wave < kSeqLoaders) {
        seq_loader<STAGE, BLANK>(p, xb, Tb, tile, lse, wave);
        return;
    }
    const int n = g * kSeqGroup + (wave - kSeqLoaders);
    if (n >= p.N) {
        seq_idle(Tb, p.F);
        return;
    }
    const float ninf = -__builtin_inff(), nan = __builtin_nanf("");
    const bool absent = p.count != nullptr && n >= p.count[b];
    int64_t len64 = 0;
    if (!absent) len64 = p.len[(int64_t)b * p.len_sb + n];
    const bool bad_len = len64 < 0 || len64 > p.L;
    const int len = __builtin_amdgcn_readfirstlane(bad_len ? 0 : (int)len64);
    const char *q = static_cast<const char *>(p.seq) +
                    ((int64_t)b * p.seq_sb + (int64_t)n * p.seq_sn) * (p.is64 ? 8 : 4);
    const int S = BLANK ? 2 * len + 1 : len;
    bool bad = false;
    float val;
    const int64_t cand = (int64_t)b * p.N + n;
    if (S <= kWave) val = seq_chain_of<STAGE, BLANK, 1, STORE>(p, xb, Tb, tile, lse, q, len, bad, cand);
    else if (S <= 2 * kWave) val = seq_chain_of<STAGE, BLANK, 2, STORE>(p, xb, Tb, tile, lse, q, len, bad, cand);
    else if (S <= 4 * kWave) val = seq_chain_of<STAGE, BLANK, 4, STORE>(p, xb, Tb, tile, lse, q, len, bad, cand);
    else val = seq_chain_of<STAGE, BLANK, 8, STORE>(p, xb, Tb, tile, lse, q, len, bad, cand);
    if (Tb == 0) val = len == 0 ? 0.0f : ninf;
    if (bad) val = nan;
    if (bad_len) val = nan;
    if (absent) val = ninf;
    if (lane_id() == 0) p.scores[(int64_t)b * p.N + n] = val;
}

// The launch of a filled SeqParams (everything but F): the staging, F and the LDS from C, the strides and the base.
// STORE: the kernel with the row sink (staged shapes only: the gradient entry refuses the others before it gets here).
template <bool STORE>
inline int seq_launch(SeqParams p, hipStream_t s)
{
    const int C = p.C, N = p.N;
    const bool staged = C <= kSeqStagedMaxC;
    const bool vec4 = C % 4 == 0 && p.st % 4 == 0 && p.sb % 4 == 0 && reinterpret_cast<uintptr_t>(p.x) % 16 == 0;
    size_t lds;
    if (staged) {
        // F: a multiple of the loader waves; a wave's share (F / 4 rows: F C / 256 dwords per lane) fits its registers;
        // two tiles fit the LDS.  C = 158: 32 frames, C = 1000: 16, C = 4096: 4.
        int F = kSeqLoaders * kSeqLoadRegs * kWave / C;
        const int fit = (int)(kSeqLdsBudget / (2 * sizeof(float) * (size_t)C));
        F = (F < fit ? F : fit) & ~(kSeqLoaders - 1);
        p.F = F < kSeqMaxFrames ? F : kSeqMaxFrames;
        lds = (2 * (size_t)p.F * C + 2 * p.F) * sizeof(float);
    } else {
        p.F = kSeqDirectFrames;
        lds = 2 * p.F * sizeof(float);
    }
    const int chains = N < kSeqGroup ? N : kSeqGroup;           // waves that would have no candidate are not launched
    const dim3 grid((unsigned)((int64_t)p.groups * p.B)), block((kSeqLoaders + chains) * kWave);
    if (staged && vec4) {
        return p.blank >= 0 ? launch<sequence_scores_kernel<4, true, STORE>>(grid, block, lds, s, p)
                            : launch<sequence_scores_kernel<4, false, STORE>>(grid, block, lds, s, p);
    }
    if (staged) {
        return p.blank >= 0 ? launch<sequence_scores_kernel<1, true, STORE>>(grid, block, lds, s, p)
                            : launch<sequence_scores_kernel<1, false, STORE>>(grid, block, lds, s, p);
    }
    if constexpr (STORE) {
        return CTC_AMD_ERR_UNSUPPORTED_SHAPE;
    } else {
        return p.blank >= 0 ? launch<sequence_scores_kernel<0, true>>(grid, block, lds, s, p)
                            : launch<sequence_scores_kernel<0, false>>(grid, block, lds, s, p);
    }
}

}  // namespace ctc
