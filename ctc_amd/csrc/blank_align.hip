// Best-path (Viterbi) forced alignment on the blank-CTC lattice, gfx950.
//
// The max-semiring twin of the blank loss recursion (blank.hip): extended labels l'_s, s = 0..2L (even s = blank,
// odd s = targets[(s-1)/2]), used as given (no normalisation):
//   v_0(0) = lp[0,blank], v_0(1) = lp[0,l'_1], every other state -inf;
//   v_t(s) = best(v_{t-1}(s), v_{t-1}(s-1), [v_{t-1}(s-2) if l'_s != blank and l'_s != l'_{s-2}]) + lp[t,l'_s],
// candidates taken in the order stay, advance, skip, a later one replacing the current one only when strictly
// greater; one fp32 add per step in natural log, -inf kept as -inf.  The read-out is state 2L when
// v(2L) > v(2L-1) (strictly), else 2L-1 (state 0 when L = 0); the path is the walk back over the back-pointers.
// Every step is one select chain and one add, so a float32 restatement run in the same order is bit-identical.
//
// Two launches:
//   blank_table_gather_kernel   (bandwidth, every CU)  em[b,t,:] = lp[t,b,{l_0 .. l_{NL-1}, blank}] (labels j >= L
//                               -> -inf): the 4 KB rows of log_probs are read once, all CUs at once, into a
//                               compact [B][T][NL + 4] table in the workspace (NL = 32K label columns; the layout is
//                               stated once, at the kernel).  Every read-out of this file starts from it.
//   blank_align_kernel<K>       (latency, one 512-thread workgroup per sample)  wave 0 runs the max-plus scan,
//                               K states per lane, the two lower neighbours of a lane's first states through ONE DPP
//                               wave shift; waves 1..7 copy the compact rows into an LDS ring ahead of it.  Back-pointers
//                               are 2 bits per state and step, packed per lane into one 32-bit word per 16/K steps
//                               (16 K bytes per step): in LDS while they fit, in the workspace beyond.  Wave 0 then
//                               walks them back with one readlane per step and writes the path 64 steps per store.
// These take 2S+1 <= 512 states (S <= 255); blank_align_wide.hpp, included below, takes 513..2047 with several waves
// per sample (ctc_amd_blank_best_path_wide).  blank_spans.hpp, included last, turns the path and the posteriors into
// one record per target label (ctc_amd_blank_token_spans).
#include "common.hpp"
#include "launch.hpp"

namespace ctc {

constexpr int kAlignThreads = 512;
constexpr int kAlignWaves = kAlignThreads / kWave;
constexpr int kAlignLoaders = kAlignWaves - 1;   // loader waves (1..7)
constexpr int kAlignHead = 64;                   // ints of LDS flags in front of the ring
constexpr int kAlignSpinLimit = 1 << 23;         // polls of an LDS flag (~0.1 us apart: ~1 s) before a wave gives up
constexpr int kAlignWalkWords = 16;              // back-pointer words per lane fetched ahead of the walk back
constexpr int kAlignGatherRows = 8;              // rows per wave of the gather launch
constexpr int kAlignGatherThreads = 256;
// LDS flag slots (ints): [0, 7) rows written per loader, 8 rows taken by the scan, 9 abort
constexpr int kSlotTaken = 8, kSlotAbort = 9;

struct AlignParams {
    const float *lp;
    int64_t st, sb;
    const void *tgt;
    int tgt64;
    const int64_t *in_len, *tgt_len;
    int T, B, C, S, blank;
    int32_t *path;
    float *score;
    unsigned *counter;               // the workspace header (status word)
    float *em;                       // [B][T][RW] emission rows
    unsigned *spill;                 // [B][NWS][64] back-pointer words that do not fit in LDS
    int RW, R, WL, NWS;              // row pitch (floats), ring rows (power of two), LDS word rows, spilled word rows
};

__host__ __device__ constexpr int align_steps_per_word(int K) { return 16 / K; }

__device__ __forceinline__ bool align_sample(const AlignParams &p, int b, int &Tb, int &L)
{
    const int64_t Tb64 = p.in_len[b], L64 = p.tgt_len[b];
    const bool ok = L64 >= 0 && L64 <= p.S && Tb64 >= 1 && Tb64 <= p.T;
    Tb = ok ? (int)Tb64 : 0;
    L = ok ? (int)L64 : 0;
    return ok;
}

__device__ __forceinline__ int align_label(const AlignParams &p, int b, int j)
{
    const int c = load_label(p.tgt, p.tgt64, (int64_t)b * p.S + j);
    return c < 0 ? 0 : (c >= p.C ? p.C - 1 : c);             // memory safety for bad labels
}

// ---- launch 1: the compact emission table -------------------------------------------------------
// THE table of every read-out here, narrow and wide: em [B][T][NL + 4] floats, NL label columns (32 K narrow, 256 W
// wide).  Row (b, t): columns j < NL = lp[t, b, l_j] (-inf for labels j >= L_b), column NL = lp[t, b, blank], column
// NL + 1 = the row's emission maximum c_t when CMAX (over the blank and the L_b labels, 0 for a row without a finite
// emission; the wide posteriors' chains read it), else -inf like the rest of the padding.  Rows t >= T_b are not written.
// grid (ceil(T / (4 * ROWS)), B); a wave takes ROWS rows, a row's NL + 4 columns dealt over its lanes in M passes, all
// loads in flight at once
__host__ __device__ constexpr int align_row_pitch(int K) { return 32 * K + 4; }   // NL + 4 at K states per lane
template <int NL, int ROWS, bool CMAX>
__global__ __launch_bounds__(kAlignGatherThreads) void blank_table_gather_kernel(AlignParams p)
{
    constexpr int RW = NL + 4, M = (RW + kWave - 1) / kWave;
    static_assert(!CMAX || ROWS == 4, "one wave_max4 for the rows of a wave");
    const int b = blockIdx.y, lane = lane_id();
    int Tb, L;
    if (!align_sample(p, b, Tb, L)) return;
    const int t0 = (blockIdx.x * (kAlignGatherThreads / kWave) + wave_id()) * ROWS;
    if (t0 >= Tb) return;                                         // (wave-uniform)
    int col[M];
#pragma unroll
    for (int m = 0; m < M; ++m) {
        const int j = lane + kWave * m;
        col[m] = j < L ? align_label(p, b, j) : (j == NL ? p.blank : -1);
    }
    const float *__restrict__ lp = p.lp + (int64_t)b * p.sb;
    float v[ROWS][M], cm[ROWS];
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
        const int t = min(t0 + r, Tb - 1);
#pragma unroll
        for (int m = 0; m < M; ++m) v[r][m] = lp[(int64_t)t * p.st + (col[m] >= 0 ? col[m] : p.blank)];
    }
    if constexpr (CMAX) {
#pragma unroll
        for (int r = 0; r < ROWS; ++r) {
            cm[r] = -__builtin_inff();
#pragma unroll
            for (int m = 0; m < M; ++m) {
                v[r][m] = col[m] >= 0 ? v[r][m] : -__builtin_inff();
                cm[r] = fmaxf(cm[r], v[r][m]);
            }
        }
        wave_max4(cm[0], cm[1], cm[2], cm[3]);
    }
    float *__restrict__ out = p.em + ((int64_t)b * p.T + t0) * RW;
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
        if (t0 + r >= Tb) break;
        float c = 0.f;                                            // (a row without a finite emission: post_row_max4)
        if constexpr (CMAX) c = cm[r] > -__builtin_inff() ? cm[r] : c;
#pragma unroll
        for (int m = 0; m < M; ++m) {
            const int j = lane + kWave * m;
            if constexpr (CMAX) {
                if (j < RW) out[r * RW + j] = j == NL + 1 ? c : v[r][m];
            } else {
                if (j < RW) out[r * RW + j] = col[m] >= 0 ? v[r][m] : -__builtin_inff();
            }
        }
    }
}

template <int NL, int ROWS, bool CMAX>
static int launch_blank_table_gather(const AlignParams &p, hipStream_t s)
{
    const int rows_per_block = (kAlignGatherThreads / kWave) * ROWS;
    return launch<blank_table_gather_kernel<NL, ROWS, CMAX>>(dim3((p.T + rows_per_block - 1) / rows_per_block, p.B),
                                                             dim3(kAlignGatherThreads), 0, s, p);
}

// ---- launch 2: scan + walk back ------------------------------------------------------------------
__device__ __forceinline__ int align_load(const int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ void align_store(int *p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

// loader wave i: rows t = i, i + 7, i + 14, ... of the sample, kAlignLoadRows in flight, each into ring slot t % R once
// the scan has taken row t - R.  false: a wait ran out (or the scan gave up)
template <int K>
__device__ __forceinline__ bool align_loader(const AlignParams &p, int *flags, float *ring, int b, int Tb, int i)
{
    constexpr int RW = align_row_pitch(K), M = (RW + kWave - 1) / kWave;
    // rows a loader wave keeps in flight: the seven loaders hold ~100 rows against the latency of the table (4 rows each
    // measured the same at config 5, 347 against 346 us: the scan does not wait for its loaders there)
    constexpr int kAlignLoadRows = K == 8 ? 8 : 16;
    const int lane = lane_id();
    const float *src = p.em + (int64_t)b * p.T * RW;
    int taken = 0;
    for (int q0 = 0; i + q0 * kAlignLoaders < Tb; q0 += kAlignLoadRows) {
        float v[kAlignLoadRows][M];
#pragma unroll
        for (int d = 0; d < kAlignLoadRows; ++d) {
            const int t = min(i + (q0 + d) * kAlignLoaders, Tb - 1);
#pragma unroll
            for (int m = 0; m < M; ++m) v[d][m] = src[(int64_t)t * RW + min(lane + kWave * m, RW - 1)];
        }
#pragma unroll
        for (int d = 0; d < kAlignLoadRows; ++d) {
            const int t = i + (q0 + d) * kAlignLoaders;
            if (t >= Tb) break;
            if (t - p.R >= taken) {                                  // the slot still holds row t - R: wait for the scan
                bool ok = false;
                for (int it = 0; it < kAlignSpinLimit; ++it) {
                    taken = align_load(flags + kSlotTaken);
                    if (t - p.R < taken) { ok = true; break; }
                    if (align_load(flags + kSlotAbort)) break;
                    __builtin_amdgcn_s_sleep(1);
                }
                if (!ok) return false;
            }
            float *dst = ring + (t & (p.R - 1)) * RW;
#pragma unroll
            for (int m = 0; m < M; ++m)
                if (lane + kWave * m < RW) dst[lane + kWave * m] = v[d][m];
            lds_order();                                             // (a wave's LDS operations complete in order)
            align_store(flags + i, q0 + d + 1);
        }
    }
    return true;
}

// THE transition rule: a label state s (odd) may be entered from s - 2 when its class is no blank and differs from that
// of s - 2.  The flag of state s, k = s % K (even k are blanks: a lane's first state is even): FWD, s takes from s - 2
// (the scans, alpha); !FWD, s takes from s + 2 under the same rule for s + 2 (beta').  (One flag per call, the loop over
// k at the call site: a routine that fills the whole array moves the instructions of every scan and chain kernel.)
template <bool FWD>
__device__ __forceinline__ bool align_skip_flag(const AlignParams &p, int b, int L, int s, int k)
{
    bool sk = false;
    if ((k & 1) && (FWD ? (s >= 3 && s <= 2 * L - 1) : (s + 2 <= 2 * L - 1))) {
        const int c1 = align_label(p, b, (s - 1) >> 1), c2 = align_label(p, b, FWD ? (s - 3) >> 1 : (s + 1) >> 1);
        sk = FWD ? (c1 != p.blank && c1 != c2) : (c2 != p.blank && c2 != c1);
    }
    return sk;
}

// THE max-plus step of K states per lane: the select chain stay -> advance -> skip, one add; the 2-bit back-pointer
// codes go into step `sub` of `word`.  el[j] = the emission of label state 2 j + 1, eb = the blank's; `fill` = the state
// below the wave's first (-inf, or the edge of the wave below: blank_align_wide.hpp)
template <int K>
__device__ __forceinline__ void align_select_step(float (&a)[K], const bool (&skip)[K], const float (&el)[K / 2], float eb,
                                                  float fill, int sub, unsigned &word)
{
    const float nb = wave_shr1(a[K - 1], fill);
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
        n[k] = best + ((k & 1) ? el[k / 2] : eb);
        word |= c << (2 * K * sub + 2 * k);
    }
#pragma unroll
    for (int k = 0; k < K; ++k) a[k] = n[k];
}

// the emissions of one step in the scan's registers: el[j] = label (lane K/2 + j), eb = blank
template <int K>
struct AlignRow {
    float el[K / 2];
    float eb;
};

template <int K>
__device__ __forceinline__ void align_read_row(const float *ring, int R, int t, AlignRow<K> &r)
{
    constexpr int RW = align_row_pitch(K);
    const float *row = ring + (t & (R - 1)) * RW;
    const int lane = lane_id();
    if constexpr (K == 2) {
        r.el[0] = row[lane];
    } else if constexpr (K == 4) {
        const float2 x = reinterpret_cast<const float2 *>(row)[lane];
        r.el[0] = x.x; r.el[1] = x.y;
    } else {
#pragma unroll
        for (int q = 0; q < K / 2; q += 4) {
            const float4 x = reinterpret_cast<const float4 *>(row)[lane * (K / 8) + q / 4];
            r.el[q] = x.x; r.el[q + 1] = x.y; r.el[q + 2] = x.z; r.el[q + 3] = x.w;
        }
    }
    r.eb = row[32 * K];
}

// value of state s (wave-uniform) from the lane that holds it
template <int K>
__device__ __forceinline__ float align_state_value(const float (&a)[K], int s)
{
    // every register read out first, the choice among them made on wave-uniform values (a select among the a[k]
    // by a runtime k becomes an indexed access to a stack copy of a[])
    const int kk = s & (K - 1);
    int x = __builtin_amdgcn_readlane(__builtin_bit_cast(int, a[0]), s / K);
#pragma unroll
    for (int k = 1; k < K; ++k) {
        const int y = __builtin_amdgcn_readlane(__builtin_bit_cast(int, a[k]), s / K);
        x = kk == k ? y : x;
    }
    return __builtin_bit_cast(float, x);
}

template <int K>
struct AlignScan {
    static constexpr int P = align_steps_per_word(K);            // steps per back-pointer word
    static constexpr int G = K == 8 ? 8 : 16;                    // steps per group (a multiple of P)
    int R, WL;                                                   // (copies: a reference to the kernel argument goes to scratch)
    int *flags;
    const float *ring;
    unsigned *bp;                                                // [WL][64] in LDS
    unsigned *spill;                                             // [NWS][64] of this sample
    int Tb, ready;
    float a[K];
    bool skip[K];

    __device__ __forceinline__ AlignScan(const AlignParams &p, int *f, const float *r, unsigned *bp_, unsigned *sp, int Tb_)
        : R(p.R), WL(p.WL), flags(f), ring(r), bp(bp_), spill(sp), Tb(Tb_), ready(0) {}

    // rows < upto (<= Tb) are in the ring; false when the wait ran out
    __device__ __forceinline__ bool wait_rows(int upto)
    {
        for (int it = 0; ready < upto; ++it) {
            if (it >= kAlignSpinLimit) return false;
            if (it) __builtin_amdgcn_s_sleep(1);
            int x = 0x7fffffff;
#pragma unroll
            for (int i = 0; i < kAlignLoaders; ++i) x = min(x, align_load(flags + i) * kAlignLoaders + i);
            ready = x;
        }
        lds_order();
        return true;
    }

    __device__ __forceinline__ void read_group(AlignRow<K> (&buf)[G], int t0)
    {
#pragma unroll
        for (int j = 0; j < G; ++j) align_read_row<K>(ring, R, t0 + j, buf[j]);
        lds_order();
        align_store(flags + kSlotTaken, t0 + G);                 // (in order behind the reads)
    }

    __device__ __forceinline__ void store_word(int w, unsigned word)
    {
        if (w < WL) bp[w * kWave + lane_id()] = word;
        else spill[(w - WL) * kWave + lane_id()] = word;
    }

    template <bool GUARD>
    __device__ __forceinline__ void group(const AlignRow<K> (&buf)[G], int t0)
    {
        unsigned word = 0;
#pragma unroll
        for (int j = 0; j < G; ++j) {
            const int t = t0 + j;
            if (GUARD && t >= Tb) break;
            if (GUARD && t == 0) {
                const int s0 = lane_id() * K;
#pragma unroll
                for (int k = 0; k < K; ++k)
                    a[k] = s0 + k == 0 ? buf[j].eb : (s0 + k == 1 ? buf[j].el[0] : -__builtin_inff());
            } else {
                align_select_step<K>(a, skip, buf[j].el, buf[j].eb, -__builtin_inff(), j % P, word);
            }
            if (j % P == P - 1 || (GUARD && t == Tb - 1)) {
                store_word(t / P, word);
                word = 0;
            }
        }
    }

    __device__ __forceinline__ void run_group(const AlignRow<K> (&buf)[G], int t0)
    {
        if (t0 > 0 && t0 + G <= Tb) group<false>(buf, t0);
        else group<true>(buf, t0);
    }

    // false: a wait ran out
    __device__ __forceinline__ bool scan()
    {
        AlignRow<K> A[G], B[G];
        if (!wait_rows(min(G, Tb))) return false;
        read_group(A, 0);
        for (int t0 = 0;;) {
            bool more = t0 + G < Tb;
            if (more) {
                if (!wait_rows(min(t0 + 2 * G, Tb))) return false;
                read_group(B, t0 + G);
            }
            run_group(A, t0);
            t0 += G;
            if (!more) break;
            more = t0 + G < Tb;
            if (more) {
                if (!wait_rows(min(t0 + 2 * G, Tb))) return false;
                read_group(A, t0 + G);
            }
            run_group(B, t0);
            t0 += G;
            if (!more) break;
        }
        return true;
    }

    __device__ __forceinline__ void load_words(unsigned (&w)[kAlignWalkWords], int wtop)
    {
#pragma unroll
        for (int i = 0; i < kAlignWalkWords; ++i) {
            const int r = wtop - i;
            w[i] = r < 0 ? 0u : (r < WL ? bp[r * kWave + lane_id()] : spill[(r - WL) * kWave + lane_id()]);
        }
    }

    // from state `s` at step Tb-1 down to step 0; path[t] = s_t, stored 64 steps at a time
    __device__ __forceinline__ void walk(int s, int32_t *out)
    {
        const int lane = lane_id();
        unsigned cur[kAlignWalkWords], nxt[kAlignWalkWords];
        int outv = -1;
        const int wtop = (Tb - 1) / P;
        load_words(nxt, wtop);
        for (int w0 = wtop; w0 >= 0; w0 -= kAlignWalkWords) {
#pragma unroll
            for (int i = 0; i < kAlignWalkWords; ++i) cur[i] = nxt[i];
            if (w0 >= kAlignWalkWords) load_words(nxt, w0 - kAlignWalkWords);
#pragma unroll
            for (int i = 0; i < kAlignWalkWords; ++i) {
                const int word = (int)cur[i];
#pragma unroll
                for (int sub = P - 1; sub >= 0; --sub) {
                    const int t = (w0 - i) * P + sub;                 // (t < 0 only below the last block: nothing to do)
                    if (t >= 0 && t < Tb) {
                        outv = lane == (t & (kWave - 1)) ? s : outv;
                        if ((t & (kWave - 1)) == 0 && t + lane < Tb) out[t + lane] = outv;
                        const unsigned x = (unsigned)__builtin_amdgcn_readlane(word, s / K);
                        if (t >= 1) s -= (int)((x >> (2 * K * sub + 2 * (s & (K - 1)))) & 3u);
                    }
                }
            }
        }
    }
};

template <int K>
__global__ __launch_bounds__(kAlignThreads) void blank_align_kernel(AlignParams p)
{
    constexpr int RW = align_row_pitch(K);
    extern __shared__ __attribute__((aligned(16))) int align_smem[];
    int *flags = align_smem;                                      // [kAlignHead]
    float *ring = reinterpret_cast<float *>(align_smem + kAlignHead);   // [R][RW]
    unsigned *bp = reinterpret_cast<unsigned *>(ring + p.R * RW);       // [WL][64]
    const int b = blockIdx.x, tid = threadIdx.x, w = wave_id(), lane = lane_id();
    int32_t *out = p.path + (int64_t)b * p.T;
    int Tb, L;
    const bool ok = align_sample(p, b, Tb, L);
    if (!ok) {
        for (int t = tid; t < p.T; t += kAlignThreads) out[t] = -1;
        if (tid == 0) p.score[b] = -__builtin_inff();
        return;
    }
    if (tid < kAlignHead) flags[tid] = 0;
    __syncthreads();

    if (w > 0) {
        for (int t = Tb + tid - kWave; t < p.T; t += kAlignThreads - kWave) out[t] = -1;
        if (!align_loader<K>(p, flags, ring, b, Tb, w - 1)) {
            align_store(flags + kSlotAbort, 1);
            raise_status(p.counter, kStatusAlignStarved);
        }
        return;
    }

    __builtin_amdgcn_s_setprio(3);
    AlignScan<K> sc(p, flags, ring, bp, p.spill + (int64_t)b * p.NWS * kWave, Tb);
#pragma unroll
    for (int k = 0; k < K; ++k) sc.skip[k] = align_skip_flag<true>(p, b, L, lane * K + k, k);
    const bool done = sc.scan();
    if (!done) {                                                  // a wait ran out: NaN score, no path
        align_store(flags + kSlotAbort, 1);
        raise_status(p.counter, kStatusAlignStarved);
        for (int t = lane; t < Tb; t += kWave) out[t] = -1;
        if (lane == 0) p.score[b] = __builtin_nanf("");
        return;
    }
    int sfin = 0;
    if (L > 0) sfin = align_state_value<K>(sc.a, 2 * L) > align_state_value<K>(sc.a, 2 * L - 1) ? 2 * L : 2 * L - 1;
    const float score = align_state_value<K>(sc.a, sfin);
    if (lane == 0) p.score[b] = score;
    if (!(score > -__builtin_inff())) {                           // no alignment
        for (int t = lane; t < Tb; t += kWave) out[t] = -1;
        return;
    }
    __builtin_amdgcn_s_waitcnt(0);                                // the spilled words have landed before they are read back
    sc.walk(sfin, out);
}

template <int K>
static int run_blank_align(AlignParams &p, hipStream_t s)
{
    constexpr int RW = align_row_pitch(K), P = align_steps_per_word(K);
    p.RW = RW;
    p.R = K == 8 ? 32 : 64;
    const size_t head = kAlignHead * sizeof(int), ring = (size_t)p.R * RW * sizeof(float);
    const int nw = (p.T + P - 1) / P;
    const int cap = (int)((kMaxLds - head - ring) / (kWave * sizeof(unsigned)));
    p.WL = nw < cap ? nw : cap;
    p.NWS = nw - p.WL;
    char *ws = reinterpret_cast<char *>(p.counter) + 256;
    p.em = reinterpret_cast<float *>(ws);
    p.spill = reinterpret_cast<unsigned *>(ws + (size_t)p.B * p.T * RW * sizeof(float));
    const size_t need = 256 + (size_t)p.B * p.T * RW * sizeof(float) + (size_t)p.B * p.NWS * kWave * sizeof(unsigned);
    if (need > ctc_amd_workspace_bytes(CTC_AMD_BLANK, p.T, p.B, p.C, p.S)) return CTC_AMD_ERR_UNSUPPORTED_SHAPE;
    int rc = launch_blank_table_gather<32 * K, kAlignGatherRows, false>(p, s);
    if (rc) return rc;
    const size_t lds = head + ring + (size_t)p.WL * kWave * sizeof(unsigned);
    return launch<blank_align_kernel<K>>(dim3(p.B), dim3(kAlignThreads), lds, s, p);
}

// ==== per-frame state posteriors (ctc_amd_blank_posteriors) =======================================
// gamma_t(s) = exp(alpha_t(s) + beta'_t(s) + nll): the sum-semiring twin of the scan above, in three launches --
//   blank_table_gather_kernel     (as above) the compact emission table em [B][T][RW];
//   blank_post_chain_kernel<K>    one 128-thread workgroup per sample: wave 0 runs alpha forward, wave 1 beta' backward
//                                 (beta' leaves out the emission of its own step), K states per lane, neighbours
//                                 through DPP, emission rows loaded kPostAhead rows ahead into registers; each wave
//                                 stores its rows [B][T][NSP] to the workspace, wave 0 writes nll;
//   blank_post_gamma_kernel<K>    (bandwidth, every CU) gamma rows = softmax_s(alpha' + beta') in coalesced stores,
//                                 zeros outside the support.
// The chains are fp32 in log2 units but never hold absolute values: every kPostRescale steps a wave subtracts its
// row maximum (wave-uniform) from its states, so the values near the maximum -- the ones gamma is made of -- stay
// small and keep their fp32 resolution over any T (the loss's chains reach -2e4 at T = 2000, one ulp 2e-3).  Each
// emission row enters relative to its own maximum (c_t, over the blank and the labels, in natural log, before the
// conversion to log2): a per-frame constant that every path pays once, so it cancels from gamma too, and the
// roundings of the conversion and of the add scale with lp - c_t instead of lp (peaked inputs, lp ~ -250 at T = 150:
// max |dgamma| 3.6e-5 without it).  Each row is then normalised on its own, so the offsets cancel from gamma; only
// alpha's (the maxima and the c_t) are summed, in double, for nll.
// Unreachable states carry the finite stand-in kPostNeg (-inf inputs included) and come out of the row softmax as 0.
constexpr int kPostAhead = 16;                  // emission rows in flight ahead of a chain
constexpr int kPostRescale = 8;                 // chain steps between two subtractions of the row maximum
constexpr int kPostRows = 4;                    // gamma rows per wave of the combine launch (and emission rows per
                                                // wave_max4 of a chain)
constexpr int kPostThreads = 256;
constexpr float kPostNeg = -1.0e30f;            // unreachable (its sums stay finite: no inf - inf in a step)
constexpr float kPostLive = -1.0e29f;           // above: a reachable value

struct PostParams {
    AlignParams a;                              // inputs, shape, em (the gather's table)
    float *al, *be;                             // [B][T][NSP] rescaled alpha / beta' rows, log2 units
    float *nll, *gamma;
    int NSP, NS;                                // lattice row pitch 64 K, gamma row pitch 2S+1
};

__device__ __forceinline__ float post_lse2(float a, float b)
{
    return vmax(a, b) + __builtin_amdgcn_logf(1.0f + __builtin_amdgcn_exp2f(-fabsf(a - b)));
}

// one emission row in registers: el[j] = label lane*K/2 + j, eb = blank (loaded per lane from one address: a vector
// load, so that every fetch of the ring is counted by the same counter)
template <int K, bool FWD>
__device__ __forceinline__ void post_fetch(const float *em, int Tb, int i, int eoff, AlignRow<K> &r)
{
    constexpr int RW = align_row_pitch(K);
    const int ii = i < Tb ? i : Tb - 1;
    const float *row = em + (int64_t)(FWD ? ii : Tb - 1 - ii) * RW;
    const int lane = lane_id();
    if constexpr (K == 2) {
        r.el[0] = row[lane];
    } else if constexpr (K == 4) {
        const float2 x = reinterpret_cast<const float2 *>(row)[lane];
        r.el[0] = x.x; r.el[1] = x.y;
    } else {
        const float4 x = reinterpret_cast<const float4 *>(row)[lane];
        r.el[0] = x.x; r.el[1] = x.y; r.el[2] = x.z; r.el[3] = x.w;
    }
    r.eb = row[32 * K + eoff];
}

template <int K, bool FWD>
struct PostChain {
    float a[K];                                  // state values (log2, relative to the offsets subtracted so far)
    bool skip[K];
    double off;                                  // alpha: the state maxima subtracted so far (log2)
    double coff;                                 // alpha: the emission maxima c_t subtracted so far (natural log)

    // pre[] = log-sum-exp over the predecessors (alpha) / successors (beta) of each state; a label state's third term is
    // folded into the neighbouring blank's two-term sum (as in blank.hip), so every state is one two-term LSE.
    // in_a / in_q: what the wave's edge lane takes from beyond the wave (blank_post_wide.hpp) -- alpha: the state below
    // the wave's first; beta: the state above its last and that state's two-term sum
    __device__ __forceinline__ void pre(float (&q)[K], float in_a = kPostNeg, float in_q = kPostNeg) const
    {
        if (FWD) {
            const float nb1 = wave_shr1(a[K - 1], in_a);
#pragma unroll
            for (int k = 0; k < K; k += 2) q[k] = post_lse2(a[k], k ? a[k - 1] : nb1);
#pragma unroll
            for (int k = 1; k < K; k += 2) q[k] = post_lse2(a[k], skip[k] ? q[k - 1] : a[k - 1]);
        } else {
            const float n1 = wave_shl1(a[0], in_a);
#pragma unroll
            for (int k = 0; k < K; k += 2) q[k] = post_lse2(a[k], a[k + 1]);
            const float nb = wave_shl1(q[0], in_q);
#pragma unroll
            for (int k = 1; k < K; k += 2)
                q[k] = post_lse2(a[k], skip[k] ? (k + 1 < K ? q[k + 1] : nb) : (k + 1 < K ? a[k + 1] : n1));
        }
    }

    // a = pre + (emission - c); the row stored is alpha_t (FWD) or beta'_t = pre (!FWD)
    __device__ __forceinline__ void add_store(const float (&q)[K], const AlignRow<K> &e, float c, float *dst, bool st)
    {
        const float eb = vmax((e.eb - c) * kLog2e, kPostNeg);
#pragma unroll
        for (int k = 0; k < K; ++k) a[k] = q[k] + ((k & 1) ? vmax((e.el[k / 2] - c) * kLog2e, kPostNeg) : eb);
        if (FWD) coff += (double)c;
        if (!st) return;
        const float *v = FWD ? a : q;
        if constexpr (K == 2) {
            *reinterpret_cast<float2 *>(dst) = make_float2(v[0], v[1]);
        } else {
#pragma unroll
            for (int k = 0; k < K; k += 4) *reinterpret_cast<float4 *>(dst + k) = make_float4(v[k], v[k + 1], v[k + 2], v[k + 3]);
        }
    }

    // the maximum of the wave's states (wave-uniform)
    __device__ __forceinline__ float state_max() const
    {
        float mx = a[0];
#pragma unroll
        for (int k = 1; k < K; ++k) mx = vmax(mx, a[k]);
        return wave_max(mx);
    }

    // subtract m from every state; clamp what is not reachable at kPostNeg
    __device__ __forceinline__ void subtract(float m)
    {
#pragma unroll
        for (int k = 0; k < K; ++k) a[k] = vmax(a[k] - m, kPostNeg);
        if (FWD) off += (double)m;
    }

    // subtract the row maximum (when anything is reachable)
    __device__ __forceinline__ void rescale()
    {
        const float m = state_max();
        subtract(m > kPostLive ? m : 0.f);
    }

    __device__ __forceinline__ void step(const AlignRow<K> &e, float c, float *dst, bool st)
    {
        float q[K];
        pre(q);
        add_store(q, e, c, dst, st);
    }
};

// the emission maxima c_t of four rows (0 for a row without a finite emission: everything on it stays unreachable)
template <int K>
__device__ __forceinline__ void post_row_max4(const AlignRow<K> *r, float (&c)[kPostRows])
{
#pragma unroll
    for (int i = 0; i < kPostRows; ++i) {
        c[i] = r[i].eb;
#pragma unroll
        for (int j = 0; j < K / 2; ++j) c[i] = fmaxf(c[i], r[i].el[j]);
    }
    wave_max4(c[0], c[1], c[2], c[3]);
#pragma unroll
    for (int i = 0; i < kPostRows; ++i) c[i] = c[i] > -__builtin_inff() ? c[i] : 0.f;
}

template <int K, bool FWD>
__device__ __forceinline__ void post_chain(const PostParams &p, int b, int Tb, int L)
{
    constexpr int RW = align_row_pitch(K), D = kPostAhead, G = kPostRescale;
    static_assert(D % G == 0 && D % kPostRows == 0, "rescale / row-maximum points are compile-time positions in the unrolled body");
    const int lane = lane_id(), s0 = lane * K, n = 2 * L + 1;
    const int T = p.a.T;
    const float *em = p.a.em + (int64_t)b * T * RW;
    float *out = (FWD ? p.al : p.be) + (int64_t)b * T * p.NSP + s0;
    const int64_t dir = FWD ? p.NSP : -(int64_t)p.NSP;
    const bool st = s0 < n;                                       // lanes wholly beyond the lattice store nothing
    const int eoff = opaque_v(0);
    PostChain<K, FWD> c;
    c.off = 0.0;
    c.coff = 0.0;
#pragma unroll
    for (int k = 0; k < K; ++k) c.skip[k] = align_skip_flag<FWD>(p.a, b, L, s0 + k, k);
    float *dst = out + (int64_t)(FWD ? 0 : Tb - 1) * p.NSP;
    {
        AlignRow<K> e0[kPostRows];
        post_fetch<K, FWD>(em, Tb, 0, eoff, e0[0]);
        e0[1] = e0[2] = e0[3] = e0[0];
        float c0[kPostRows];
        post_row_max4<K>(e0, c0);
        float q[K];
        const int sa = FWD ? 0 : 2 * L, sb = FWD ? 1 : 2 * L - 1;       // entry states
#pragma unroll
        for (int k = 0; k < K; ++k) q[k] = (s0 + k == sa || s0 + k == sb) ? 0.f : kPostNeg;
        c.add_store(q, e0[0], c0[0], dst, st);
        dst += dir;
    }
    AlignRow<K> ring[D];
    float cm[kPostRows];
#pragma unroll
    for (int j = 0; j < D; ++j) post_fetch<K, FWD>(em, Tb, 1 + j, eoff, ring[j]);
    int i = 1;
    for (; i + D <= Tb; i += D) {
#pragma unroll
        for (int j = 0; j < D; ++j) {
            if (j % kPostRows == 0) post_row_max4<K>(ring + j, cm);
            const AlignRow<K> e = ring[j];
            post_fetch<K, FWD>(em, Tb, i + j + D, eoff, ring[j]);
            c.step(e, cm[j % kPostRows], dst, st);
            dst += dir;
            if (j % G == G - 1) c.rescale();
        }
    }
#pragma unroll
    for (int j = 0; j < D; ++j)
        if (i + j < Tb) {
            if (j % kPostRows == 0) post_row_max4<K>(ring + j, cm);
            c.step(ring[j], cm[j % kPostRows], dst, st);
            dst += dir;
            if (j % G == G - 1) c.rescale();
        }
    if (FWD) {
        const float x = align_state_value<K>(c.a, 2 * L);
        const float y = L > 0 ? align_state_value<K>(c.a, 2 * L - 1) : kPostNeg;
        const float v = post_lse2(x, y);
        if (lane == 0)
            p.nll[b] = v > kPostLive ? (float)(-((double)v + c.off) * (double)kLn2 - c.coff) : __builtin_inff();
    }
}

template <int K>
__global__ __launch_bounds__(2 * kWave) void blank_post_chain_kernel(PostParams p)
{
    const int b = blockIdx.x;
    int Tb, L;
    if (!align_sample(p.a, b, Tb, L)) {                          // lengths outside the tensor: no alignment (+inf, gamma rows 0),
        if (threadIdx.x == 0) p.nll[b] = __builtin_inff();       // as ctc_amd_blank_loss_grad reports such a sample
        return;
    }
    if (wave_id() == 0) post_chain<K, true>(p, b, Tb, L);
    else post_chain<K, false>(p, b, Tb, L);
}

// The row arithmetic of the combine launches (blank_post_gamma_kernel below, blank_post_conf_kernel in blank_spans.hpp):
// rows t0 .. t0 + kPostRows - 1 of a sample, state s = lane + 64 k.  In: z[r][k] = alpha' + beta' (-inf outside the
// support) and m[r] = the lane's maximum over its k.  Out: m[r] = the row maximum, z[r][k] = exp2(z - m) (0 outside the
// support), sum[r] = the row sum, both in every lane.  gamma = z * post_row_inv(sum).
// (The masked loads in front stay in each kernel's body: moved into a routine they reorder the instructions of all twelve
// combine kernels, and the one run that had them so did not show the wide posteriors as fast as before at W = 3;
// profiles/r24_blank_readouts_refactor.md.)
template <int K>
__device__ __forceinline__ void post_row_terms(float (&z)[kPostRows][K], float (&m)[kPostRows], float (&sum)[kPostRows])
{
    wave_max4(m[0], m[1], m[2], m[3]);
#pragma unroll
    for (int r = 0; r < kPostRows; ++r) {
        sum[r] = 0.f;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            z[r][k] = z[r][k] > -__builtin_inff() ? __builtin_amdgcn_exp2f(z[r][k] - m[r]) : 0.f;
            sum[r] += z[r][k];
        }
    }
    wave_sum4(sum[0], sum[1], sum[2], sum[3]);
}

__device__ __forceinline__ float post_row_inv(float sum) { return sum > 0.f ? 1.0f / sum : 0.f; }

// grid (ceil(T / (4 * kPostRows)), B): wave w of block x takes rows t0 .. t0 + kPostRows - 1, state s = lane + 64 k
template <int K>
__global__ __launch_bounds__(kPostThreads) void blank_post_gamma_kernel(PostParams p)
{
    const int b = blockIdx.y, lane = lane_id(), T = p.a.T;
    const int t0 = (blockIdx.x * (kPostThreads / kWave) + wave_id()) * kPostRows;
    if (t0 >= T) return;
    int Tb, L;
    const bool ok = align_sample(p.a, b, Tb, L);
    const bool feasible = ok && p.nll[b] < __builtin_inff();     // (+inf: no alignment, bad lengths included)
    const int n = 2 * L + 1;
    const int64_t r0 = (int64_t)b * T + t0;
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
    float *out = p.gamma + r0 * p.NS;
#pragma unroll
    for (int r = 0; r < kPostRows; ++r) {
        if (t0 + r >= T) break;
        const float inv = post_row_inv(sum[r]);
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int s = lane + kWave * k;
            if (s < p.NS) stream_store(out + r * p.NS + s, z[r][k] * inv);
        }
    }
}

// where the posteriors' rows lie: the gather's table em, then alpha', then beta' (ctc_amd_blank_token_spans lays its
// posterior stage out with this too)
template <int K>
static int blank_post_layout(PostParams &pp)
{
    constexpr int RW = align_row_pitch(K);
    AlignParams &p = pp.a;
    p.RW = RW;
    pp.NSP = kWave * K;
    pp.NS = 2 * p.S + 1;
    const size_t cells = (size_t)p.B * p.T;
    char *ws = reinterpret_cast<char *>(p.counter) + 256;
    p.em = reinterpret_cast<float *>(ws);
    pp.al = p.em + cells * RW;
    pp.be = pp.al + cells * pp.NSP;
    // the three lattice areas of the blank loss ([B][T][NSP] each, NSP = 64 K) hold em + al + be; nothing behind them
    if ((size_t)RW + 2 * (size_t)pp.NSP > 3 * (size_t)pp.NSP) return CTC_AMD_ERR_UNSUPPORTED_SHAPE;
    return 0;
}

template <int K>
static int run_blank_post(PostParams &pp, hipStream_t s)
{
    int rc = blank_post_layout<K>(pp);
    if (rc) return rc;
    AlignParams &p = pp.a;
    rc = launch_blank_table_gather<32 * K, kAlignGatherRows, false>(p, s);
    if (rc) return rc;
    rc = launch<blank_post_chain_kernel<K>>(dim3(p.B), dim3(2 * kWave), 0, s, pp);
    if (rc) return rc;
    const int rows = (kPostThreads / kWave) * kPostRows;
    return launch<blank_post_gamma_kernel<K>>(dim3((p.T + rows - 1) / rows, p.B), dim3(kPostThreads), 0, s, pp);
}

}  // namespace ctc

#include "blank_align_wide.hpp"
#include "blank_post_wide.hpp"
#include "blank_spans.hpp"

using namespace ctc;

// What the five entries have in common: the null and range checks, and the inputs and the shape into `p`.
// `outputs`: the entry's own output pointers are all non-null.
static int blank_readout_params(AlignParams &p, const float *log_probs, int64_t stride_t, int64_t stride_b,
                                const void *targets, int targets_i64, const int64_t *in_len, const int64_t *tgt_len,
                                int T, int B, int C, int S, int blank, bool outputs, void *workspace)
{
    if (!log_probs || !targets || !in_len || !tgt_len || !outputs || !workspace) return CTC_AMD_ERR_BAD_ARGUMENT;
    if (T < 1 || B < 1 || C < 1 || S < 1 || blank < 0 || blank >= C) return CTC_AMD_ERR_BAD_ARGUMENT;
    p.lp = log_probs; p.st = stride_t; p.sb = stride_b;
    p.tgt = targets; p.tgt64 = targets_i64;
    p.in_len = in_len; p.tgt_len = tgt_len;
    p.T = T; p.B = B; p.C = C; p.S = S; p.blank = blank;
    p.counter = static_cast<unsigned *>(workspace);
    return 0;
}

// states per lane of the narrow kernels (S <= 255): 2S+1 <= 128 / 256 / 512
static int align_states_per_lane(int S) { return 2 * S + 1 <= kWave * 2 ? 2 : (2 * S + 1 <= kWave * 4 ? 4 : 8); }

extern "C" int ctc_amd_blank_best_path_wide(const float *log_probs, int64_t stride_t, int64_t stride_b,
                                            const void *targets, int targets_i64,
                                            const int64_t *in_len, const int64_t *tgt_len,
                                            int T, int B, int C, int S, int blank,
                                            int32_t *path, float *score, void *workspace, void *stream)
{
    AlignParams p;
    const int rc = blank_readout_params(p, log_probs, stride_t, stride_b, targets, targets_i64, in_len, tgt_len, T, B, C, S,
                                        blank, path && score, workspace);
    if (rc) return rc;
    if (S < 256 || S > 1023) return CTC_AMD_ERR_UNSUPPORTED_SHAPE;           // 513 <= 2S+1 <= 2047: two to four waves of 512
    p.path = path; p.score = score;
    return run_blank_align_wide(p, static_cast<hipStream_t>(stream));
}

extern "C" int ctc_amd_blank_best_path(const float *log_probs, int64_t stride_t, int64_t stride_b,
                                       const void *targets, int targets_i64,
                                       const int64_t *in_len, const int64_t *tgt_len,
                                       int T, int B, int C, int S, int blank,
                                       int32_t *path, float *score, void *workspace, void *stream)
{
    AlignParams p;
    const int rc = blank_readout_params(p, log_probs, stride_t, stride_b, targets, targets_i64, in_len, tgt_len, T, B, C, S,
                                        blank, path && score, workspace);
    if (rc) return rc;
    if (S > 255) return CTC_AMD_ERR_UNSUPPORTED_SHAPE;                        // 2S+1 <= 512: one wave
    p.path = path; p.score = score;
    return with_constant<2, 4, 8>(align_states_per_lane(S), [&](auto k) {
        return run_blank_align<decltype(k)::value>(p, static_cast<hipStream_t>(stream));
    });
}

extern "C" int ctc_amd_blank_posteriors(const float *log_probs, int64_t stride_t, int64_t stride_b,
                                        const void *targets, int targets_i64,
                                        const int64_t *in_len, const int64_t *tgt_len,
                                        int T, int B, int C, int S, int blank,
                                        float *nll, float *gamma, void *workspace, void *stream)
{
    PostParams pp = {};
    const int rc = blank_readout_params(pp.a, log_probs, stride_t, stride_b, targets, targets_i64, in_len, tgt_len, T, B, C,
                                        S, blank, nll && gamma, workspace);
    if (rc) return rc;
    if (S > 255) return CTC_AMD_ERR_UNSUPPORTED_SHAPE;                        // 2S+1 <= 512: one wave
    pp.nll = nll; pp.gamma = gamma;
    return with_constant<2, 4, 8>(align_states_per_lane(S), [&](auto k) {
        return run_blank_post<decltype(k)::value>(pp, static_cast<hipStream_t>(stream));
    });
}

extern "C" int ctc_amd_blank_posteriors_wide(const float *log_probs, int64_t stride_t, int64_t stride_b,
                                             const void *targets, int targets_i64,
                                             const int64_t *in_len, const int64_t *tgt_len,
                                             int T, int B, int C, int S, int blank,
                                             float *nll, float *gamma, void *workspace, void *stream)
{
    PostParams pp = {};
    const int rc = blank_readout_params(pp.a, log_probs, stride_t, stride_b, targets, targets_i64, in_len, tgt_len, T, B, C,
                                        S, blank, nll && gamma, workspace);
    if (rc) return rc;
    if (S < 256 || S > 1023) return CTC_AMD_ERR_UNSUPPORTED_SHAPE;           // 513 <= 2S+1 <= 2047: two to four waves of 512
    pp.nll = nll; pp.gamma = gamma;
    return run_blank_post_wide(pp, static_cast<hipStream_t>(stream));
}

extern "C" int ctc_amd_blank_token_spans(const float *log_probs, int64_t stride_t, int64_t stride_b,
                                         const void *targets, int targets_i64,
                                         const int64_t *in_len, const int64_t *tgt_len,
                                         int T, int B, int C, int S, int blank,
                                         int32_t *path, float *score, float *nll, float *frame_conf,
                                         int32_t *start, int32_t *end, float *conf,
                                         void *workspace, void *stream)
{
    SpanParams q = {};
    const int rc = blank_readout_params(q.p.a, log_probs, stride_t, stride_b, targets, targets_i64, in_len, tgt_len, T, B, C,
                                        S, blank, path && score && nll && frame_conf && start && end && conf, workspace);
    if (rc) return rc;
    if (S > 1023) return CTC_AMD_ERR_UNSUPPORTED_SHAPE;                       // 2S+1 <= 2047: four waves of 512
    q.p.a.path = path; q.p.a.score = score;
    q.p.nll = nll;
    q.frame_conf = frame_conf; q.start = start; q.end = end; q.conf = conf;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (S > 255) return run_blank_spans_wide(q, s);
    return with_constant<2, 4, 8>(align_states_per_lane(S), [&](auto k) { return run_blank_spans<decltype(k)::value>(q, s); });
}
