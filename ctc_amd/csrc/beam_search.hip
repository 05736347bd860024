// CTC prefix beam search on the device, gfx950: the most probable label sequences of a sample when no
// transcript is given, on the blank lattice (x holds log-probabilities) and on the no-blank lattice (blank < 0: x holds raw
// logits, the kernel subtracts each row's log-sum-exp).  One launch, one 256-thread workgroup per sample, which steps
// through the sample's frames with __syncthreads() alone: no flags, no polling, no atomics, nothing between workgroups;
// every loop has a bound known at entry (T_b, C, W, K).  It allocates nothing and never synchronises the host: safe under
// stream capture, deterministic.  Every global store is a plain C++ store.
//
// State (LDS, two copies that swap per frame): per beam pb, pnb (log probability of the prefix ending in blank / in a
// label), last (its last token, -1: the empty prefix), node (its identity), par (the identity of its parent prefix) and
// len.  The trie of prefixes -- (parent, token) per node, node 0 the empty prefix, node 1 + t W + slot the extension kept
// in slot `slot` at frame t -- lives in the caller's scratch and is read once, at the end, to write the tokens out.
//
// A frame, four barriers:
//   row      every wave takes a quarter of the row (1024 classes per pass: four per lane, the first pass from registers
//            that were loaded while the frame before was being selected) as 64-bit keys (value, ~class) and extracts its K
//            largest by K wave reductions; the no-blank lattice also keeps a running (max, sum exp) per wave.      barrier
//            The 4 K keys are ranked by counting (each of 4 K threads counts the keys above its own): the K class
//            candidates in the order of the rule -- raw value descending, ties to the lower class.               barrier
//   cands    thread i < W: the stay candidate of beam i, with the one extension that IS beam i's prefix (from its parent
//            beam, by its last token) added in; the other threads: the extensions (beam, class rank), those that are a
//            beam's prefix left out (a W-long comparison of (par, last) each).  Each candidate is a 64-bit key
//            (score, stay before extension, slot, rank) whose unsigned order is the total order of the rule.
//   select   every wave extracts the W largest of its keys (W wave reductions, no barrier);                       barrier
//            the 4 W keys are ranked by counting; the key of rank r < W becomes beam r of the next frame.          barrier
// After the last frame the beams are in final order (the selection key of a frame is the final score of its prefix).
//
// beam_search_kernel<true> is the same search under a bigram table: every beam carries g, the sum of its
// tokens' increments lm_weight lm[previous or C][c] + token_bonus, which enters the selection keys; an extension thread
// gathers its table entry first thing behind the barrier that publishes the class list.  beam_search_kernel<false> is the
// plain search: no instruction of it knows of the table.
#include <limits.h>

#include "common.hpp"
#include "launch.hpp"

namespace ctc {

constexpr int kBeamThreads = 256;
constexpr int kBeamWaves = kBeamThreads / kWave;
constexpr int kBeamMaxW = 64, kBeamMaxK = 32;
constexpr int kRowRegs = 4;                                     // classes per lane and pass over the row
constexpr int kRowPass = kBeamThreads * kRowRegs;
constexpr int kCandRegs = (kBeamMaxW + kBeamMaxW * kBeamMaxK + kBeamThreads - 1) / kBeamThreads;    // 9 keys per lane
constexpr int kExtBit = 1 << 11;                                // tie-break word: extension | slot << 5 | rank
constexpr unsigned kTieMask = 0xfffu;

typedef unsigned long long key_t;

struct BeamParams {
    const float *x;                             // [T][B][C] through (st, sb), unit class stride
    int64_t st, sb;
    const int64_t *in_len;
    int T, B, C, blank, W, K, N, L;
    int32_t *tokens;                            // [B][N][L]
    int64_t *lengths;                           // [B][N]
    float *scores;                              // [B][N]
    int32_t *count;                             // [B]
    int2 *trie;                                 // [B][T W + 1] (parent, token)
};

// the fused search: a bigram table beside the acoustic search.  The plain kernel's arguments come first
// and unchanged, so the LM = false instantiation is the kernel it was.
struct BeamLmParams : BeamParams {
    const float *lm;                            // [C + 1][C] through lm_stride, unit column stride; row C: the first token
    int64_t lm_stride;
    float lm_weight, token_bonus;
    float *ctc_scores;                          // [B][N]
};
template <bool LM> struct BeamArgs { typedef BeamParams type; };
template <> struct BeamArgs<true> { typedef BeamLmParams type; };

// fp32 -> 32 bits whose unsigned order is the order of the values (-inf lowest; -0 has become +0 before)
__device__ __forceinline__ unsigned ordered_bits(float f)
{
    const unsigned u = __builtin_bit_cast(unsigned, f);
    return u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);
}
__device__ __forceinline__ float ordered_value(unsigned o)
{
    return __builtin_bit_cast(float, o ^ ((o >> 31) ? 0x80000000u : 0xffffffffu));
}
// (value, tie word): a larger key is a better candidate -- larger value, then the SMALLER tie word.  Never 0 for a value
// above -inf; key 0 is "no candidate".
__device__ __forceinline__ key_t make_key(float v, unsigned tie_inverted)
{
    if (v == 0.0f) v = 0.0f;                                    // -0 and +0 tie
    return ((key_t)ordered_bits(v) << 32) | tie_inverted;
}

__device__ __forceinline__ key_t max_key(key_t a, key_t b) { return a > b ? a : b; }

template <int CTRL, int ROW_MASK>
__device__ __forceinline__ key_t dpp_key(key_t v)              // lanes without a source get key 0, the identity of max
{
    const unsigned lo = __builtin_amdgcn_update_dpp(0u, (unsigned)v, CTRL, ROW_MASK, 0xf, false);
    const unsigned hi = __builtin_amdgcn_update_dpp(0u, (unsigned)(v >> 32), CTRL, ROW_MASK, 0xf, false);
    return ((key_t)hi << 32) | lo;
}
// the largest key of the wave, in every lane (wave-uniform): the steps of wave_max (common.hpp) on 64 bits
__device__ __forceinline__ key_t wave_max_key(key_t v)
{
    v = max_key(v, dpp_key<kQuadXor1, 0xf>(v));
    v = max_key(v, dpp_key<kQuadXor2, 0xf>(v));
    v = max_key(v, dpp_key<kRowHalfMirror, 0xf>(v));
    v = max_key(v, dpp_key<kRowMirror, 0xf>(v));
    v = max_key(v, dpp_key<kRowBcast15, 0xa>(v));
    v = max_key(v, dpp_key<kRowBcast31, 0xc>(v));
    const unsigned lo = __builtin_amdgcn_readlane((unsigned)v, 63), hi = __builtin_amdgcn_readlane((unsigned)(v >> 32), 63);
    return ((key_t)hi << 32) | lo;
}

// The n largest of the wave's keys (R per lane, the first `used` of them live; unique except for zeros), largest first,
// into out[0 .. n) (LDS, this wave's own); zeros where the wave has fewer.  The keys are consumed.
template <int R>
__device__ __forceinline__ void wave_extract(key_t (&k)[R], int used, int n, key_t *out)
{
    for (int r = 0; r < n; ++r) {
        key_t m = 0;
#pragma unroll
        for (int q = 0; q < R; ++q)
            if (q < used) m = max_key(m, k[q]);
        m = wave_max_key(m);
        if (lane_id() == 0) out[r] = m;
#pragma unroll
        for (int q = 0; q < R; ++q)
            if (q < used && k[q] == m) k[q] = 0;
    }
}

// list[0 .. M) (LDS; unique except for zeros): the number of keys above list[tid] (tid < M), and the number of non-zero
// keys.  Every thread runs the whole loop, so `nz` is the same everywhere.
__device__ __forceinline__ void rank_by_counting(const key_t *list, int M, int tid, key_t &mine, int &rank, int &nz)
{
    mine = tid < M ? list[tid] : 0;
    rank = 0;
    nz = 0;
    for (int i = 0; i < M; ++i) {
        const key_t k = list[i];
        nz += k != 0;
        rank += k > mine;
    }
}

// logaddexp: m + log1p(exp(-|a - b|)) with the log argument in [1, 2] (lse2, common.hpp); -inf where both are
__device__ __forceinline__ float beam_lae(float a, float b)
{
    const float ninf = -__builtin_inff();
    if (fmaxf(a, b) == ninf) return ninf;
    return lse2(a, b);
}

__device__ __forceinline__ void load_row_pass(float (&v)[kRowRegs], const float *row, int c0, int C, int tid)
{
#pragma unroll
    for (int q = 0; q < kRowRegs; ++q) {
        const int c = c0 + q * kBeamThreads + tid;
        v[q] = c < C ? row[c] : -__builtin_inff();
    }
}

// LM: every beam carries g, the sum of lm_weight lm[last or C][c] + token_bonus over its tokens, beside (pb, pnb).  A
// candidate's selection key is its acoustic score + g; an extension whose table entry is -inf is no candidate; an extension
// merged into the beam that is its prefix adds its acoustic value alone (that beam's g was formed from the same numbers).
template <bool LM>
__global__ __launch_bounds__(kBeamThreads) void beam_search_kernel(typename BeamArgs<LM>::type p)
{
    __shared__ key_t s_list[kBeamWaves * kBeamMaxW];            // the waves' extracted keys: 4 K of the row, 4 W candidates
    __shared__ float s_pb[2][kBeamMaxW], s_pnb[2][kBeamMaxW];
    __shared__ int s_last[2][kBeamMaxW], s_node[2][kBeamMaxW], s_par[2][kBeamMaxW], s_len[2][kBeamMaxW];
    __shared__ float s_tot[kBeamMaxW], s_spb[kBeamMaxW], s_spnb[kBeamMaxW];
    __shared__ float s_ext[kBeamMaxW * kBeamMaxK];              // value of extension (beam, rank) at [beam K + rank]
    __shared__ int s_cls[kBeamMaxK];
    __shared__ float s_clp[kBeamMaxK];
    __shared__ float s_red[2 * kBeamWaves];                     // no-blank lattice: the waves' (max, sum exp)
    __shared__ float s_g[2][LM ? kBeamMaxW : 1];                // LM: the beams' g
    __shared__ float s_extg[LM ? kBeamMaxW * kBeamMaxK : 1];    // LM: g of extension (beam, rank), beside s_ext

    const float ninf = -__builtin_inff();
    const int b = blockIdx.x, tid = threadIdx.x, lane = lane_id(), wave = wave_id();
    const int W = p.W, K = p.K, C = p.C, blank = p.blank;
    const int64_t Tb64 = p.in_len[b];
    const int Tb = Tb64 < 0 ? 0 : (Tb64 > p.T ? p.T : (int)Tb64);       // (memory safety: never beyond the tensor)
    const float *xb = p.x + (int64_t)b * p.sb;
    const int64_t nodes = (int64_t)p.T * W + 1;
    int2 *trie = p.trie + (int64_t)b * nodes;
    const int ncand = W + W * K, cand_regs = (ncand + kBeamThreads - 1) / kBeamThreads;
    const int passes = (C + kRowPass - 1) / kRowPass;

    int cur = 0, nbeam = 1;
    if (tid == 0) {
        s_pb[0][0] = 0.0f; s_pnb[0][0] = ninf;
        s_last[0][0] = -1; s_node[0][0] = 0; s_par[0][0] = -1; s_len[0][0] = 0;
        if constexpr (LM) s_g[0][0] = 0.0f;
    }
    float ahead[kRowRegs] = {ninf, ninf, ninf, ninf};           // the first pass of the next frame's row
    if (Tb > 0) load_row_pass(ahead, xb, 0, C, tid);
    __syncthreads();

    for (int t = 0; t < Tb; ++t) {
        const float *row = xb + (int64_t)t * p.st;
        // what the stay candidates need of the row, asked for before anything waits
        float x_last = ninf, x_blank = ninf;
        int my_last = -1;
        if (tid < nbeam) {
            my_last = s_last[cur][tid];
            if (my_last >= 0) x_last = row[my_last];
            s_tot[tid] = beam_lae(s_pb[cur][tid], s_pnb[cur][tid]);
        }
        if (blank >= 0) x_blank = row[blank];

        // ---- row: this wave's K largest classes; the no-blank lattice's log-sum-exp
        key_t *mine_out = s_list + wave * K;
        float wmax = ninf, wsum = 0.0f;
        for (int ps = 0; ps < passes; ++ps) {
            float v[kRowRegs];
            if (ps == 0) {
#pragma unroll
                for (int q = 0; q < kRowRegs; ++q) v[q] = ahead[q];
            } else {
                load_row_pass(v, row, ps * kRowPass, C, tid);
            }
            key_t rk[kRowRegs + 1];
#pragma unroll
            for (int q = 0; q < kRowRegs; ++q) {
                const int c = ps * kRowPass + q * kBeamThreads + tid;           // (v is -inf at c >= C)
                rk[q] = (c != blank && v[q] > ninf) ? make_key(v[q], ~(unsigned)c) : 0;
            }
            lds_order();
            rk[kRowRegs] = (ps > 0 && lane < K) ? mine_out[lane] : 0;           // the best of the passes before
            lds_order();
            if (blank < 0) {
                float m = fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3]));
                m = fmaxf(wave_max(m), wmax);
                if (m > ninf) {
                    float s = 0.0f;
#pragma unroll
                    for (int q = 0; q < kRowRegs; ++q) s += fast_exp(v[q] - m);
                    wsum = wsum * fast_exp(wmax - m) + wave_sum(s);
                    wmax = m;
                }
            }
            wave_extract<kRowRegs + 1>(rk, kRowRegs + 1, K, mine_out);
        }
        if (blank < 0 && lane == 0) {
            s_red[wave] = wmax;
            s_red[kBeamWaves + wave] = wsum;
        }
        if (t + 1 < Tb) load_row_pass(ahead, row + p.st, 0, C, tid);           // in flight across the selection
        __syncthreads();

        key_t mine;
        int rank, nz;
        rank_by_counting(s_list, kBeamWaves * K, tid, mine, rank, nz);
        const int ncls = min(nz, K);
        float lse = 0.0f;
        if (blank < 0) {
            float m = s_red[0];
#pragma unroll
            for (int w = 1; w < kBeamWaves; ++w) m = fmaxf(m, s_red[w]);
            float s = 0.0f;
#pragma unroll
            for (int w = 0; w < kBeamWaves; ++w) s += s_red[kBeamWaves + w] * fast_exp(s_red[w] - m);
            lse = m + fast_log(s);
        }
        if (mine != 0 && rank < K) {
            const float xv = ordered_value((unsigned)(mine >> 32));
            s_cls[rank] = (int)~(unsigned)mine;
            s_clp[rank] = blank < 0 ? xv - lse : xv;
        }
        __syncthreads();

        // ---- candidates
        key_t ck[kCandRegs];
#pragma unroll
        for (int q = 0; q < kCandRegs; ++q) {
            ck[q] = 0;
            if (q >= cand_regs) continue;
            const int idx = q * kBeamThreads + tid;
            if (idx < W) {                                                      // (q == 0, idx == tid)
                if (idx < nbeam) {
                    const int i = idx;
                    const float spb = blank >= 0 ? s_tot[i] + x_blank : ninf;
                    float spnb = my_last >= 0 ? s_pnb[cur][i] + (blank < 0 ? x_last - lse : x_last) : ninf;
                    const int par = s_par[cur][i];
                    if (par >= 0) {                                             // the extension that is this prefix
                        int pj = -1, rr = -1;
                        for (int j = 0; j < nbeam; ++j)
                            if (s_node[cur][j] == par) pj = j;
                        for (int r = 0; r < ncls; ++r)
                            if (s_cls[r] == my_last) rr = r;
                        if (pj >= 0 && rr >= 0) {
                            const float v = s_clp[rr] + (my_last == s_last[cur][pj] ? s_pb[cur][pj] : s_tot[pj]);
                            spnb = beam_lae(spnb, v);
                        }
                    }
                    s_spb[i] = spb;
                    s_spnb[i] = spnb;
                    float score = beam_lae(spb, spnb);
                    if constexpr (LM) score += s_g[cur][i];
                    if (score > ninf) ck[q] = make_key(score, kTieMask - (unsigned)(i << 5));
                }
            } else if (idx < ncand) {
                const int e = idx - W, i = e / K, r = e - i * K;
                if (i < nbeam && r < ncls) {
                    const int c = s_cls[r], node = s_node[cur][i];
                    // LM: the table entry of this extension, asked for as soon as the class list stands -- one dependent
                    // gather from L2, in flight across the W-long comparison below.  Row: the beam's own last token or C;
                    // column: a class of the kernel's list (never the blank; never the diagonal on the no-blank lattice).
                    float entry = ninf;
                    if constexpr (LM) {
                        const int last = s_last[cur][i];
                        if (blank >= 0 || c != last) entry = p.lm[(int64_t)(last < 0 ? C : last) * p.lm_stride + c];
                    }
                    const float v = s_clp[r] + (c == s_last[cur][i] ? s_pb[cur][i] : s_tot[i]);
                    bool is_beam = false;
                    for (int j = 0; j < nbeam; ++j) is_beam |= s_par[cur][j] == node && s_last[cur][j] == c;
                    s_ext[e] = v;
                    if constexpr (LM) {
                        const float g = s_g[cur][i] + (p.lm_weight * entry + p.token_bonus);
                        s_extg[e] = g;
                        if (!is_beam && entry > ninf && v + g > ninf)
                            ck[q] = make_key(v + g, kTieMask - (unsigned)(kExtBit | (i << 5) | r));
                    } else {
                        if (!is_beam && v > ninf) ck[q] = make_key(v, kTieMask - (unsigned)(kExtBit | (i << 5) | r));
                    }
                }
            }
        }

        // ---- selection
        wave_extract<kCandRegs>(ck, cand_regs, W, s_list + wave * W);
        __syncthreads();
        rank_by_counting(s_list, kBeamWaves * W, tid, mine, rank, nz);
        if (mine != 0 && rank < W) {
            const unsigned tie = kTieMask - ((unsigned)mine & kTieMask);
            const int i = (tie >> 5) & (kBeamMaxW - 1), r = tie & (kBeamMaxK - 1), nx = cur ^ 1;
            if (tie & kExtBit) {
                const int node = 1 + t * W + rank, c = s_cls[r];
                s_pb[nx][rank] = ninf;
                s_pnb[nx][rank] = s_ext[i * K + r];
                s_last[nx][rank] = c;
                s_node[nx][rank] = node;
                s_par[nx][rank] = s_node[cur][i];
                s_len[nx][rank] = s_len[cur][i] + 1;
                if constexpr (LM) s_g[nx][rank] = s_extg[i * K + r];
                trie[node] = make_int2(s_node[cur][i], c);
            } else {
                s_pb[nx][rank] = s_spb[i];
                s_pnb[nx][rank] = s_spnb[i];
                s_last[nx][rank] = s_last[cur][i];
                s_node[nx][rank] = s_node[cur][i];
                s_par[nx][rank] = s_par[cur][i];
                s_len[nx][rank] = s_len[cur][i];
                if constexpr (LM) s_g[nx][rank] = s_g[cur][i];
            }
        }
        nbeam = min(nz, W);
        cur ^= 1;
        __syncthreads();
    }

    // ---- write-out: the beams are in final order.  Thread n walks hypothesis n's prefix backwards through the trie
    // (tokens at positions < min(len, L)); all threads together write the -1 of every other position.
    const int N = p.N, L = p.L, cnt = min(nbeam, N);
    if (tid == 0) p.count[b] = cnt;
    if (tid < N) {
        const int64_t o = (int64_t)b * N + tid;
        const bool have = tid < cnt;
        const int len = have ? s_len[cur][tid] : 0;
        p.lengths[o] = len;
        const float acoustic = have ? beam_lae(s_pb[cur][tid], s_pnb[cur][tid]) : ninf;
        if constexpr (LM) {
            p.scores[o] = have ? acoustic + s_g[cur][tid] : ninf;
            p.ctc_scores[o] = acoustic;
        } else {
            p.scores[o] = acoustic;
        }
        int node = have ? s_node[cur][tid] : 0;
        for (int pos = len - 1; pos >= 0; --pos) {                              // len <= T_b
            if (node <= 0 || node >= nodes) break;                              // (memory safety; never taken)
            const int2 e = trie[node];
            if (pos < L) p.tokens[o * L + pos] = e.y;
            node = e.x;
        }
    }
    for (int idx = tid; idx < N * L; idx += kBeamThreads) {
        const int n = idx / L, pos = idx - n * L;
        const int len = n < cnt ? s_len[cur][n] : 0;
        if (pos >= len) p.tokens[((int64_t)b * N + n) * L + pos] = -1;
    }
}

}  // namespace ctc

using namespace ctc;

static bool beam_sizes_ok(int T, int B, int W)
{
    return T >= 1 && B >= 1 && W >= 1 && W <= kBeamMaxW && (int64_t)T * W + 1 <= INT_MAX;
}

extern "C" size_t ctc_amd_beam_search_scratch_bytes(int T, int B, int W)
{
    if (!beam_sizes_ok(T, B, W)) return 0;
    return (size_t)B * ((size_t)T * W + 1) * sizeof(int2);
}

// the checks both entries share, and the plain kernel's arguments
static int beam_params(BeamParams &p, const float *x, int64_t stride_t, int64_t stride_b, const int64_t *in_len,
                       int T, int B, int C, int blank, int W, int K, int N, int L,
                       int32_t *tokens, int64_t *lengths, float *scores, int32_t *count,
                       void *scratch, size_t scratch_bytes)
{
    if (!x || !in_len || !tokens || !lengths || !scores || !count || !scratch) return CTC_AMD_ERR_BAD_ARGUMENT;
    if (!beam_sizes_ok(T, B, W) || C < 2 || blank >= C) return CTC_AMD_ERR_BAD_ARGUMENT;
    if (N < 1 || N > W || K < 1 || K > kBeamMaxK || L < 1 || (int64_t)N * L > INT_MAX) return CTC_AMD_ERR_BAD_ARGUMENT;
    if (scratch_bytes < ctc_amd_beam_search_scratch_bytes(T, B, W)) return CTC_AMD_ERR_BAD_ARGUMENT;
    p.x = x; p.st = stride_t; p.sb = stride_b; p.in_len = in_len;
    p.T = T; p.B = B; p.C = C; p.blank = blank < 0 ? -1 : blank;
    const int classes = blank < 0 ? C : C - 1;                  // the classes a prefix can be extended by
    p.W = W; p.K = K < classes ? K : classes; p.N = N; p.L = L;
    p.tokens = tokens; p.lengths = lengths; p.scores = scores; p.count = count;
    p.trie = static_cast<int2 *>(scratch);
    return 0;
}

extern "C" int ctc_amd_beam_search(const float *x, int64_t stride_t, int64_t stride_b, const int64_t *in_len,
                                   int T, int B, int C, int blank, int W, int K, int N, int L,
                                   int32_t *tokens, int64_t *lengths, float *scores, int32_t *count,
                                   void *scratch, size_t scratch_bytes, void *stream)
{
    BeamParams p;
    const int rc = beam_params(p, x, stride_t, stride_b, in_len, T, B, C, blank, W, K, N, L, tokens, lengths, scores, count,
                               scratch, scratch_bytes);
    if (rc != 0) return rc;
    return launch<beam_search_kernel<false>>(dim3(B), dim3(kBeamThreads), 0, static_cast<hipStream_t>(stream), p);
}

extern "C" int ctc_amd_beam_search_lm(const float *x, int64_t stride_t, int64_t stride_b, const int64_t *in_len,
                                      int T, int B, int C, int blank, int W, int K, int N, int L,
                                      const float *lm, int64_t lm_stride, float lm_weight, float token_bonus,
                                      int32_t *tokens, int64_t *lengths, float *scores, float *ctc_scores, int32_t *count,
                                      void *scratch, size_t scratch_bytes, void *stream)
{
    if (!lm || !ctc_scores || lm_stride < C) return CTC_AMD_ERR_BAD_ARGUMENT;
    if (!(lm_weight >= 0.0f) || !__builtin_isfinite(lm_weight) || !__builtin_isfinite(token_bonus))
        return CTC_AMD_ERR_BAD_ARGUMENT;
    BeamLmParams p;
    const int rc = beam_params(p, x, stride_t, stride_b, in_len, T, B, C, blank, W, K, N, L, tokens, lengths, scores, count,
                               scratch, scratch_bytes);
    if (rc != 0) return rc;
    p.lm = lm; p.lm_stride = lm_stride; p.lm_weight = lm_weight; p.token_bonus = token_bonus; p.ctc_scores = ctc_scores;
    return launch<beam_search_kernel<true>>(dim3(B), dim3(kBeamThreads), 0, static_cast<hipStream_t>(stream), p);
}
