// One record per target label on the no-blank and the binary lattice (ctc_amd_noblank_token_spans,
// ctc_amd_binary_token_spans): where the best path puts label j, where it ends, and the mean posterior
// of the frames it owns.  Included by decode.hip behind the best-path kernels, whose emission stage
// (noblank_emissions / binary_emissions) and max-scan (viterbi_wave) it runs unchanged: path and score are theirs.
//
// ONE launch, one 1024-thread workgroup per sample, everything between the logits and the outputs in LDS:
//   1. emissions   all 16 waves: em[T_b][SP], the sentinel in masked cells and in kPrefetch pad rows on both sides
//   2. three waves wave 0: viterbi_wave<K> and the walk back (path to memory and to LDS); wave 1: alpha; wave 2: beta'
//                  (lattice_chain<K>, lattice.hpp); wave 3 clears the span boundaries
//   3. confidences one wave per live row: gamma_t(l) = exp(alpha + beta' - e) normalised over the row (posterior_row's
//                  arithmetic without the repeat folding), of which only gamma_t(path_t) is kept: frame_conf
//   4. spans       one lane per frame finds the boundaries on the path; one lane per label sums its frames in
//                  ascending t and divides once
// gamma [B,T,S] is never written.  No atomics, no hand-off between workgroups, nothing polls: deterministic.
// LDS per sample: 13 bytes per cell of T x SP (em, alpha, beta' in fp32, one back-pointer byte), 8 SP floats of pad
// rows, 8 bytes per frame, and the label table (no-blank: SP ints) or the waves' row buffers (binary: 16 C floats).
#pragma once

namespace ctc {

constexpr int kTokThreads = 1024;
constexpr int kTokWaves = kTokThreads / kWave;

struct TokenSpanParams {
    DecodeParams d;                             // inputs, shape, path, score
    float *nll;                                 // [B]
    float *frame_conf;                          // [B][T]
    int32_t *start, *end;                       // [B][S]
    float *conf;                                // [B][S]
};

// `extra`: floats behind the span boundaries -- the label table (no-blank) or the waves' row buffers (binary)
struct TokenSmem {
    float *em, *al, *be, *fc, *dummy, *extra;
    int *path, *start, *end;
    unsigned char *bp;
    __device__ TokenSmem(float *base, int T, int SP, size_t nextra)
    {
        em = base + kPrefetch * SP;                     // pad rows on both sides (lattice.hpp)
        al = em + (size_t)(T + kPrefetch) * SP;
        be = al + (size_t)T * SP;
        fc = be + (size_t)T * SP;                       // [T] frame confidences
        dummy = fc + T;                                 // 8 spare floats for the chains' idle lanes
        path = reinterpret_cast<int *>(dummy + 8);      // [T]
        start = path + T;                               // [SP]
        end = start + SP;                               // [SP]
        extra = reinterpret_cast<float *>(end + SP);
        bp = reinterpret_cast<unsigned char *>(extra + nextra);   // [T][SP]
    }
};
static size_t token_smem_bytes(int T, int SP, size_t nextra)
{
    return ((size_t)(3 * T + 2 * kPrefetch) * SP + 2 * (size_t)T + 8 + 2 * (size_t)SP + nextra) * 4 + (size_t)T * SP + 16;
}

__device__ __forceinline__ void token_pad_rows(const TokenSmem &sm, int T, int SP)
{
    for (int i = threadIdx.x; i < kPrefetch * SP; i += kTokThreads) {
        sm.em[i - kPrefetch * SP] = kNeg;
        sm.em[T * SP + i] = kNeg;
    }
    if (threadIdx.x < 8) sm.dummy[threadIdx.x] = 0.f;
}

// stages 2 to 4, behind the workgroup barrier that ends the emission stage
template <int K>
__device__ __forceinline__ void token_spans_tail(const TokenSmem &sm, const TokenSpanParams &q, int b, int Tb, int L, bool ok)
{
    const DecodeParams &p = q.d;
    const int tid = threadIdx.x, w = wave_id(), lane = lane_id(), SP = p.SP;
    if (w == 0) {
        viterbi_wave<K>(sm.em, sm.bp, p, b, Tb, L, ok, sm.path);
    } else if (w == 1 || w == 2) {
        if (Tb > 0) {
            const bool rot = SP <= 63 * K;
            if (w == 1) {
                if (rot) lattice_chain<K, true, true>(sm.em, sm.al, sm.dummy, Tb, L, SP);
                else lattice_chain<K, true, false>(sm.em, sm.al, sm.dummy, Tb, L, SP);
            } else {
                if (rot) lattice_chain<K, false, true>(sm.em, sm.be, sm.dummy, Tb, L, SP);
                else lattice_chain<K, false, false>(sm.em, sm.be, sm.dummy, Tb, L, SP);
            }
        }
    } else if (w == 3) {
        for (int j = lane; j < SP; j += kWave) {
            sm.start[j] = -1;
            sm.end[j] = -1;
        }
    }
    __syncthreads();

    const float nll = ok ? -sm.al[(Tb - 1) * SP + (L - 1)] : -kNeg;
    const bool feasible = ok && nll < kInfeasible;
    if (tid == 0) q.nll[b] = feasible ? nll : __builtin_inff();

    // frame_conf[t] = gamma_t(path_t): state l of the row sits in lane l % 64 at k = l / 64
    for (int t = w; t < p.T; t += kTokWaves) {
        const int pt = __builtin_amdgcn_readfirstlane((feasible && t < Tb) ? sm.path[t] : -1);
        float val = 0.f;
        if (pt >= 0) {
            const int off = t * SP;
            float v[K];
            float m = -__builtin_inff();
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const int l = lane + kWave * k;
                v[k] = l < L ? cell_posterior_log(sm.al[off + l], sm.be[off + l], sm.em[off + l]) : -__builtin_inff();
                m = fmaxf(m, v[k]);
            }
            m = wave_max(m);
            float s = 0.f, pick = 0.f;
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const float pe = lane + kWave * k < L ? fast_exp(v[k] - m) : 0.f;
                s += pe;
                pick = (pt >> 6) == k ? pe : pick;
            }
            s = wave_sum(s);
            val = pick * (1.0f / s);
        }
        if (lane == (pt >= 0 ? (pt & (kWave - 1)) : 0)) {
            sm.fc[t] = val;
            q.frame_conf[(int64_t)b * p.T + t] = val;
        }
    }
    __syncthreads();

    // boundaries: the path is monotone, one label per step, so a label's frames are contiguous and each boundary has
    // one writer
    for (int t = tid; t < Tb; t += kTokThreads) {
        const int j = sm.path[t];
        if (j >= 0 && j < p.S) {
            if (t == 0 || sm.path[t - 1] != j) sm.start[j] = t;
            if (t == Tb - 1 || sm.path[t + 1] != j) sm.end[j] = t + 1;
        }
    }
    __syncthreads();
    // conf = (sum of frame_conf over start .. end - 1, from 0.0f, ascending t, fp32) / float(end - start)
    for (int j = tid; j < p.S; j += kTokThreads) {
        int t0 = sm.start[j], t1 = sm.end[j];
        float c = 0.f;
        if (t0 >= 0 && t1 > t0) {
            float acc = 0.0f;
            for (int t = t0; t < t1; ++t) acc += sm.fc[t];
            c = __fdiv_rn(acc, (float)(t1 - t0));
        } else {
            t0 = t1 = -1;
        }
        const int64_t o = (int64_t)b * p.S + j;
        q.start[o] = t0;
        q.end[o] = t1;
        q.conf[o] = c;
    }
}

template <int K, typename E = float>
__global__ __launch_bounds__(kTokThreads) void noblank_token_spans_kernel(TokenSpanParams q)
{
    extern __shared__ float4 smem_raw[];
    const DecodeParams &p = q.d;
    const TokenSmem sm(reinterpret_cast<float *>(smem_raw), p.T, p.SP, p.SP);
    const int b = blockIdx.x;
    const int64_t Tb64 = p.in_len[b], L64 = p.tgt_len[b];
    const bool ok = L64 >= 1 && L64 <= p.S && Tb64 >= L64 && Tb64 <= p.T;
    const int Tb = ok ? (int)Tb64 : 0, L = ok ? (int)L64 : 0;
    token_pad_rows(sm, p.T, p.SP);
    noblank_emissions<kTokWaves, E>(p, sm.em, reinterpret_cast<int *>(sm.extra), b, Tb, L);
    __syncthreads();
    token_spans_tail<K>(sm, q, b, Tb, L, ok);
}

template <int K, typename E = float>
__global__ __launch_bounds__(kTokThreads) void binary_token_spans_kernel(TokenSpanParams q, const float *y)
{
    extern __shared__ float4 smem_raw[];
    const DecodeParams &p = q.d;
    const TokenSmem sm(reinterpret_cast<float *>(smem_raw), p.T, p.SP, (size_t)kTokWaves * p.C);
    const int b = blockIdx.x;
    const int64_t Tb64 = p.in_len[b], L64 = p.tgt_len[b];
    const bool ok = L64 >= 1 && L64 <= p.S && Tb64 >= L64 && Tb64 <= p.T;
    const int Tb = ok ? (int)Tb64 : 0, L = ok ? (int)L64 : 0;
    token_pad_rows(sm, p.T, p.SP);
    binary_emissions<kTokWaves, E>(p, y, sm.em, sm.extra, b, Tb, L);
    __syncthreads();
    token_spans_tail<K>(sm, q, b, Tb, L, ok);
}

// y == nullptr: the no-blank lattice.  E: the element type of q.d.x
template <typename E>
static int run_token_spans(const TokenSpanParams &q, const float *y, int K, hipStream_t s)
{
    const DecodeParams &p = q.d;
    const size_t smem = token_smem_bytes(p.T, p.SP, y ? (size_t)kTokWaves * p.C : (size_t)p.SP);
    if (smem > kMaxLds) return CTC_AMD_ERR_UNSUPPORTED_SHAPE;
    const dim3 grid(p.B), block(kTokThreads);
    if (y) {
        switch (K) {
            case 1: return launch<binary_token_spans_kernel<1, E>>(grid, block, smem, s, q, y);
            case 2: return launch<binary_token_spans_kernel<2, E>>(grid, block, smem, s, q, y);
            default: return launch<binary_token_spans_kernel<4, E>>(grid, block, smem, s, q, y);
        }
    }
    switch (K) {
        case 1: return launch<noblank_token_spans_kernel<1, E>>(grid, block, smem, s, q);
        case 2: return launch<noblank_token_spans_kernel<2, E>>(grid, block, smem, s, q);
        default: return launch<noblank_token_spans_kernel<4, E>>(grid, block, smem, s, q);
    }
}

}  // namespace ctc
