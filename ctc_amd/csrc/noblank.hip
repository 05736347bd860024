// Fused no-blank CTC loss + input gradient for gfx950 (MI355X).
//
// Replaces NoBlankCTC.forward (NoBlankCTC.py:129-141) and the autograd backward the
// reference runs over it (train.py:444).  One 16-wave workgroup per sample b, one launch:
//
//   P1  at kernel entry every wave issues the loads of its kRows rows x[t,b,:]
//       (coalesced 256-B requests; the rows then STAY in registers until P3).  While
//       they are in flight the workgroup builds the label tables.  Row max / sum-exp
//       (LogSoftmax(dim=2), :136) by DPP reductions; the S emissions
//       e[t,l] = lp[t, lab[l]] (:96-102) are gathered out of the row registers with
//       ds_bpermute and stored to LDS.
//   P2  wave 0 runs the alpha scan, wave 1 the mirrored beta' scan, concurrently,
//       one lattice row per step, states across lanes (lattice.hpp).
//   P3  each wave turns its own rows into gradient: gamma_t = softmax_l(alpha_t +
//       beta'_t - e_t) (row-normalised; repeated labels folded onto the first
//       occurrence), grad = scale * (softmax(x) - gamma scattered by class) from the
//       resident row registers, written with 256-B coalesced stores.
//
// The batch mean is taken in-launch by the last workgroup to publish its nll
// (common.hpp), overlapped with P3.  HBM traffic = read x once, write grad once.
// Shapes beyond the register-resident tiling (T > 160 rows per pass, C > 256) fall
// back to re-reading rows from L2 in P3 / to strided row passes.
#include <type_traits>

#include "lattice.hpp"
#include "launch.hpp"

namespace ctc {

struct NoblankParams {
    const float *x;
    int64_t st, sb;
    const void *lab;
    int lab64;
    const int64_t *in_len, *tgt_len;
    int T, B, C, S, SP;
    int stop;                   // debug: leave after phase `stop` (0 = run everything);
                                // < 0: workgroup 0 / wave -stop-1 stamps (s_memtime, s_memrealtime)
                                // pairs into workspace bytes [64,256) at each phase boundary
    float loss_scale, grad_scale;
    float *nll, *loss, *grad;
    float *gamma;               // optional [B][T][S] posteriors output (ctc_amd_noblank_posteriors)
    float *lattice;             // global-memory lattice slabs (workspace, behind header and list) when T x S exceeds LDS
    int64_t slab;               // floats per sample in `lattice`
    unsigned *counter;
    int next_round;             // > 0: B exceeds one round of workgroups -- blocks prefetch for block + next_round
    float ls_a, ls_b;           // label-smoothed emission a lp[c_l] + b sum_n lp[n] (NoBlankCTC.py:100-107); 1, 0: plain
    int koff;                   // noblank_km_kernel: what the exponent recurrence starts with (log2 of the path count / 2)
    const float *upstream;      // r16 kernel: a folded scale_grad call's grad_out -- every gradient value is multiplied by
                                // *upstream as it is stored (launch.hpp); null: 1.  The other kernels never read it.
};

// Every field through an empty volatile asm: the copy holds the same values, but the compiler no longer knows that
// they are the launch's constants.  For kernels that LOOP over samples: whatever is computed from `p` inside the loop
// stays inside (hoisted out, the address arithmetic of a whole sample waits in registers for its turn -- see
// noblank_r16_kernel<.., PS>).
__device__ __forceinline__ NoblankParams opaque_params(NoblankParams q)
{
#define CTC_OPQ(f) asm volatile("" : "+s"(q.f))
    CTC_OPQ(x); CTC_OPQ(st); CTC_OPQ(sb); CTC_OPQ(lab); CTC_OPQ(lab64); CTC_OPQ(in_len); CTC_OPQ(tgt_len);
    CTC_OPQ(T); CTC_OPQ(B); CTC_OPQ(C); CTC_OPQ(S); CTC_OPQ(SP); CTC_OPQ(stop); CTC_OPQ(loss_scale); CTC_OPQ(grad_scale);
    CTC_OPQ(nll); CTC_OPQ(loss); CTC_OPQ(grad); CTC_OPQ(gamma); CTC_OPQ(lattice); CTC_OPQ(slab); CTC_OPQ(counter);
    CTC_OPQ(next_round); CTC_OPQ(ls_a); CTC_OPQ(ls_b); CTC_OPQ(koff); CTC_OPQ(upstream);
#undef CTC_OPQ
    return q;
}

#ifndef CTC_NOBLANK_THREADS
#define CTC_NOBLANK_THREADS 1024
#endif
constexpr int kThreads = CTC_NOBLANK_THREADS;  // 16 waves: one pass of kRows rows each covers T <= 160
constexpr int kWaves = kThreads / kWave;
constexpr int kRows = 160 / kWaves;            // rows of x resident per wave
constexpr int kRowsPerPass = kWaves * kRows;

struct NoblankSmem {
    float *em, *al, *be, *mx, *ls, *dummy;
    int *cnt, *lab, *nxt, *dup, *inv;
    // `glb` != nullptr: the T x S arrays live in that global slab (long sequences), only the
    // small tables stay in LDS
    __device__ NoblankSmem(float *base, int T, int SP, int C, float *glb = nullptr)
    {
        float *lat = glb ? glb : base;
        em = lat + kPrefetch * SP;                      // pad rows on both sides (lattice.hpp)
        al = em + (size_t)(T + kPrefetch) * SP;
        be = al + (size_t)T * SP;
        mx = be + (size_t)T * SP;
        ls = mx + T;
        dummy = glb ? base : ls + T;
        cnt = reinterpret_cast<int *>(dummy + 8);            // 16 progress counters (pipelined kernel)
        lab = cnt + 16;
        nxt = lab + SP;
        dup = nxt + SP;
        inv = dup + SP;
    }
};

static size_t noblank_lattice_floats(int T, int SP) { return (size_t)(3 * T + 2 * kPrefetch) * SP + 2 * (size_t)T; }
static size_t noblank_tables_bytes(int SP, int C) { return (8 + 16 + 3 * (size_t)SP + C + 4) * 4; }
static size_t noblank_smem_bytes(int T, int SP, int C)
{
    return noblank_lattice_floats(T, SP) * 4 + noblank_tables_bytes(SP, C);
}
// What a shape needs of the phase-serial kernel (noblank_fused_kernel), which takes every supported shape.  `glb`: a
// long sequence -- the T x S lattice does not fit in LDS and lives in the workspace, one slab per sample; `smem` then
// counts the tables alone.  K > 4 or smem > kMaxLds: no kernel takes the shape.
struct NoblankSizes {
    int K, SP;
    bool glb;
    size_t smem;
};
static NoblankSizes noblank_sizes(int T, int C, int S)
{
    const auto [K, SP] = lane_states(S);
    const size_t smem = noblank_smem_bytes(T, SP, C);
    if (smem <= kMaxLds) return {K, SP, false, smem};
    return {K, SP, true, noblank_tables_bytes(SP, C)};
}
// extra workspace (beyond the first 256 B) of the no-blank entry points: 0 while the lattice
// fits in LDS, else one slab per sample
size_t noblank_extra_workspace(int T, int B, int C, int S)
{
    const NoblankSizes z = noblank_sizes(T, C, S);
    if (z.K > 4 || !z.glb) return 0;
    return (size_t)B * noblank_lattice_floats(T, z.SP) * 4;
}

__device__ __forceinline__ const float *row_ptr(const NoblankParams &p, int t, int b)
{
    return p.x + (int64_t)t * p.st + (int64_t)b * p.sb;
}

// ---- register-resident rows (C <= 64*CH) ------------------------------------------
template <int CH>
struct Rows {
    float v[kRows][CH];

    // rows t0..t0+kRows-1.  Every load is issued unconditionally (row / column indices
    // clamped into range) so that the compiler can wait for OLDER loads with an exact
    // vmcnt(N) while these stay in flight; out-of-range values are masked at the use.
    __device__ __forceinline__ void load(const NoblankParams &p, int b, int t0, int tmax)
    {
        const int lane = lane_id();
        const int tlast = tmax > 0 ? tmax - 1 : 0;
#pragma unroll
        for (int r = 0; r < kRows; ++r) {
            const float *row = row_ptr(p, t0 + r < tlast ? t0 + r : tlast, b);
#pragma unroll
            for (int j = 0; j < CH; ++j) {
                const int c = lane + 64 * j;
                v[r][j] = row[c < p.C ? c : p.C - 1];
            }
        }
    }

    // LogSoftmax statistics + emission gather for rows < Tb (NoBlankCTC.py:136, :96-102)
    __device__ __forceinline__ void emit(const NoblankParams &p, const NoblankSmem &sm, int t0, int Tb, int L)
    {
        const int lane = lane_id();
#pragma unroll
        for (int r = 0; r < kRows; ++r) {
            const int t = t0 + r;
            if (t >= Tb) break;                              // wave-uniform
            const float ninf = -__builtin_inff();
            float m = ninf;
#pragma unroll
            for (int j = 0; j < CH; ++j) m = fmaxf(m, lane + 64 * j < p.C ? v[r][j] : ninf);
            m = wave_max(m);
            float s = 0.f;
#pragma unroll
            for (int j = 0; j < CH; ++j) s += lane + 64 * j < p.C ? fast_exp(v[r][j] - m) : 0.f;
            s = wave_sum(s);
            const float lsum = fast_log(s);
            if (lane == 0) { sm.mx[t] = m; sm.ls[t] = lsum; }
            for (int lb = 0; lb < p.SP; lb += kWave) {       // wave-uniform trips (one when S <= 64):
                const int l = lb + lane;                      // every lane must stay active, it is a
                const int k = l < p.SP ? sm.lab[l] : 0;       // bpermute SOURCE for the other lanes
                float xv = 0.f;
#pragma unroll
                for (int j = 0; j < CH; ++j) {
                    const float q = __shfl(v[r][j], k & 63, kWave);
                    if ((k >> 6) == j) xv = q;
                }
                if (l < p.SP) sm.em[t * p.SP + l] = (l < L) ? masked_floor((xv - m) - lsum) : kNeg;
            }
        }
    }

    __device__ __forceinline__ void grad(const NoblankParams &p, const NoblankSmem &sm, int b, int t0,
                                         int Tlive, const int (&first)[CH])
    {
        const int lane = lane_id();
#pragma unroll
        for (int r = 0; r < kRows; ++r) {
            const int t = t0 + r;
            if (t >= p.T) break;                             // wave-uniform
            float *g = p.grad + ((int64_t)t * p.B + b) * p.C;
            if (t < Tlive) {
                const float m = sm.mx[t], lsum = sm.ls[t];
#pragma unroll
                for (int j = 0; j < CH; ++j) {
                    const int c = lane + 64 * j;
                    if (c < p.C) {
                        const float occ = first[j] >= 0 ? sm.be[t * p.SP + first[j]] : 0.f;
                        stream_store(&g[c], p.grad_scale * (fast_exp((v[r][j] - m) - lsum) - occ));
                    }
                }
            } else {
#pragma unroll
                for (int j = 0; j < CH; ++j) {
                    const int c = lane + 64 * j;
                    if (c < p.C) stream_store(&g[c], 0.f);
                }
            }
        }
    }
};

// ---- generic rows (C > 256): strided passes, rows come back from L1/L2 -------------
__device__ __forceinline__ void rows_emit_generic(const NoblankParams &p, const NoblankSmem &sm, int b, int Tb, int L)
{
    const int lane = lane_id();
    for (int t = wave_id(); t < Tb; t += kWaves) {
        const float *row = row_ptr(p, t, b);
        float m = -__builtin_inff();
        for (int c = lane; c < p.C; c += kWave) m = fmaxf(m, row[c]);
        m = wave_max(m);
        float s = 0.f;
        for (int c = lane; c < p.C; c += kWave) s += fast_exp(row[c] - m);
        s = wave_sum(s);
        const float lsum = fast_log(s);
        if (lane == 0) { sm.mx[t] = m; sm.ls[t] = lsum; }
        for (int l = lane; l < p.SP; l += kWave)
            sm.em[t * p.SP + l] = (l < L) ? masked_floor((row[sm.lab[l]] - m) - lsum) : kNeg;
    }
}

__device__ __forceinline__ void rows_grad_generic(const NoblankParams &p, const NoblankSmem &sm, int b, int Tlive, int L)
{
    const int lane = lane_id();
    const int G = posterior_group(p.SP), per = kWave / G, sub = lane / G;
    for (int t0 = wave_id() * per; t0 < Tlive; t0 += kWaves * per)
        posterior_row<true>(sm.al, sm.be, sm.em, sm.nxt, sm.dup, t0 + sub, t0 + sub < Tlive, L, p.SP, G);
    __syncthreads();
    for (int t = wave_id(); t < p.T; t += kWaves) {
        const float *row = row_ptr(p, t, b);
        float *g = p.grad + ((int64_t)t * p.B + b) * p.C;
        if (t < Tlive) {
            const float m = sm.mx[t], lsum = sm.ls[t];
            for (int c = lane; c < p.C; c += kWave) {
                const int f = sm.inv[c];
                stream_store(&g[c], p.grad_scale * (fast_exp((row[c] - m) - lsum) - (f >= 0 ? sm.be[t * p.SP + f] : 0.f)));
            }
        } else {
            for (int c = lane; c < p.C; c += kWave) stream_store(&g[c], 0.f);
        }
    }
}

// label tables: lab[] (0 beyond L: those lanes only feed masked cells), first-occurrence
// map inv[], next-duplicate chain nxt[], dup[] flags.  inv/nxt/dup are consumed in P3,
// behind later barriers.
__device__ __forceinline__ void build_label_tables(const NoblankParams &p, const NoblankSmem &sm, int raw_label, int L)
{
    const int tid = threadIdx.x;
    if (tid < p.SP) {                                        // SP <= 256 < kThreads
        int k = 0;
        if (tid < L) {
            k = raw_label % p.C;
            if (k < 0) k += p.C;                             // python negative index (:102)
        }
        sm.lab[tid] = k;
    }
    for (int c = tid; c < p.C; c += kThreads) sm.inv[c] = 0x7fffffff;
    __syncthreads();
    if (tid < L) {
        const int k = sm.lab[tid];
        atomicMin(&sm.inv[k], tid);
        int n = -1;
        for (int l2 = tid + 1; l2 < L; ++l2)
            if (sm.lab[l2] == k) { n = l2; break; }
        sm.nxt[tid] = n;
    }
    __syncthreads();
    for (int c = tid; c < p.C; c += kThreads)
        if (sm.inv[c] == 0x7fffffff) sm.inv[c] = -1;
    if (tid < p.SP) sm.dup[tid] = (tid < L && sm.inv[sm.lab[tid]] == tid && sm.nxt[tid] >= 0) ? 1 : 0;
}

// CH = 0: generic rows (C > 256).  GLB: lattice in global memory (T x S beyond LDS; slower:
// the chains then prefetch their rows from L2) -- completeness path for long sequences.
template <int K, int CH, bool GLB = false>
__global__ __launch_bounds__(kThreads) void noblank_fused_kernel(NoblankParams p)
{
    extern __shared__ float4 smem_raw[];
    const int b = xcd_sample(blockIdx.x, p.B), tid = threadIdx.x, w = wave_id();
    if (tid == kThreads - 64) note_arrival(p.counter, b);       // (the last wave: its first wait is the workgroup barrier)
    const NoblankSmem sm(reinterpret_cast<float *>(smem_raw), p.T, p.SP, p.C,
                         GLB ? p.lattice + (int64_t)b * p.slab : nullptr);
    constexpr int CHR = CH > 0 ? CH : 1;
    Rows<CHR> rows;

    // loads first, oldest = needed first (vmcnt retires in order): the two lengths, this
    // thread's label, then the wave's rows of x -- the label tables are built while the
    // rows are still in flight
    stamp(p, 0);
    const int64_t Tb64 = p.in_len[b], L64 = p.tgt_len[b];
    const int raw_label = tid < p.S ? load_label(p.lab, p.lab64, (int64_t)b * p.S + tid) : 0;
    if (CH > 0) rows.load(p, b, w * kRows, p.T);

    // contract: 1 <= L_b <= S, L_b <= T_b <= T (the dataset guarantees it,
    // charades_ctc_next_pred.py:609-610); anything else has no alignment.
    const bool ok = L64 >= 1 && L64 <= p.S && Tb64 >= L64 && Tb64 <= p.T;
    const int Tb = ok ? (int)Tb64 : 0, L = ok ? (int)L64 : 0;

    build_label_tables(p, sm, raw_label, L);
    if (tid < 8) sm.dummy[tid] = 0.f;
    for (int i = tid; i < kPrefetch * p.SP; i += kThreads) {          // pad rows of em
        sm.em[i - kPrefetch * p.SP] = kNeg;
        sm.em[p.T * p.SP + i] = kNeg;
    }
    if (CTC_DIAG(p) == 1) return;
    stamp(p, 1);

    // P1 (passes beyond the first are processed first so that pass 0 stays resident)
    if (CH > 0) {
        for (int base = ((Tb - 1) / kRowsPerPass) * kRowsPerPass; base > 0; base -= kRowsPerPass) {
            Rows<CHR> extra;
            extra.load(p, b, base + w * kRows, Tb);
            extra.emit(p, sm, base + w * kRows, Tb, L);
        }
        rows.emit(p, sm, w * kRows, Tb, L);
    } else {
        rows_emit_generic(p, sm, b, Tb, L);
    }
    stamp(p, 2);
    __syncthreads();
    if (CTC_DIAG(p) == 2) return;
    stamp(p, 3);

    // P2
    if (Tb > 0) {
        const bool rot = p.SP <= 63 * K;
        if (w == 0) {
            if (rot) lattice_chain<K, true, true>(sm.em, sm.al, sm.dummy, Tb, L, p.SP);
            else lattice_chain<K, true, false>(sm.em, sm.al, sm.dummy, Tb, L, p.SP);
        } else if (w == 1 && (p.grad || p.gamma)) {
            if (rot) lattice_chain<K, false, true>(sm.em, sm.be, sm.dummy, Tb, L, p.SP);
            else lattice_chain<K, false, false>(sm.em, sm.be, sm.dummy, Tb, L, p.SP);
        }
    }
    stamp(p, 4);
    __syncthreads();
    if (CTC_DIAG(p) == 3) return;
    stamp(p, 5);

    const float nll = ok ? -sm.al[(Tb - 1) * p.SP + (L - 1)] : -kNeg;   // readout, :58-68,139
    // published by the LAST wave: it owns the fewest rows (none when T <= 150), so the
    // store-drain + ticket round trip stays off the other waves' critical path
    if (w == kWaves - 1)
        publish_and_reduce_sum(nll, b, p.B, p.nll, p.loss, p.loss_scale, p.counter);
    if (!p.grad && !p.gamma) return;

    // P3
    const bool feasible = ok && nll < kInfeasible;
    const int Tlive = feasible ? Tb : 0;
    if (p.gamma) {                                           // posteriors output (no folding): own pass
        const int G = posterior_group(p.SP), per = kWave / G, sub = lane_id() / G;
        for (int t0 = w * per; t0 < p.T; t0 += kWaves * per) {
            const int t = t0 + sub;
            posterior_row<false>(sm.al, sm.be, sm.em, nullptr, nullptr, t, t < Tlive, L, p.SP, G);
            if (t < p.T)
                for (int l = lane_id() % G; l < p.S; l += G)
                    p.gamma[((int64_t)b * p.T + t) * p.S + l] = t < Tlive ? sm.be[t * p.SP + l] : 0.f;
        }
        return;
    }
    if (CH > 0) {
        const int lane = lane_id();
        int first[CHR];
#pragma unroll
        for (int j = 0; j < CHR; ++j) {
            const int c = lane + 64 * j;
            first[j] = (c < p.C) ? sm.inv[c] : -1;
        }
        const int G = posterior_group(p.SP), per = kWave / G, sub = lane / G;
        for (int base = 0; base < p.T; base += kRowsPerPass) {
            const int t0 = base + w * kRows;
            for (int r = 0; r < kRows; r += per)             // this wave's own rows: wave-local
                if (t0 + r < Tlive)
                    posterior_row<true>(sm.al, sm.be, sm.em, sm.nxt, sm.dup, t0 + r + sub,
                                  r + sub < kRows && t0 + r + sub < Tlive, L, p.SP, G);
            if (CTC_DIAG(p) == 4) continue;
            stamp(p, 6);
            if (base == 0) {
                rows.grad(p, sm, b, t0, Tlive, first);
            } else {
                Rows<CHR> extra;
                extra.load(p, b, t0, Tlive);
                extra.grad(p, sm, b, t0, Tlive, first);
            }
        }
    } else {
        rows_grad_generic(p, sm, b, Tlive, L);
    }
    stamp(p, 7);
}

}  // namespace ctc

#include "noblank_pipe.hpp"
#include "noblank_xr.hpp"
#include "noblank_r16.hpp"
#ifdef CTC_AMD_DIAGNOSTICS                                    // measured and not taken: A/B through CTC_AMD_KM=1
#include "noblank_km.hpp"
#endif

namespace ctc {

__global__ __launch_bounds__(256) void scale_grad_kernel(float *g, const float *go, size_t n)
{
    const float s = *go;
    if (s == 1.0f) return;                                   // loss.backward(): nothing to do
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if ((reinterpret_cast<uintptr_t>(g) & 15) == 0) {
        float4 *g4 = reinterpret_cast<float4 *>(g);
        const size_t n4 = n / 4;
        for (size_t k = i; k < n4; k += stride) {
            float4 v = g4[k];
            v.x *= s; v.y *= s; v.z *= s; v.w *= s;
            g4[k] = v;
        }
        for (size_t k = n4 * 4 + i; k < n; k += stride) g[k] *= s;
    } else {
        for (size_t k = i; k < n; k += stride) g[k] *= s;
    }
}

// the same for a 2-byte gradient (ctc_amd_scale_grad_typed): round(float(g) * s), 8 bytes per access where the array is
// 8-byte aligned
template <typename E>
__global__ __launch_bounds__(256) void scale_grad_lowp_kernel(E *g, const float *go, size_t n)
{
    const float s = *go;
    if (s == 1.0f) return;                                   // loss.backward(): nothing to do
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    size_t done = 0;
    if ((reinterpret_cast<uintptr_t>(g) & 7) == 0) {
        wt_u2 *g4 = reinterpret_cast<wt_u2 *>(g);
        const size_t n4 = n / 4;
        const f2_t s2 = {s, s};
        for (size_t k = i; k < n4; k += stride) {
            wt_u2 v = g4[k];
            v.x = r16_narrow2<E>(r16_widen2<E>(v.x) * s2);
            v.y = r16_narrow2<E>(r16_widen2<E>(v.y) * s2);
            g4[k] = v;
        }
        done = n4 * 4;
    }
    // (the tail through the same widen, multiply, narrow as the body: written as `(E)((float)g[k] * s)` the fp16 form
    // compiles to a mixed-precision multiply-ADD of +0, which turns a -0 product into +0)
    for (size_t k = done + i; k < n; k += stride) {
        const unsigned short e = *reinterpret_cast<const unsigned short *>(g + k);
        const f2_t v = r16_widen2<E>((unsigned)e) * f2_t{s, s};
        *reinterpret_cast<unsigned short *>(g + k) = (unsigned short)r16_narrow2<E>(v);
    }
}

// ---- host side of the entry points: parameters, then a plan, then a launch -------------------------

// Forced kernel choices and debug stops of the diagnostics build (launch.hpp: the product library reads none of them).
struct NoblankSwitches {
    bool no_pipe, no_xr, no_r16, no_ps, km;
    bool nograd;                // forward only
    int stop;                   // NoblankParams::stop
};
static const NoblankSwitches &noblank_switches()
{
    static const NoblankSwitches sw = {diag_env("CTC_AMD_NOPIPE") != 0, diag_env("CTC_AMD_NOXR") != 0,
                                       diag_env("CTC_AMD_NOR16") != 0,  diag_env("CTC_AMD_NOPS") != 0,
                                       diag_env("CTC_AMD_KM") != 0,     diag_env("CTC_AMD_DEBUG_NOGRAD") != 0,
                                       diag_env("CTC_AMD_DEBUG_STOP")};
    return sw;
}

// Step 1: what the kernels take, from an entry point's arguments.  `gamma` set: the posteriors call, whose batch-mean
// slot of the in-launch reduction lands in a spare workspace word.  label_smoothing < 0: the plain loss.  next_round
// and koff belong to the plan (noblank_launch).
static int noblank_params(NoblankParams &p, const void *x, int64_t stride_t, int64_t stride_b,
                          const void *labels, int labels_i64, const int64_t *in_len, const int64_t *tgt_len,
                          int T, int B, int C, int S, float loss_scale, float grad_scale,
                          float *nll, float *loss, void *grad, float *gamma, void *workspace, float label_smoothing,
                          const NoblankSwitches &sw)
{
    if (!x || !labels || !in_len || !tgt_len || !nll || !(loss || gamma) || !workspace) return CTC_AMD_ERR_BAD_ARGUMENT;
    if (T < 1 || B < 1 || C < 1 || S < 1) return CTC_AMD_ERR_BAD_ARGUMENT;
    const NoblankSizes z = noblank_sizes(T, C, S);
    char *ws = static_cast<char *>(workspace);
    p.x = static_cast<const float *>(x); p.st = stride_t; p.sb = stride_b;
    p.lab = labels; p.lab64 = labels_i64;
    p.in_len = in_len; p.tgt_len = tgt_len;
    p.T = T; p.B = B; p.C = C; p.S = S; p.SP = z.SP;
    p.stop = sw.stop;
    p.loss_scale = loss_scale; p.grad_scale = grad_scale;
    p.nll = nll; p.loss = gamma ? reinterpret_cast<float *>(ws + 32) : loss;
    p.grad = sw.nograd ? nullptr : static_cast<float *>(grad);
    p.gamma = gamma;
    p.counter = static_cast<unsigned *>(workspace);
    p.lattice = z.glb ? reinterpret_cast<float *>(ws + 256 + acc_list_bytes(B)) : nullptr;   // behind header and list
    p.slab = z.glb ? (int64_t)noblank_lattice_floats(T, z.SP) : 0;
    p.next_round = 0; p.koff = 0;
    p.upstream = nullptr;
    const bool smooth = label_smoothing >= 0.f;
    p.ls_b = smooth ? (1.f - label_smoothing) / (float)C : 0.f;
    p.ls_a = smooth ? label_smoothing - p.ls_b : 1.f;
    return 0;
}

// Step 2: which kernel takes a call.  Everything the choice depends on ...
struct NoblankQuery {
    int T, B, C, S;
    int dtype;                  // CTC_AMD_F32 / _BF16 / _F16: element type of x and grad
    int64_t st, sb;             // strides of x, in elements
    unsigned x_low, grad_low;   // low four bits of the two addresses (no gradient: 0)
    bool want_grad, want_gamma, smooth;
    int cus;                    // compute units of the device
    NoblankSwitches sw;
};
// ... and the choice: the template selectors of the family's kernel, grid, dynamic LDS, NoblankParams::next_round / koff.
enum NoblankFamily { kNoblankUnsupported = 0, kNoblankR16, kNoblankKm, kNoblankXr, kNoblankPipelined, kNoblankFused };
struct NoblankPlan {
    int family;
    int n4, n2, nt, ps;         // r16, km: row chunking (r16_shape), non-temporal gradient stores, persistent form
    int ch, dual;               // xr, pipelined, fused: 64-column chunks of a row (0: generic rows), two workgroups per CU
    int K, glb;                 // fused: states per lane, lattice in the workspace
    int grid;
    size_t lds;
    int next_round, koff;
};

// The four-rows-per-wave kernel (noblank_r16.hpp) takes a shape when one wave holds the states (S <= 31 of K = 1), the
// rows fit its workers (T <= 168, C even <= 256), it can move them in aligned 8-byte pieces -- `align` is what that
// asks of the two addresses: 8 bytes for fp32, 4 bytes for 2-byte elements -- and its arrays fit in LDS.
static bool r16_takes(const NoblankQuery &q, const NoblankSizes &z, unsigned align, int &n4, int &n2)
{
    return z.K == 1 && q.T <= kPipeMaxT && q.C % 2 == 0 && q.st % 2 == 0 && q.sb % 2 == 0 && q.x_low % align == 0 &&
           q.grad_low % align == 0 && r16_shape(q.C, n4, n2) && z.SP <= 31 && r16_smem_bytes(q.T, z.SP, q.C) <= kMaxLds;
}

static NoblankPlan noblank_plan(const NoblankQuery &q)
{
    const NoblankSizes z = noblank_sizes(q.T, q.C, q.S);
    NoblankPlan pl = {};
    if (z.K > 4) return pl;                                  // S <= 256
    const bool lowp = q.dtype != CTC_AMD_F32;
    const int esz = lowp ? 2 : 4, cus = q.cus;
    pl.grid = q.B;
    int n4 = 0, n2 = 0;
    const bool r16 = r16_takes(q, z, lowp ? 4 : 8, n4, n2);
    // label_smoothing: the smoothed emission lives in the r16 kernel only.  2-byte logits: that kernel or nothing (no
    // silent detour through another kernel or an fp32 copy), whatever the switches say.
    const bool r16_only = q.smooth || lowp;
    const bool fast = z.K == 1 && q.C <= 256 && q.T <= kPipeMaxT && !q.sw.no_pipe && !z.glb && !q.want_gamma;
    // The r16 kernel wherever it takes the shape (which then always fits in LDS).  The posteriors: same chains, the
    // gradient phase cut off after the row-normalised posteriors.  The loss: in the common case (S <= 64, C <= 256,
    // T <= 168: the schedules that overlap rows, chains and gradient), also with more samples than CUs: one workgroup
    // per CU at a time still beats two of the one-row-per-wave kind
    // (T = 150, C = 158, us per launch r16 / xr: B = 384 22.5 / 27.7, 512 25.9 / 31.2, 768 37.6 / 45.2,
    // 1024 49.7 / 56.6, 1536 78.2 / 78.5, 2048 101.3 / 99.7)
    if (r16 && (q.want_gamma || lowp || (fast && !q.sw.no_r16))) {
        pl.n4 = n4; pl.n2 = n2;
        pl.lds = r16_smem_bytes(q.T, z.SP, q.C);
        if (q.want_gamma) { pl.family = kNoblankR16; return pl; }
        // logits + gradient beyond the memory-side cache: non-temporal gradient stores
        pl.nt = !within_memory_side_cache(2 * esz, q.T, q.B, q.C);
#ifdef CTC_AMD_DIAGNOSTICS
        // the chains split over exponent and mantissa waves (noblank_km.hpp) wherever its arrays fit and the number of
        // lattice paths leaves two mantissas room in fp32
        const int koff = km_offset(q.T, q.S);
        if (q.sw.km && !lowp && km_smem_bytes(q.T, z.SP, q.C) <= kMaxLds && koff >= 0) {
            pl.family = kNoblankKm;
            pl.lds = km_smem_bytes(q.T, z.SP, q.C);
            pl.koff = koff;
            pl.next_round = (q.B > cus && (size_t)q.T * ((q.C * 4 + 127) / 128) <= (size_t)kKmWorkers * kWave) ? cus : 0;
            return pl;
        }
#endif
        pl.family = kNoblankR16;
        // more samples than CUs: a workgroup prefetches the rows of the sample that follows it on its CU
        pl.next_round = (q.B > cus && (size_t)q.T * ((q.C * esz + 127) / 128) <= (size_t)kPipeWorkers * kWave) ? cus : 0;
        // More than two rounds of samples: one PERSISTENT workgroup per CU that keeps the next sample's rows in a
        // second set of registers (noblank_r16.hpp), wherever two sets fit the 128 VGPRs of a 16-wave workgroup
        // (4 n4 + 2 n2 <= 12, which is C <= 192) and a gradient is wanted.  T = 150, C = 158, us per launch persistent /
        // one sample per workgroup: B = 2048 82.7 / 98.0, 1024 41.7 / 45.1, 512 24.3 / 24.1.
        pl.ps = q.B > 2 * cus && cus > 0 && !q.sw.no_ps && q.want_grad && 4 * n4 + 2 * n2 <= 12;
        if (pl.ps) pl.grid = cus;
        return pl;
    }
    if (r16_only || (z.glb && z.smem > kMaxLds)) return NoblankPlan{};
    if (fast) {
        pl.ch = (q.C + kWave - 1) / kWave;
        pl.dual = q.B > cus && 2 * z.smem <= kMaxLds;        // more samples than CUs: two workgroups per CU
        // extended-range linear lattice (noblank_xr.hpp) wherever its 8-byte cells fit
        const size_t xsmem = xr_smem_bytes(q.T, z.SP, q.C);
        const bool xr = !q.sw.no_xr && xsmem <= kMaxLds && (!pl.dual || 2 * xsmem <= kMaxLds);
        pl.family = xr ? kNoblankXr : kNoblankPipelined;
        pl.lds = xr ? xsmem : z.smem;
        return pl;
    }
    pl.family = kNoblankFused;
    pl.K = z.K; pl.glb = z.glb;
    pl.ch = q.C <= 256 && !z.glb ? (q.C + kWave - 1) / kWave : 0;
    pl.lds = z.smem;
    return pl;
}

// Step 3: the plan's numbers as template arguments (with_constant, launch.hpp).
// f(n4, n2) for the twelve row chunkings that r16_shape gives
template <typename F>
static int with_row_chunks(int n4, int n2, F f)
{
    return with_constant<1, 2, 4, 5, 6, 8, 9, 10, 12, 13, 14, 16>(4 * n4 + n2, [&](auto k) {
        return f(std::integral_constant<int, decltype(k)::value / 4>(), std::integral_constant<int, decltype(k)::value % 4>());
    });
}

static int noblank_launch(const NoblankPlan &pl, int dtype, NoblankParams &p, hipStream_t s)
{
    const dim3 grid(pl.grid), block(kThreads);
    p.next_round = pl.next_round; p.koff = pl.koff;
    switch (pl.family) {
        case kNoblankR16:
            // the persistent form only for the nine chunkings whose two row sets fit the registers (noblank_plan)
            return with_row_chunks(pl.n4, pl.n2, [&](auto n4, auto n2) {
                return with_constant<0, 1>(pl.nt, [&](auto nt) {
                    return with_constant<CTC_AMD_BF16, CTC_AMD_F16, CTC_AMD_F32>(dtype, [&](auto dt) {
                        using E = std::conditional_t<decltype(dt)::value == CTC_AMD_BF16, __bf16,
                                                     std::conditional_t<decltype(dt)::value == CTC_AMD_F16, _Float16, float>>;
                        constexpr int A = decltype(n4)::value, Bq = decltype(n2)::value;
                        constexpr bool NT = decltype(nt)::value != 0;
                        // (the kernel that takes a folded scale_grad: remembered when captured, launch.hpp)
                        const size_t n = (size_t)p.T * p.B * p.C;
                        if constexpr (4 * A + 2 * Bq <= 12)
                            if (pl.ps)
                                return launch_loss<noblank_r16_kernel<A, Bq, NT, true, E>>(grid, block, pl.lds, s, !p.gamma, dtype, n, p);
                        return launch_loss<noblank_r16_kernel<A, Bq, NT, false, E>>(grid, block, pl.lds, s, !p.gamma, dtype, n, p);
                    });
                });
            });
#ifdef CTC_AMD_DIAGNOSTICS
        case kNoblankKm:
            return with_row_chunks(pl.n4, pl.n2, [&](auto n4, auto n2) {
                return with_constant<0, 1>(pl.nt, [&](auto nt) {
                    return launch<noblank_km_kernel<decltype(n4)::value, decltype(n2)::value, decltype(nt)::value != 0>>(
                        grid, block, pl.lds, s, p);
                });
            });
#endif
        case kNoblankXr:
        case kNoblankPipelined:
            return with_constant<1, 2, 3, 4>(pl.ch, [&](auto ch) {
                return with_constant<0, 1>(pl.dual, [&](auto dual) {
                    constexpr int CH = decltype(ch)::value;
                    constexpr bool DUAL = decltype(dual)::value != 0;
                    return pl.family == kNoblankXr ? launch<noblank_xr_kernel<CH, DUAL>>(grid, block, pl.lds, s, p)
                                                   : launch<noblank_pipelined_kernel<CH, DUAL>>(grid, block, pl.lds, s, p);
                });
            });
        case kNoblankFused:
            return with_constant<1, 2, 4>(pl.K, [&](auto k) {
                constexpr int K = decltype(k)::value;
                if (pl.glb) return launch<noblank_fused_kernel<K, 0, true>>(grid, block, pl.lds, s, p);
                return with_constant<1, 2, 3, 4, 0>(pl.ch, [&](auto ch) {
                    return launch<noblank_fused_kernel<K, decltype(ch)::value>>(grid, block, pl.lds, s, p);
                });
            });
        default: return CTC_AMD_ERR_UNSUPPORTED_SHAPE;
    }
}

// All no-blank entry points.  label_smoothing < 0: the plain loss (every kernel); in [0, 1]: the smoothed emission, r16
// kernel only.  x_dtype CTC_AMD_BF16 / CTC_AMD_F16: 2-byte x and grad, the r16 kernel's shape domain only
// (include/ctc_amd.h).  `gamma`: posteriors instead of loss and gradient; they read no diagnostic switch.
static int noblank_run(const void *x, int64_t stride_t, int64_t stride_b,
                       const void *labels, int labels_i64,
                       const int64_t *in_len, const int64_t *tgt_len,
                       int T, int B, int C, int S,
                       float loss_scale, float grad_scale,
                       float *nll, float *loss, void *grad,
                       void *workspace, void *stream, float label_smoothing, int x_dtype = CTC_AMD_F32,
                       float *gamma = nullptr)
{
    const NoblankSwitches sw = gamma ? NoblankSwitches{} : noblank_switches();
    NoblankParams p;
    if (const int rc = noblank_params(p, x, stride_t, stride_b, labels, labels_i64, in_len, tgt_len, T, B, C, S, loss_scale,
                                      grad_scale, nll, loss, grad, gamma, workspace, label_smoothing, sw))
        return rc;
    const NoblankQuery q = {T, B, C, S, x_dtype, stride_t, stride_b,
                            (unsigned)(reinterpret_cast<uintptr_t>(x) & 15), (unsigned)(reinterpret_cast<uintptr_t>(grad) & 15),
                            p.grad != nullptr, gamma != nullptr, label_smoothing >= 0.f,
                            gamma ? 0 : device_cus(),        // (per device: a process may drive several; the posteriors' plan
                                                             // does not read it, and refuses a shape before any HIP call)
                            sw};
    return noblank_launch(noblank_plan(q), x_dtype, p, static_cast<hipStream_t>(stream));
}

// the grid of the two scale kernels: in the common case (grad_out == 1) every block only reads one float and leaves: the
// launch costs one kernel boundary, 1.7 us in a graph, for any grid up to 2048 blocks (tools/scale_grad_time.py: 64
// blocks 1.68, 1024 blocks 1.72 us).  When the gradient must be scaled -- `(loss / accum_steps).backward()`, a loss
// scaler -- the grid is what moves the 2 x 24 MB of config 2: 64 blocks 17.7 us, 256 blocks 7.8, 1024 blocks 5.9
// (round 3; it was 64).
static dim3 scale_grad_grid(size_t n)
{
    size_t blocks = (n / 4 + 255) / 256;
    static const int cap = diag_env("CTC_AMD_SCALE_BLOCKS", 1024);
    if (blocks > (size_t)cap) blocks = cap;
    if (blocks < 1) blocks = 1;
    return dim3((unsigned)blocks);
}

}  // namespace ctc

using namespace ctc;

extern "C" int ctc_amd_noblank_loss_grad(const float *x, int64_t stride_t, int64_t stride_b,
                                         const void *labels, int labels_i64,
                                         const int64_t *in_len, const int64_t *tgt_len,
                                         int T, int B, int C, int S,
                                         float loss_scale, float grad_scale,
                                         float *nll, float *loss, float *grad,
                                         void *workspace, void *stream)
{
    return noblank_run(x, stride_t, stride_b, labels, labels_i64, in_len, tgt_len, T, B, C, S, loss_scale, grad_scale,
                       nll, loss, grad, workspace, stream, -1.f);
}

extern "C" int ctc_amd_noblank_smoothed_loss_grad(const float *x, int64_t stride_t, int64_t stride_b,
                                                  const void *labels, int labels_i64,
                                                  const int64_t *in_len, const int64_t *tgt_len,
                                                  int T, int B, int C, int S, float label_smoothing,
                                                  float loss_scale, float grad_scale,
                                                  float *nll, float *loss, float *grad,
                                                  void *workspace, void *stream)
{
    if (!(label_smoothing >= 0.f && label_smoothing <= 1.f)) return CTC_AMD_ERR_BAD_ARGUMENT;
    return noblank_run(x, stride_t, stride_b, labels, labels_i64, in_len, tgt_len, T, B, C, S, loss_scale, grad_scale,
                       nll, loss, grad, workspace, stream, label_smoothing);
}

extern "C" int ctc_amd_scale_grad(float *grad, const float *grad_out, size_t n, void *stream)
{
    if (!grad || !grad_out) return CTC_AMD_ERR_BAD_ARGUMENT;
    if (n == 0) return 0;
    if (fold_scale_grad(static_cast<hipStream_t>(stream), grad, CTC_AMD_F32, grad_out, n)) return 0;
    hipLaunchKernelGGL(scale_grad_kernel, scale_grad_grid(n), dim3(256), 0,
                       static_cast<hipStream_t>(stream), grad, grad_out, n);
    return (int)hipGetLastError();
}

extern "C" int ctc_amd_noblank_loss_grad_typed(const void *x, int x_dtype, int64_t stride_t, int64_t stride_b,
                                               const void *labels, int labels_i64,
                                               const int64_t *in_len, const int64_t *tgt_len,
                                               int T, int B, int C, int S, float label_smoothing,
                                               float loss_scale, float grad_scale,
                                               float *nll, float *loss, void *grad,
                                               void *workspace, void *stream)
{
    if (x_dtype != CTC_AMD_F32 && x_dtype != CTC_AMD_BF16 && x_dtype != CTC_AMD_F16) return CTC_AMD_ERR_BAD_ARGUMENT;
    if (label_smoothing != label_smoothing || label_smoothing > 1.f) return CTC_AMD_ERR_BAD_ARGUMENT;
    return noblank_run(x, stride_t, stride_b, labels, labels_i64, in_len, tgt_len, T, B, C, S, loss_scale, grad_scale,
                       nll, loss, grad, workspace, stream, label_smoothing < 0.f ? -1.f : label_smoothing, x_dtype);
}

extern "C" int ctc_amd_scale_grad_typed(void *grad, int dtype, const float *grad_out, size_t n, void *stream)
{
    if (dtype == CTC_AMD_F32) return ctc_amd_scale_grad(static_cast<float *>(grad), grad_out, n, stream);
    if ((dtype != CTC_AMD_BF16 && dtype != CTC_AMD_F16) || !grad || !grad_out) return CTC_AMD_ERR_BAD_ARGUMENT;
    if (n == 0) return 0;
    if (fold_scale_grad(static_cast<hipStream_t>(stream), grad, dtype, grad_out, n)) return 0;
    if (dtype == CTC_AMD_BF16)
        hipLaunchKernelGGL(scale_grad_lowp_kernel<__bf16>, scale_grad_grid(n), dim3(256), 0,
                           static_cast<hipStream_t>(stream), static_cast<__bf16 *>(grad), grad_out, n);
    else
        hipLaunchKernelGGL(scale_grad_lowp_kernel<_Float16>, scale_grad_grid(n), dim3(256), 0,
                           static_cast<hipStream_t>(stream), static_cast<_Float16 *>(grad), grad_out, n);
    return (int)hipGetLastError();
}

extern "C" int ctc_amd_noblank_posteriors(const float *x, int64_t stride_t, int64_t stride_b,
                                          const void *labels, int labels_i64,
                                          const int64_t *in_len, const int64_t *tgt_len,
                                          int T, int B, int C, int S,
                                          float *nll, float *gamma,
                                          void *workspace, void *stream)
{
    if (!gamma) return CTC_AMD_ERR_BAD_ARGUMENT;
    return noblank_run(x, stride_t, stride_b, labels, labels_i64, in_len, tgt_len, T, B, C, S, 0.f, 0.f, nll, nullptr,
                       nullptr, workspace, stream, -1.f, CTC_AMD_F32, gamma);
}

// The same on logits of x_dtype (CTC_AMD_F32: the entry above).  2-byte logits: the r16 kernel's shape domain only, as for
// ctc_amd_noblank_loss_grad_typed; CTC_AMD_ERR_UNSUPPORTED_SHAPE outside it.
extern "C" int ctc_amd_noblank_posteriors_typed(const void *x, int x_dtype, int64_t stride_t, int64_t stride_b,
                                                const void *labels, int labels_i64,
                                                const int64_t *in_len, const int64_t *tgt_len,
                                                int T, int B, int C, int S,
                                                float *nll, float *gamma,
                                                void *workspace, void *stream)
{
    if (x_dtype != CTC_AMD_F32 && x_dtype != CTC_AMD_BF16 && x_dtype != CTC_AMD_F16) return CTC_AMD_ERR_BAD_ARGUMENT;
    if (!gamma) return CTC_AMD_ERR_BAD_ARGUMENT;
    return noblank_run(x, stride_t, stride_b, labels, labels_i64, in_len, tgt_len, T, B, C, S, 0.f, 0.f, nll, nullptr,
                       nullptr, workspace, stream, -1.f, x_dtype, gamma);
}

#ifdef CTC_AMD_DIAGNOSTICS
// Diagnostic entry point (tests/test_scale_fold_gpu.py), not part of include/ctc_amd.h: how many scale_grad calls were
// folded into a captured loss launch / met a remembered launch under capture and were refused, since the library was loaded.
extern "C" int ctc_amd_debug_scale_folds(unsigned *taken, unsigned *refused)
{
    if (!taken || !refused) return CTC_AMD_ERR_BAD_ARGUMENT;
    *taken = ctc::fold_table().taken.load(std::memory_order_relaxed);
    *refused = ctc::fold_table().refused.load(std::memory_order_relaxed);
    return 0;
}

// Diagnostic entry point (tools/chain_probe.py), not part of include/ctc_amd.h: the lattice chains of
// noblank_r16.hpp alone, every emission row pre-published; out[0], out[1] = shader cycles of the
// alpha / beta chain.
extern "C" int ctc_amd_debug_chain_probe(int T, int SP, int waves_alive, int grid, void *out, void *stream, int mode,
                                         int chain_b)
{
    using namespace ctc;
    NoblankParams p = {};
    p.T = T; p.SP = SP; p.S = SP; p.B = grid; p.C = 32;
    p.stop = -77;                                            // the chains also time their main loop: out[8], out[9]
    p.counter = reinterpret_cast<unsigned *>(static_cast<unsigned long long *>(out) + 8);
    const size_t smem = r16_smem_bytes(T, SP, 158);
    return launch<r16_chain_probe_kernel>(dim3(grid), dim3(kThreads), smem, static_cast<hipStream_t>(stream), p,
                                          static_cast<unsigned long long *>(out), waves_alive, mode, chain_b);
}

// Diagnostic entry point (tests/test_noblank_plan.py), not part of include/ctc_amd.h: noblank_plan() for a call with
// these properties, no device touched.  switches: bit 0 CTC_AMD_NOPIPE, 1 _NOXR, 2 _NOR16, 3 _NOPS, 4 _KM.
// out[0..12] = family (NoblankFamily), n4, n2, nt, ps, ch, dual, K, glb, grid, LDS bytes, next_round, koff.
extern "C" int ctc_amd_debug_noblank_plan(int T, int B, int C, int S, int dtype, int64_t stride_t, int64_t stride_b,
                                          unsigned x_low, unsigned grad_low, int want_grad, int want_gamma, int smooth,
                                          int cus, int switches, int64_t *out)
{
    if (!out || T < 1 || B < 1 || C < 1 || S < 1) return CTC_AMD_ERR_BAD_ARGUMENT;
    const NoblankSwitches sw = {(switches & 1) != 0, (switches & 2) != 0, (switches & 4) != 0, (switches & 8) != 0,
                                (switches & 16) != 0, false, 0};
    const NoblankPlan pl = noblank_plan({T, B, C, S, dtype, stride_t, stride_b, x_low, grad_low, want_grad != 0,
                                         want_gamma != 0, smooth != 0, cus, sw});
    const int64_t v[13] = {pl.family, pl.n4, pl.n2, pl.nt, pl.ps, pl.ch, pl.dual, pl.K, pl.glb, pl.grid,
                           (int64_t)pl.lds, pl.next_round, pl.koff};
    for (int i = 0; i < 13; ++i) out[i] = v[i];
    return 0;
}
#endif
