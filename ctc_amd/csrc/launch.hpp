// Host-side launch helper for the C-ABI entry points (no allocation, no sync).
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <type_traits>

#include "../../include/ctc_amd.h"

namespace ctc {

constexpr size_t kMaxLds = 160 * 1024;        // LDS per CU on gfx950
constexpr size_t kDefaultDynLds = 64 * 1024;  // above this the attribute must be raised
constexpr int kMaxDevices = 64;               // per-device caches below are indexed by the HIP device ordinal

// Do the [T][B][C] logits and their gradient, `bytes` per element for the two together, stay within the memory-side
// cache (256 MB)?  Then the gradient is stored write-through; beyond it, with non-temporal stores.
inline bool within_memory_side_cache(size_t bytes, int T, int B, int C) { return bytes * T * B * C <= ((size_t)230 << 20); }

// ordinal of the calling thread's current device, or -1 (then nothing is cached)
inline int current_device()
{
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) return -1;
    return dev;
}

// compute units of the current device (cached per device: a process may drive several GPUs)
inline int device_cus()
{
    static std::atomic<int> cus[kMaxDevices];
    const int dev = current_device();
    if (dev < 0) return 0;
    int n = cus[dev].load(std::memory_order_relaxed);
    if (n == 0) {
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) n = 0;
        cus[dev].store(n, std::memory_order_relaxed);
    }
    return n;
}

// Diagnostic switches (phase stamps, forced kernel choices) exist only in builds made with
// -DCTC_AMD_DIAGNOSTICS (python -m ctc_amd.build --diag -> libctc_amd_diag.so, used by tools/); the
// product library reads none of them.
inline int diag_env(const char *name, int fallback = 0)
{
#ifdef CTC_AMD_DIAGNOSTICS
    const char *v = getenv(name);
    return v ? (v[0] ? atoi(v) : 1) : fallback;
#else
    (void)name;
    return fallback;
#endif
}

// x_dtype of the typed read-out entries -> the element type E of their kernels: f(LogitElem<E>{})
template <typename E> struct LogitElem { using type = E; };
template <typename F>
inline int with_logit_elem(int x_dtype, F f)
{
    switch (x_dtype) {
    case CTC_AMD_F32: return f(LogitElem<float>{});
    case CTC_AMD_BF16: return f(LogitElem<__bf16>{});
    case CTC_AMD_F16: return f(LogitElem<_Float16>{});
    default: return CTC_AMD_ERR_BAD_ARGUMENT;
    }
}

// A run-time number as a template argument: f(std::integral_constant<int, N>()) for N = n if it is one of Ns..., else
// for the last of them.
template <int N, int... Ns, typename F>
inline int with_constant(int n, F f)
{
    if constexpr (sizeof...(Ns) == 0) {
        return f(std::integral_constant<int, N>());
    } else {
        return n == N ? f(std::integral_constant<int, N>()) : with_constant<Ns...>(n, f);
    }
}

template <auto kern, typename... Args>
inline int launch(dim3 grid, dim3 block, size_t smem, hipStream_t stream, Args... args)
{
    if (smem > kDefaultDynLds) {
        // the attribute is sticky per kernel AND per device: one flag per (instantiation, device)
        static std::atomic<bool> granted[kMaxDevices];
        const int dev = current_device();
        if (dev < 0 || !granted[dev].load(std::memory_order_relaxed)) {
            hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kern),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)kMaxLds);
            if (e != hipSuccess) return (int)e;
            if (dev >= 0) granted[dev].store(true, std::memory_order_relaxed);
        }
    }
    hipLaunchKernelGGL(kern, grid, block, smem, stream, args...);
    return (int)hipGetLastError();
}

// ---- a scale_grad call folded into the captured loss launch it scales (include/ctc_amd.h) ----------------
//
// Under stream capture, ctc_amd_scale_grad[_typed] issued DIRECTLY behind a *_loss_grad launch on the same capturing
// stream, for exactly that launch's gradient buffer, adds no node: the loss launch's kernel node gets the grad_out device
// pointer as its `upstream` argument (hipGraphKernelNodeSetParams) and the kernel multiplies by *grad_out as it stores, at
// every replay.  A loss launch that was captured is remembered here, one record per stream, in a small fixed table: no
// allocation, no synchronisation with the device, one mutex.  Everything that does not meet the conditions -- an eager
// call, another node captured in between, another buffer / count / dtype, a kernel family that does not take the
// pointer, a second scale call, any HIP error on the way -- launches the scale kernel as before.
#pragma GCC visibility push(hidden)                          // (host-side helpers: the library exports its C ABI, nothing of this)
constexpr int kFoldRecords = 16;              // streams capturing a loss launch at the same time (beyond: the oldest record goes)
constexpr size_t kFoldParamBytes = 256;       // the largest params struct a record can copy

struct FoldRecord {
    bool live, consumed, foldable;
    hipStream_t stream;
    unsigned long long capture_id;
    hipGraphNode_t node;
    void *func;
    dim3 grid, block;
    unsigned lds;
    alignas(16) unsigned char params[kFoldParamBytes];
    size_t upstream_offset;                   // of `const float *upstream` inside the params copy
    int extra, n_extra;                       // a trailing int kernel argument (binary: the row pitch), if any
    const void *grad;
    size_t n;
    int dtype;
};
struct FoldTable {
    std::mutex lock;
    FoldRecord rec[kFoldRecords];
    unsigned next_victim;
    std::atomic<unsigned> taken, refused;     // since load (ctc_amd_debug_scale_folds, diagnostics build)
};
// (one table for the whole library)
inline FoldTable &fold_table()
{
    static FoldTable t;
    return t;
}

// the node a launch that was just captured on `stream` became: the stream's dependency set, if it is exactly one node
inline bool captured_tail(hipStream_t stream, unsigned long long &id, hipGraphNode_t &node)
{
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    hipGraph_t graph = nullptr;
    const hipGraphNode_t *deps = nullptr;
    size_t ndeps = 0;
    id = 0;
    if (hipStreamGetCaptureInfo_v2(stream, &st, &id, &graph, &deps, &ndeps) != hipSuccess) {
        (void)hipGetLastError();                             // (not sticky: the next launch must not report it)
        return false;
    }
    if (st != hipStreamCaptureStatusActive || ndeps != 1 || !deps) return false;
    node = deps[0];
    return true;
}

// Behind a loss+gradient launch of `kern` with params `p` (and `extra...`: at most one trailing int): remember it if it
// was captured.  `foldable`: the kernel reads p.upstream.
template <auto kern, typename P, typename... Extra>
inline void note_loss_launch(dim3 grid, dim3 block, size_t smem, hipStream_t stream, const P &p, bool foldable,
                             const void *grad, size_t n, int dtype, Extra... extra)
{
    static_assert(sizeof(P) <= kFoldParamBytes && std::is_trivially_copyable<P>::value, "params copy");
    static_assert(sizeof...(Extra) <= 1, "one trailing int at most");
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(stream, &st) != hipSuccess) {
        (void)hipGetLastError();
        return;
    }
    FoldTable &t = fold_table();
    std::lock_guard<std::mutex> guard(t.lock);
    FoldRecord *r = nullptr;
    for (FoldRecord &q : t.rec)
        if (q.live && q.stream == stream) r = &q;
    if (st != hipStreamCaptureStatusActive) {                // an eager launch: whatever was remembered for the stream is stale
        if (r) r->live = false;
        return;
    }
    unsigned long long id;
    hipGraphNode_t node;
    if (!captured_tail(stream, id, node)) {
        if (r) r->live = false;
        return;
    }
    if (!r)
        for (FoldRecord &q : t.rec)
            if (!q.live) { r = &q; break; }
    if (!r) r = &t.rec[t.next_victim++ % kFoldRecords];
    r->live = true; r->consumed = false; r->foldable = foldable;
    r->stream = stream; r->capture_id = id; r->node = node;
    r->func = reinterpret_cast<void *>(kern);
    r->grid = grid; r->block = block; r->lds = (unsigned)smem;
    memcpy(r->params, &p, sizeof(P));
    r->upstream_offset = offsetof(P, upstream);
    r->n_extra = (int)sizeof...(Extra);
    r->extra = 0;
    ((r->extra = extra), ...);
    r->grad = grad; r->n = n; r->dtype = dtype;
}

// ctc_amd_scale_grad[_typed]: true when the call was folded into the loss launch in front of it (nothing to launch)
inline bool fold_scale_grad(hipStream_t stream, const void *grad, int dtype, const float *grad_out, size_t n)
{
    FoldTable &t = fold_table();
    std::lock_guard<std::mutex> guard(t.lock);
    FoldRecord *r = nullptr;
    for (FoldRecord &q : t.rec)
        if (q.live && q.stream == stream) r = &q;
    if (!r) return false;                                    // no captured loss launch on this stream: the ordinary launch
    unsigned long long id;
    hipGraphNode_t node;
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(stream, &st) != hipSuccess) (void)hipGetLastError();
    if (st != hipStreamCaptureStatusActive) {                // the capture is over (an eager call)
        r->live = false;
        return false;
    }
    bool ok = captured_tail(stream, id, node) && id == r->capture_id && node == r->node &&   // nothing captured or joined in behind it
              r->foldable && !r->consumed && grad == r->grad && n == r->n && dtype == r->dtype;
    if (ok) {
        memcpy(r->params + r->upstream_offset, &grad_out, sizeof(grad_out));
        void *args[2] = {r->params, &r->extra};
        hipKernelNodeParams np = {};
        np.func = r->func;
        np.gridDim = r->grid;
        np.blockDim = r->block;
        np.sharedMemBytes = r->lds;
        np.kernelParams = args;
        np.extra = nullptr;
        if (hipGraphKernelNodeSetParams(r->node, &np) != hipSuccess) {
            (void)hipGetLastError();
            const float *none = nullptr;
            memcpy(r->params + r->upstream_offset, &none, sizeof(none));
            ok = false;
        }
    }
    if (ok) {
        r->consumed = true;
        t.taken.fetch_add(1, std::memory_order_relaxed);
    } else {
        t.refused.fetch_add(1, std::memory_order_relaxed);
    }
    return ok;
}

// launch<kern>(..., p, extra...) of a loss+gradient kernel, remembered for a scale_grad call that may follow
template <auto kern, typename P, typename... Extra>
inline int launch_loss(dim3 grid, dim3 block, size_t smem, hipStream_t stream, bool foldable, int dtype, size_t n, const P &p,
                       Extra... extra)
{
    const int rc = launch<kern>(grid, block, smem, stream, p, extra...);
    if (rc == 0 && p.grad) note_loss_launch<kern>(grid, block, smem, stream, p, foldable, p.grad, n, dtype, extra...);
    return rc;
}
#pragma GCC visibility pop

}  // namespace ctc
