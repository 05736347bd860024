// Host-side launch helper for the C-ABI entry points (no allocation, no sync).
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdlib>
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

}  // namespace ctc
