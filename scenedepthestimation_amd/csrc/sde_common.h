// Shared helpers for the libsde HIP sources (gfx950 / CDNA4 only).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>
#include <type_traits>

#include "sde.h"

#define SDE_EXPORT extern "C" __attribute__((visibility("default")))

namespace sde {

static inline hipStream_t as_stream(void *s) { return reinterpret_cast<hipStream_t>(s); }

static inline int launch_status()
{
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? SDE_OK : SDE_ERR_LAUNCH;
}

static inline int cdiv(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }

// Per-device one-time setup (kernel attributes such as the >64 KB dynamic-LDS opt-in are per
// device): `done` holds one bit per device id; the first caller on a device runs `fn` and
// publishes the bit.  Concurrent first calls may both run `fn`, which is idempotent.  A callback
// returning bool publishes the bit only on success (a failed setup is retried by the next call,
// and every call returns whether the setup holds); a void callback always publishes.
template <typename F>
static inline bool once_per_device(std::atomic<uint64_t> &done, F fn)
{
    constexpr bool checked = std::is_same<decltype(fn()), bool>::value;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) {
        if constexpr (checked) return fn();
        fn();
        return true;
    }
    const uint64_t bit = 1ull << dev;
    if (done.load(std::memory_order_acquire) & bit) return true;
    bool ok = true;
    if constexpr (checked) ok = fn();
    else fn();
    if (ok) done.fetch_or(bit, std::memory_order_acq_rel);
    return ok;
}

// Launch kernel K with smem <= MAX bytes of dynamic LDS.  More than 64 KB needs a per-device opt-in on the
// kernel: it is made here (for MAX bytes), on K's first launch on a device whatever that launch's size, so no
// instantiation can be launched without it.  (The function-local atomic is trivially destructible: no
// exit-time code.)
template <auto K, size_t MAX, typename... Args>
static inline void launch_lds_dyn(dim3 grid, dim3 block, size_t smem, hipStream_t st, Args... args)
{
    static std::atomic<uint64_t> done{0};
    once_per_device(done, [] {
        (void)hipFuncSetAttribute((const void *)K, hipFuncAttributeMaxDynamicSharedMemorySize, (int)MAX);
    });
    hipLaunchKernelGGL(K, grid, block, smem, st, args...);
}

// ... with a compile-time size
template <auto K, size_t SMEM, typename... Args>
static inline void launch_lds(dim3 grid, dim3 block, hipStream_t st, Args... args)
{
    launch_lds_dyn<K, SMEM>(grid, block, SMEM, st, args...);
}

// CU count of the current device, cached per device id (256 when the runtime does not say).
static inline int device_cus()
{
    static std::atomic<int> cached[64];
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
    if (const int c = cached[dev].load(std::memory_order_relaxed)) return c;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
    cached[dev].store(n, std::memory_order_relaxed);
    return n;
}

// Buffer descriptor (wave-uniform inputs only) for raw buffer loads/stores with a 32-bit per-lane voffset, an
// SGPR soffset and the hardware range check on voffset (>= bytes: load 0, store dropped).  Every range in
// use is < 2^31, so a voffset of BUF_OOB is out of every range: no exec-mask branch around an edge lane.
constexpr uint32_t BUF_OOB = 0x80000000u;
__device__ __forceinline__ __amdgpu_buffer_rsrc_t buf_rsrc(const void *base, uint32_t bytes)
{
    const uintptr_t b = (uintptr_t)base;
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)b);
    const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(b >> 32));
    return __builtin_amdgcn_make_buffer_rsrc((void *)(((uintptr_t)hi << 32) | lo), 0,
                                             (int)__builtin_amdgcn_readfirstlane(bytes), 0x00020000);
}

__device__ __forceinline__ bool finite_f32(float v) { return (__float_as_uint(v) & 0x7fffffffu) < 0x7f800000u; }

// Logical id of block b of nb, so that the blocks one XCD runs share its L2 on neighbouring work.
__device__ __forceinline__ int xcd_remap(int b, int nb)
{
    // bijective: blocks b, b+8, ... (one XCD under round-robin dispatch) get consecutive logical ids
    const int q = nb / 8, r = nb % 8, x = b % 8;
    return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + b / 8;
}

// NumPy float32 pairwise sum of elementwise products, 0.0f + pairwise(a*b)
// (numpy loops_utils.h.src pairwise_sum; add.reduce identity 0.0).  Products
// and sums are separately rounded: the library is built with -ffp-contract=off.
__device__ static float pw_prod_rec(const float *a, const float *b, int n)
{
    if (n < 8) {
        float res = 0.0f;
        for (int i = 0; i < n; i++) res += a[i] * b[i];
        return res;
    }
    if (n <= 128) {
        float r[8];
#pragma unroll
        for (int j = 0; j < 8; j++) r[j] = a[j] * b[j];
        int i = 8;
        for (; i < n - (n % 8); i += 8) {
#pragma unroll
            for (int j = 0; j < 8; j++) r[j] += a[i + j] * b[i + j];
        }
        float res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
        for (; i < n; i++) res += a[i] * b[i];
        return res;
    }
    int n2 = n / 2;
    n2 -= n2 % 8;
    return pw_prod_rec(a, b, n2) + pw_prod_rec(a + n2, b + n2, n - n2);
}

__device__ __forceinline__ float np_neg_dot(const float *a, const float *b, int n)
{
    float s = 0.0f + pw_prod_rec(a, b, n);
    return -s;
}

// First-min merge: b replaces a iff it is strictly smaller, or equal with a lower
// index -- the sequential `v < best` scan's answer for any split of the d range.
__device__ __forceinline__ void argmin_merge(float &ma, int &aa, float mb, int ab)
{
    if (mb < ma || (mb == ma && ab < aa)) {
        ma = mb;
        aa = ab;
    }
}

}  // namespace sde
