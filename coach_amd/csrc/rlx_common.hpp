// Shared host-side plumbing for librlx.so (gfx950 only — no dual backend).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <cstdint>
#include <mutex>
#include "../../include/rlx.h"

namespace rlx {

void set_error(const char *fmt, ...);

inline hipStream_t as_stream(void *s) { return reinterpret_cast<hipStream_t>(s); }

// Number of CUs on MI355X; grids for streaming kernels are capped at CUS*8 blocks
// (cdna_hip_programming.md G11) and grid-stride the rest.
constexpr int kCUs = 256;
constexpr int kMaxStreamBlocks = kCUs * 8;

inline int grid_for(long long work_items, int block, int cap = kMaxStreamBlocks) {
    long long g = (work_items + block - 1) / block;
    if (g < 1) g = 1;
    if (g > cap) g = cap;
    return (int)g;
}


// In-process kernel timer (rlx_profile_*): while it is armed every launch of this library goes out through
// hipExtLaunchKernel with a private (start, stop) event pair, which the runtime fills from the dispatch packet's own
// begin / end timestamps — the duration a kernel trace (rocprofv3 --kernel-trace) reports for that dispatch, taken
// in situ: same stream, same neighbours, operands as the previous kernel left them.  Eager launches only (an armed
// timer inside a stream capture is refused by rlx_profile_begin's caller contract: the events are not graph nodes).
struct Profiler {
    bool active = false;
    int n = 0, cap = 0;         // records taken / allocated event pairs
    int limit = 0, dropped = 0; // max_records of the armed trace / launches that found it full (rlx_profile_end fails)
    hipEvent_t *start = nullptr, *stop = nullptr;
    const char **name = nullptr;
};
extern Profiler g_prof;

template <typename F, typename... Args>
inline void launch(const char *name, F kernel, dim3 grid, dim3 block, unsigned shmem, hipStream_t s,
                   Args... args) {
    if (g_prof.active && g_prof.n < g_prof.limit) {
        const int i = g_prof.n++;
        g_prof.name[i] = name;
        hipExtLaunchKernelGGL(kernel, grid, block, shmem, s, g_prof.start[i], g_prof.stop[i], 0, args...);
    } else {
        if (g_prof.active) ++g_prof.dropped;
        kernel<<<grid, block, shmem, s>>>(args...);
    }
}

// Lets kKernel be launched with `bytes` of dynamic LDS (above the 64 KB a kernel gets without asking), on the CURRENT
// device: the attribute belongs to the device, so the largest value set is remembered per device, and a launch on a
// second GPU sets it there too.  Two threads may both make a first launch: the mutex keeps the value remembered equal to
// the value set; later calls only read.  A larger `bytes` raises the value (mlp_fused.hip's LDS depends on the layer sizes).
constexpr int kMaxDevices = 64;
template <auto kKernel>
inline hipError_t allow_lds(size_t bytes) {
    static std::atomic<size_t> allowed[kMaxDevices];
    static std::mutex first_launch;
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    std::atomic<size_t> *seen = dev >= 0 && dev < kMaxDevices ? &allowed[dev] : nullptr;      // beyond the table: set every time
    if (seen && bytes <= seen->load(std::memory_order_acquire)) return hipSuccess;
    std::lock_guard<std::mutex> lock(first_launch);
    if (seen && bytes <= seen->load(std::memory_order_relaxed)) return hipSuccess;
    e = hipFuncSetAttribute(reinterpret_cast<const void *>(kKernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e == hipSuccess && seen) seen->store(bytes, std::memory_order_release);
    return e;
}

// np.clip(x, lo, hi) = np.minimum(np.maximum(x, lo), hi) as numpy evaluates it: x is kept where it is a NaN or strictly
// inside the bound, the bound is taken otherwise -- a NaN x stays NaN (fmin / fmax return the bound and hide a diverged
// network behind a legal value) and a NaN bound comes through.  x inside [lo, hi] keeps its bits.
__device__ __forceinline__ double np_clip(double x, double lo, double hi) {
    x = (x > lo || x != x) ? x : lo;
    return (x < hi || x != x) ? x : hi;
}

// np.minimum(a, b) over the twin Q streams as a SELECTION (the value and the gradient of the minimum go to one side): a
// where a <= b -- a tie goes to a, tf.minimum's gradient rule -- or where a is a NaN, b otherwise.  A NaN of either stream
// comes through (`a <= b ? a : b` alone returned b for a NaN a); NaN-free inputs select as before.
__device__ __forceinline__ bool np_min_takes_first(float a, float b) { return a <= b || a != a; }

// One step of np.argmax over a row: the FIRST maximum wins and a NaN counts as the maximum, so the first NaN of a row
// wins and nothing after it is looked at (argmax_rows_kernel, explore.hip).  bv / best: the running maximum and its index.
__device__ __forceinline__ void np_argmax_step(float v, int a, float &bv, int &best) {
    if (bv == bv && (v > bv || v != v)) {
        bv = v;
        best = a;
    }
}
}  // namespace rlx

#define RLX_REQUIRE(cond, ...)                      \
    do {                                            \
        if (!(cond)) {                              \
            rlx::set_error(__VA_ARGS__);            \
            return RLX_ERR_INVALID_ARG;             \
        }                                           \
    } while (0)

#define RLX_HIP(call)                                                              \
    do {                                                                           \
        hipError_t e__ = (call);                                                   \
        if (e__ != hipSuccess) {                                                   \
            rlx::set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(e__), \
                           __FILE__, __LINE__);                                    \
            return RLX_ERR_HIP;                                                    \
        }                                                                          \
    } while (0)

// After a kernel launch: surfaces launch-configuration errors without syncing.
#define RLX_LAUNCH_CHECK()                                                              \
    do {                                                                                \
        hipError_t e__ = hipGetLastError();                                             \
        if (e__ != hipSuccess) {                                                        \
            rlx::set_error("kernel launch failed: %s (%s:%d)", hipGetErrorString(e__),  \
                           __FILE__, __LINE__);                                         \
            return RLX_ERR_HIP;                                                         \
        }                                                                               \
    } while (0)

// Every kernel of the library is launched through this (see rlx::launch): `kernel` in parentheses, so that template
// argument lists with commas stay one macro argument.
#define RLX_LAUNCH(kernel, grid, block, shmem, stream, ...) \
    rlx::launch(#kernel, kernel, grid, block, shmem, stream, ##__VA_ARGS__)
