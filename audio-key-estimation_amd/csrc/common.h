// Shared host-side helpers of libake_hip.so: error reporting across the C ABI and the
// hipEvent kernel timer used by bench.py's roofline leg.
#pragma once

#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../include/ake_hip.h"

namespace ake {

void set_error(const char* fmt, ...);

#define AKE_HIP_CHECK(expr)                                                                  \
    do {                                                                                     \
        hipError_t _e = (expr);                                                              \
        if (_e != hipSuccess) {                                                              \
            ake::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
            return AKE_ERR_HIP;                                                              \
        }                                                                                    \
    } while (0)

#define AKE_REQUIRE(cond, code, ...)   \
    do {                               \
        if (!(cond)) {                 \
            ake::set_error(__VA_ARGS__); \
            return (code);             \
        }                              \
    } while (0)

// ---- kernel timer -------------------------------------------------------------------------
// When enabled, a ProfScope brackets what is launched while it lives with two hipEvents recorded on the
// launch stream (ake::launch below opens one per launch).  Elapsed times are summed per kernel name by collect().
struct ProfScope {
    ProfScope(const char* name, hipStream_t stream);
    ~ProfScope();
    int slot;
    hipStream_t stream;
};
bool prof_active();

// One-time setup that must happen once PER DEVICE (hipFuncSetAttribute applies to the current device only; a handle may be
// recreated on another GPU of the same process).  Racing threads at worst repeat an idempotent call.
struct DeviceOnce {
    std::atomic<uint64_t> done{0};
    static int dev() { int d = 0; (void)hipGetDevice(&d); return d & 63; }
    bool need() const { return !((done.load(std::memory_order_acquire) >> dev()) & 1); }
    void mark() { done.fetch_or(1ull << dev(), std::memory_order_release); }
};

// Set the dynamic-LDS limit of `kernels` to `bytes` on the current device ...
template <typename... K>
int set_lds_limit(int bytes, K... kernels) {
    for (const void* f : {reinterpret_cast<const void*>(kernels)...})
        AKE_HIP_CHECK(hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    return AKE_OK;
}

// ... and once per device, for a limit that never changes (`once` is the call site's own static).
template <typename... K>
int raise_lds_limit(DeviceOnce& once, int bytes, K... kernels) {
    if (!once.need()) return AKE_OK;
    const int rc = set_lds_limit(bytes, kernels...);
    if (!rc) once.mark();
    return rc;
}

// ---- kernel launch ------------------------------------------------------------------------
// Every kernel of the library is launched through one of these.  A launch the runtime rejects is reported by the call that made it,
// by kernel name and geometry, as AKE_ERR_HIP; the caller returns that code and launches nothing more.  Nothing synchronises.
// launch() brackets the launch with the kernel timer under `name`; launch_untimed() uses `name` for the error text alone.
template <typename... P, typename... A>
int launch_untimed(const char* name, void (*kernel)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t s, const A&... args) {
    hipLaunchKernelGGL(kernel, grid, block, lds, s, static_cast<P>(args)...);
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) return AKE_OK;
    set_error("%s: launch failed: %s (grid %u x %u x %u, block %u x %u x %u, %zu B of dynamic LDS)", name, hipGetErrorString(e), grid.x, grid.y,
              grid.z, block.x, block.y, block.z, lds);
    return AKE_ERR_HIP;
}

template <typename... P, typename... A>
int launch(const char* name, void (*kernel)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t s, const A&... args) {
    ProfScope ps(name, s);
    return launch_untimed(name, kernel, grid, block, lds, s, args...);
}

// one thread per element, 256 to a block
template <typename... P, typename... A>
int launch_flat(const char* name, void (*kernel)(P...), hipStream_t s, long long total, const A&... args) {
    return launch(name, kernel, dim3(static_cast<unsigned>((total + 255) / 256)), dim3(256), 0, s, args...);
}

// LDS-DMA: every lane's 16 bytes at `src` go straight to the LDS, lane i's to byte address lds_dst + 16 i (wave-uniform; of an LDS
// pointer the low 32 bits are the LDS byte address), without passing through registers.  Nothing waits here: the caller places
// vmcnt(0) and its barrier.  Inline asm because hipcc orders every later LDS access behind a builtin LDS-DMA with vmcnt(0) (it cannot
// tell the halves of a double buffer apart), which would serialise load and multiply.  m0 is saved and restored around the request.
__device__ __forceinline__ void lds_dma_16(const uint4* src, unsigned int lds_dst) {
    unsigned int keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(src), "s"(lds_dst) : "memory");
}

// cfg.local of a handle: the --local pooling window, 0 for a clip-level net (pcnet.hip)
int pcnet_local_window(const ake_pcnet* net);

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// Bump allocator over the caller's workspace.
struct Carver {
    char* base;
    size_t off;
    size_t cap;   // 0 = size query only
    explicit Carver(void* b, size_t c) : base(static_cast<char*>(b)), off(0), cap(c) {}
    template <typename T>
    T* take(size_t n) {
        off = align_up(off, 256);
        T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
        off += n * sizeof(T);
        return p;
    }
};

}  // namespace ake
