// launch_common.h — host side of every translation unit that launches kernels: the one HIP_TRY, the one s5_trace, option tables, the
// per-device facts, and what the units of the press path (encode_kernels.hip, decode_kernels.hip, batch_kernels.hip, order_launch.hip) call
// of each other.  Host only: nothing here is device code.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include <atomic>
#include <mutex>

#include "../../include/slow5gpu.h"

extern "C" void s5gpu_set_error(const char *fmt, ...);
extern uint32_t s5host_generation;                    // host_api.hip: bumped by s5gpu_shutdown

#define HIP_TRY(x)                                                                                   \
    do {                                                                                             \
        hipError_t e_ = (x);                                                                         \
        if (e_ != hipSuccess) {                                                                      \
            s5gpu_set_error("%s failed: %s (%s:%d)", #x, hipGetErrorString(e_), __FILE__, __LINE__); \
            return S5GPU_ERR_HIP;                                                                    \
        }                                                                                            \
    } while (0)

// S5GPU_TRACE=1 (tools): milliseconds since the calling thread's previous trace point in this translation unit, to stderr — where a call's time goes
static inline void s5_trace(const char *what) {
    static int on = -1;
    if (on < 0) { const char *e = getenv("S5GPU_TRACE"); on = e && atoi(e) ? 1 : 0; }
    if (!on) return;
    static thread_local double last = 0;
    struct timespec t;
    clock_gettime(CLOCK_MONOTONIC, &t);
    const double now = (double)t.tv_sec + 1e-9 * (double)t.tv_nsec;
    fprintf(stderr, "s5gpu[trace] %p +%8.3f ms  %s\n", (void *)&last, last ? 1e3 * (now - last) : 0.0, what);
    last = now;
}

// A unit's options: values lo .. hi are taken, and the bits of `keep` kept.  S5GPU_ERR_ARG: not this table's key, or a value out of range
// (s5gpu_set_option then asks the next unit, and calls the key unknown when nobody takes it).
struct S5Option { const char *name; uint32_t *var; long lo, hi; uint32_t keep; };
template <size_t N>
static inline int s5_set_option(const S5Option (&table)[N], const char *key, long value) {
    for (const S5Option &o : table)
        if (key && strcmp(key, o.name) == 0 && value >= o.lo && value <= o.hi) { *o.var = (uint32_t)value & o.keep; return S5GPU_OK; }
    return S5GPU_ERR_ARG;
}

#pragma GCC visibility push(hidden)   // what follows is the library's own: not exported
// What is known about a device, per ordinal; found out by the first call that needs it there (the batch API runs host threads on several
// devices at once: atomics, and two threads that find out the same thing at the same time do no harm).  An ordinal past the table has no
// record and is served uncached: asked every time, never taken for another device.  (batch_kernels.hip)
constexpr int DEV_MAX = 64;
struct DeviceFacts {
    std::atomic<bool> enc_attrs{false}, dec_attrs{false};   // hipFuncAttributeMaxDynamicSharedMemorySize is set on every kernel of the encode / decode unit's tables
    std::atomic<int> cus{0};               // compute units
    std::atomic<uint32_t> np_resident[6];  // workgroups the device holds at once, per no-payload decode variant (np_kernel); 0 = not asked yet
};
DeviceFacts *device_facts();               // the current device's, or nullptr
int device_cus(int *cus);                  // (<= 0 where the runtime does not say: not kept)
constexpr int LDS_MAX = 160 * 1024 - 256;  // the attribute's value

// each unit of the press path: its options, and warm() = its code object loaded on the current device (s5gpu_warmup)
namespace enck { int set_option(const char *key, long value); int warm(); }   // encode_kernels.hip
namespace deck { int set_option(const char *key, long value); int warm(); }   // decode_kernels.hip
namespace ordk { int set_option(const char *key, long value); int warm(); }   // order_launch.hip

// order_launch.hip — the length-ordered launch lists (order_dev.h).  *out = nullptr when no list is wanted or none can be had (no scratch:
// file order is always correct).  `hold` keeps the device's pool locked until the caller has enqueued the kernels that read the list: two
// threads that share a stream (the default stream, say) must not interleave "build my list" / "build yours" / "read mine".
// The decode side's launch order: batches of at least order_min records (want_order = false: no list at all).  `extra_words` more words of
// the same scratch (16-byte aligned, behind the list) come back in *extra — the zstd decoders' weights pass; handed out with or without a list.
int s5kern_decode_order(const s5gpu_decode_args_t *a, hipStream_t st, const uint32_t **out, std::unique_lock<std::mutex> &hold,
                        size_t extra_words = 0, uint32_t **extra = nullptr, bool want_order = true);
// ... the routed inflate's: always built, the records of >= 32 KiB in front (ROUTE_LONG_BUCKET)
int s5kern_routed_order(const s5gpu_decode_args_t *a, hipStream_t st, const uint32_t **out, std::unique_lock<std::mutex> &hold);
// ... the encode side's: the overflow list of a mixed batch (how many reads are on it is only known on the device: the grids cover n_reads)
int s5kern_encode_order(const s5gpu_encode_args_t *a, hipStream_t st, const uint32_t **out, std::unique_lock<std::mutex> &hold);
#pragma GCC visibility pop
