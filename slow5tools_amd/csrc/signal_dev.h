// signal_dev.h — what signal_kernels.hip and signal_api.hip share: where the kernels find a record's signal slot, and the launchers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/slow5gpu.h"

namespace sigk {

// Per-record sig_off (u64) and sig_cap (u32) at a byte stride: plain arrays (the public *_dev calls) or the decoder's own s5gpu_rec_desc_t
// table where it already sits on the device (s5gpu_signal_stats_stream).
struct SigRecs {
    const int16_t *sig;
    const uint8_t *off, *cap;
    const s5gpu_rec_fields_t *fields;
    uint32_t off_stride, cap_stride, n;
#ifdef __HIPCC__
    __device__ __forceinline__ uint64_t o(uint32_t i) const { return *(const uint64_t *)(off + (uint64_t)i * off_stride); }
    // the ONLY sample count a kernel may use: 0 for a failed record (status 6 leaves the count it needed in n_samples), never past the slot
    __device__ __forceinline__ uint32_t n_eff(uint32_t i, int32_t *status) const {
        const int32_t st = fields[i].status;
        const uint32_t ns = fields[i].n_samples, c = *(const uint32_t *)(cap + (uint64_t)i * cap_stride);
        *status = st;
        return st == 0 ? (ns < c ? ns : c) : 0u;
    }
#endif
};

struct Quantiles { uint32_t n; double q[4]; };

struct WinArgs {
    const s5gpu_sig_stats_t *stats;
    const uint32_t *win_read, *win_start;
    int32_t *win_status;
    void *out;
    uint32_t n_windows, W;
    int mode;
    double a, b;
};

int launch_stats(const SigRecs &R, const Quantiles &Q, s5gpu_sig_stats_t *stats, hipStream_t st);
int launch_windows(const SigRecs &R, const WinArgs &A, int dtype, hipStream_t st);

}  // namespace sigk
