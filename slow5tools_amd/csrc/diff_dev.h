// diff_dev.h — what diff_kernels.hip and diff_api.hip share: the two decoded batches k_sig_diff reads at once, its options and the launchers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/slow5gpu.h"

namespace dfk {

// LDS counters per bin: lane l of a wave adds to copy l & (COPIES - 1).  Differences sit on a handful of values (nine after `degrade -b 3`), so
// without the copies nearly every lane of a wave would meet on the same few counters; with 32 at most two lanes of a wave share one.
constexpr uint32_t COPIES = 32;
constexpr uint32_t MAX_GRID = 1024;      // workgroups of one launch: four per CU (option "diff_grid" lowers it: a workgroup then walks several pairs)
constexpr uint32_t MIN_BINS = 8, MAX_BINS = 256, DEFAULT_BINS = 64;   // COPIES * MAX_BINS u32 counters = 32 KiB of LDS
constexpr uint32_t ZERO_BIN = 65535;     // acc->hist[d + ZERO_BIN]

// One decoded batch: per-record sig_off (u64), sig_cap (u32), pay_off (u64) and pay_cap (u32) at a byte stride, so that plain arrays (the public
// call) and the decoder's own s5gpu_rec_desc_t table (the handle) are read by the same kernel.
struct Side {
    const int16_t *sig;
    const uint8_t *off, *cap;
    const s5gpu_rec_fields_t *fields;
    const uint8_t *payload;              // NULL: ID and AUX are not compared, poff / pcap are not read
    const uint8_t *poff, *pcap;
    uint32_t off_stride, cap_stride, poff_stride, pcap_stride, n;
#ifdef __HIPCC__
    __device__ __forceinline__ uint64_t o(uint32_t i) const { return *(const uint64_t *)(off + (uint64_t)i * off_stride); }
    __device__ __forceinline__ uint64_t po(uint32_t i) const { return *(const uint64_t *)(poff + (uint64_t)i * poff_stride); }
    __device__ __forceinline__ uint32_t pc(uint32_t i) const { return *(const uint32_t *)(pcap + (uint64_t)i * pcap_stride); }
    // the ONLY sample count the kernel may use (docs/codecs.md §4.11): 0 for a failed record, never past the slot
    __device__ __forceinline__ uint32_t n_eff(uint32_t i, int32_t *status) const {
        const int32_t st = fields[i].status;
        const uint32_t ns = fields[i].n_samples, c = *(const uint32_t *)(cap + (uint64_t)i * cap_stride);
        *status = st;
        return st == 0 ? (ns < c ? ns : c) : 0u;
    }
#endif
};

struct Opts {
    uint32_t bins;       // LDS bins of the window [-bins / 2, bins / 2): 0 or a power of two, MIN_BINS .. MAX_BINS
    uint32_t flush;      // a workgroup sends its LDS counters to acc->hist before a pair would take its samples since the last flush past this
};

int set_option(const char *key, long value);   // "diff_lds_bins", "diff_flush_samples", "diff_grid"; S5GPU_ERR_ARG: not one of them
int launch_reset(s5gpu_diff_acc_t *acc, hipStream_t st);
int launch_diff(uint32_t n_pairs, const uint32_t *pair_a, const uint32_t *pair_b, const Side &A, const Side &B, s5gpu_sig_diff_t *out,
                s5gpu_diff_acc_t *acc, hipStream_t st);
int launch_add_failed(s5gpu_diff_acc_t *acc, uint32_t k, hipStream_t st);   // acc->n_pairs, n_failed += k (pairs with a record the host dropped)

}  // namespace dfk
