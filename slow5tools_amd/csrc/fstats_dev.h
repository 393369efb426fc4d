// fstats_dev.h — what fstats_kernels.hip and fstats_api.hip share: the launchers of the file-wide accumulator and its options.
#pragma once
#include "signal_dev.h"

namespace fsk {

// LDS counters per bin: lane l of a wave adds to copy l & (COPIES - 1), so lanes that meet on one value spread over COPIES adjacent banks
constexpr uint32_t COPIES = 4;
constexpr uint32_t MAX_GRID = 1024;      // workgroups of one launch: four per CU (option "fstats_grid" lowers it: a workgroup then walks several records)
constexpr uint32_t MAX_BINS = 2048;      // COPIES * MAX_BINS u32 counters = 32 KiB of LDS: four workgroups per CU

struct Opts {
    int32_t win_lo;      // bin (sample value + 32768) of the window's low edge; -1: every workgroup centres its window on the data it meets first
    uint32_t bins;       // LDS bins: 0 (every sample goes to global atomics) or a power of two, 64 .. MAX_BINS
    uint32_t flush;      // a workgroup sends its LDS counters to acc->hist before a read would take its samples since the last flush past this
};

int set_option(const char *key, long value);   // "fstats_window_lo", "fstats_lds_bins", "fstats_flush_samples", "fstats_grid"; S5GPU_ERR_ARG: not one of them
int launch_reset(s5gpu_file_stats_t *acc, hipStream_t st);
int launch_accum(const sigk::SigRecs &R, s5gpu_file_stats_t *acc, hipStream_t st);
int launch_add_failed(s5gpu_file_stats_t *acc, uint32_t k, hipStream_t st);   // acc->n_failed += k (records the host dropped from a batch)

}  // namespace fsk

// tools/fstats_time.py's floor (k_read_floor): every whole 16 bytes of p[0, bytes) (device, 16-byte aligned) loaded once, a lane per 16 bytes,
// XOR-folded into *out (device, u32).  A tool hook: exported, but not declared in include/slow5gpu.h.
extern "C" int s5tool_read_floor_dev(const void *p, uint64_t bytes, uint32_t *out, void *stream);
