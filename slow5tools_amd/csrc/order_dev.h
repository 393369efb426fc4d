// order_dev.h — the one counting sort by length behind every length-ordered launch list: 128 buckets, four per octave, longest first.
//
// One wave (or lane) decodes one record, so a batch ends when its longest record does — and a record of 300 k samples takes a wave ~15 ms however
// idle the rest of the device is.  In file order it starts wherever it happens to stand: 262 144 records with the read lengths of a real
// run decode in 23.7 ms, 16.6 ms with the longest first (tools/mixed_lengths.py: the rate per sample of a batch of equal reads).  Four lists
// are built this way, all in the library's per-(device, stream) scratch (order_launch.hip: order_scratch):
//   * the launch order of the wave-per-record decoders (round 3): records by compressed length;
//   * the overflow list of a mixed ENCODE batch (round 4: the reads the staged kernels redo) by number of samples — a 300 k-sample read keeps
//     one workgroup busy for most of a millisecond, and in list order (the order in which the fused kernel's workgroups happened to give
//     up) it starts wherever it stands.  The list holds read indices;
//   * the routing of big zlib batches to the lane and wave kernels (round 1): records by compressed length, the ones of >= 32 KiB in front;
//   * the order in which k_rec_digest takes decoded records: by the length of their canonical form, so that the sixteen records of a wave end together;
//   * the order in which k_sig_events takes decoded reads: by n_eff, a read per lane, so that the 64 reads of a wave end together.
// Scratch layout: ord[0..127] bucket counts, then cursors; ord[ORD_NLONG]: how many items stand in front of the buckets below `long_bucket`
// (0 when the build names none); ord[ORD_FLAG] != 0: one length class, no list (file order is as good); the list from ord[ORD_LIST] on.
#pragma once
#include "dev_common.h"
#include "digest_dev.h"
#include "signal_dev.h"
#include "../../include/slow5gpu.h"

constexpr uint32_t ORD_NLONG = 128, ORD_FLAG = 129, ORD_LIST = 132;
constexpr uint32_t ROUTE_LONG_BUCKET = 15 * 4;   // compressed records of >= 32 KiB

__device__ __forceinline__ uint32_t length_bucket(uint32_t len) {
    if (len < 4) return len;
    const uint32_t hb = 31u - (uint32_t)__clz((int)len);
    return hb * 4 + ((len >> (hb - 2)) & 3u);
}
// item `i` in launch order when there is a list, else `i` itself
__device__ __forceinline__ uint32_t order_at(const uint32_t *ord, uint32_t i) {
    return ord && !ord[ORD_FLAG] ? ord[ORD_LIST + i] : i;
}
// entry `it` of the overflow list, in launch order when there is one
__device__ __forceinline__ uint32_t ovf_at(const uint32_t *ovf, const uint32_t *ord, uint32_t it) {
    return ord && !ord[ORD_FLAG] ? ord[ORD_LIST + it] : ovf[1 + it];
}

// (a translation unit that only READS a list defines S5_ORDER_LIST_ONLY: the sort's kernels below live in order_launch.hip alone)
#ifndef S5_ORDER_LIST_ONLY
// What is sorted: for grid index i, is there an item, which id goes on the list, and how long is it.
struct OrderByInLen {            // the records of a decode batch by compressed length
    const s5gpu_rec_desc_t *desc;
    uint32_t n;
    __device__ __forceinline__ bool item(uint32_t i, uint32_t &id, uint32_t &len) const {
        if (i >= n) return false;
        id = i; len = desc[i].in_len;
        return true;
    }
};
struct OrderByCanonLen {         // the decoded records of a digest batch by the length of their canonical form (a failed record: 0)
    const s5gpu_rec_desc_t *desc;
    const s5gpu_rec_fields_t *fields;
    uint32_t n;
    __device__ __forceinline__ bool item(uint32_t i, uint32_t &id, uint32_t &len) const {
        if (i >= n) return false;
        const digk::Pieces P = digk::pieces_of(desc[i], fields[i]);
        id = i; len = P.total > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)P.total;
        return true;
    }
};
struct OrderBySigLen {           // the decoded reads of an event batch by the samples a kernel may touch (a failed record: 0)
    sigk::SigRecs R;
    __device__ __forceinline__ bool item(uint32_t i, uint32_t &id, uint32_t &len) const {
        if (i >= R.n) return false;
        int32_t st;
        id = i; len = R.n_eff(i, &st);
        return true;
    }
};
struct OrderOvfBySamples {       // the reads on an encode batch's overflow list (ovf[0] of them: only the device knows) by number of samples
    const s5gpu_read_desc_t *desc;
    const uint32_t *ovf;
    __device__ __forceinline__ bool item(uint32_t i, uint32_t &id, uint32_t &len) const {
        if (i >= ovf[0]) return false;
        id = ovf[1 + i]; len = desc[id].n_samples;
        return true;
    }
};

__global__ __launch_bounds__(s5::NT) void k_order_zero(uint32_t *ord) {
    if (threadIdx.x < ORD_LIST) ord[threadIdx.x] = 0;
}
template <class Key>
__global__ __launch_bounds__(s5::NT) void k_order_count(Key key, uint32_t *ord) {   // workgroup histogram in LDS, one global add per bucket in use
    __shared__ uint32_t h[128];
    if (threadIdx.x < 128) h[threadIdx.x] = 0;
    __syncthreads();
    uint32_t id, len;
    if (key.item(blockIdx.x * s5::NT + threadIdx.x, id, len)) atomicAdd(&h[length_bucket(len)], 1u);
    __syncthreads();
    if (threadIdx.x < 128 && h[threadIdx.x]) atomicAdd(&ord[threadIdx.x], h[threadIdx.x]);
}
// one workgroup of 128: thread t owns bucket 127 - t.  long_bucket != 0 (the routed inflate): ord[ORD_NLONG] = everything in front of the
// buckets below long_bucket, and a length class that reaches into the long buckets still gets its list — those records are the wave kernel's
__global__ __launch_bounds__(128) void k_order_scan(uint32_t *ord, uint32_t long_bucket) {
    __shared__ uint32_t ws[2];
    __shared__ uint64_t su[2];
    const uint32_t b = 127u - threadIdx.x;
    const uint32_t c = ord[b];
    const uint32_t incl = s5::wave_incl_add(c);
    if (s5::lane_id() == 63) ws[s5::wave_id()] = incl;
    const uint64_t used = __ballot(c != 0);
    if (s5::lane_id() == 0) su[s5::wave_id()] = used;
    __syncthreads();
    const uint32_t start = incl - c + (s5::wave_id() ? ws[0] : 0u);
    ord[b] = start;                                                     // cursor of the bucket in the descending list
    if (long_bucket && b == long_bucket) ord[ORD_NLONG] = start + c;
    if (threadIdx.x == 0) {
        // su[0] bit i = bucket 127 - i, su[1] bit i = bucket 63 - i: at most three neighbouring buckets in use = one length class
        const int nb = __popcll((unsigned long long)su[0]) + __popcll((unsigned long long)su[1]);
        int first = -1, last = -1;
        for (int t = 0; t < 128; t++) {
            const bool u = ((t < 64 ? su[0] >> t : su[1] >> (t - 64)) & 1ull) != 0;
            if (u) { if (first < 0) first = t; last = t; }
        }
        // (an empty batch: no list for the launch orders; the routed form, which never sees one, says "list" as it always did)
        const bool one_class = nb == 0 ? long_bucket == 0 : last - first <= 2 && (long_bucket == 0 || 127u - (uint32_t)first < long_bucket);
        ord[ORD_FLAG] = one_class ? 1u : 0u;
    }
}
template <class Key>
__global__ __launch_bounds__(s5::NT) void k_order_scatter(Key key, uint32_t *ord) {   // a workgroup reserves one range per bucket
    __shared__ uint32_t h[128], base[128];
    if (ord[ORD_FLAG]) return;
    if (threadIdx.x < 128) h[threadIdx.x] = 0;
    __syncthreads();
    uint32_t id, len, b = 0, rank = 0;                                             // (id, len: only read where item() set them)
    const bool have = key.item(blockIdx.x * s5::NT + threadIdx.x, id, len);
    if (have) { b = length_bucket(len); rank = atomicAdd(&h[b], 1u); }
    __syncthreads();
    if (threadIdx.x < 128 && h[threadIdx.x]) base[threadIdx.x] = atomicAdd(&ord[threadIdx.x], h[threadIdx.x]);
    __syncthreads();
    if (have) ord[ORD_LIST + base[b] + rank] = id;
}
#endif  // S5_ORDER_LIST_ONLY
