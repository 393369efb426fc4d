// digest_dev.h — what digest_kernels.hip, digest_api.hip and order_launch.hip share: the record table k_rec_digest walks, the canonical length of a
// record (the key of its launch order) and the launcher.
//
// The canonical record C(r) (docs/codecs.md §4.12) is never built: it is the virtual stream
//     payload[0, hl)  |  u64 N  |  2N bytes of the record's signal slot  |  payload[aux_off, aux_off + aux_len)         hl = 2 + id_len + 36
// and its digest is XXH64(C(r), seed 0).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <mutex>

#include "../../include/slow5gpu.h"

namespace digk {

// What the full form of s5gpu_decode_dev left on the device.  `payload` and `sig` are 16-byte aligned and both have 16 readable bytes behind
// their last slot: the kernel takes aligned 8-byte words, so it touches a slot rounded out to 16 bytes and nothing else.
struct DigRecs {
    const s5gpu_rec_desc_t *desc;
    const uint8_t *payload;
    const int16_t *sig;
    const s5gpu_rec_fields_t *fields;
    uint32_t n;
};

// The pieces of one record's virtual stream, or ok = false: the record failed to decode, or its fields point outside its own slots (then
// nothing of it is read and its digest is 0).
struct Pieces {
    uint64_t n_samples;     // N
    uint64_t sig_at;        // virtual offset of the first signal byte: hl + 8
    uint64_t aux_at;        // virtual offset of the first aux byte: hl + 8 + 2N
    uint64_t total;         // length of C(r)
    uint32_t hl, aux_off;
    bool ok;
};

#ifdef __HIPCC__
__device__ __forceinline__ Pieces pieces_of(const s5gpu_rec_desc_t &d, const s5gpu_rec_fields_t &f) {
    Pieces P;
    P.ok = false; P.n_samples = 0; P.sig_at = 0; P.aux_at = 0; P.total = 0; P.hl = 0; P.aux_off = 0;
    if (f.status != 0) return P;
    const uint64_t hl = 2ull + f.read_id_len + 36ull;
    if (hl > d.pay_cap || f.n_samples > d.sig_cap || f.aux_off > d.pay_cap || f.aux_len > d.pay_cap - f.aux_off) return P;
    P.ok = true;
    P.hl = (uint32_t)hl; P.aux_off = f.aux_off;
    P.n_samples = f.n_samples;
    P.sig_at = hl + 8;
    P.aux_at = P.sig_at + 2 * P.n_samples;
    P.total = P.aux_at + f.aux_len;
    return P;
}
#endif

// build the launch order (longest canonical record first) in the stream's order scratch and run k_rec_digest; asynchronous on st
int launch_digest(const DigRecs &R, uint64_t *digest, hipStream_t st);

}  // namespace digk

// order_launch.hip: the counting sort of order_dev.h with OrderByCanonLen as its key.  *ord = nullptr: no list (file order).  `hold` keeps the
// scratch until the kernel that reads the list is enqueued.
int s5kern_digest_order(const digk::DigRecs &R, hipStream_t st, const uint32_t **ord, std::unique_lock<std::mutex> &hold);
