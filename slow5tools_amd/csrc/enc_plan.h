// enc_plan.h — the LDS budget rules of the encode launches (encode_kernels.hip, host_api.hip).  Plain C++, no HIP: tests/test_enc_plan.py
// compiles it on its own and compares every rule with its arithmetic restated.
#pragma once
#include <stdint.h>

namespace s5plan {
constexpr int SIG_SVB_ZD = 1, SIG_EX_ZD = 2;   // = S5GPU_SIG_* ...
constexpr uint32_t BLK = 16384;                // ... and = DEFL_BLK, for callers that do not see deflate_dev.h (encode_kernels.hip asserts all three)

// max_payload is a bound: it assumes the worst case per sample (3.25 bytes for svb-zd, 9.5 for ex-zd), real signals take ~1.27 / ~1.06.
// The fused kernels keep room in LDS for 1.55 / 1.30 bytes per sample and a little for the record's head; everything in hundredths.
struct SigRule { uint32_t bound, keep, head; };   // per sample: what the payload bound assumes, what the fused budget keeps; + bytes
inline SigRule sig_rule(int sig_method) {
    return sig_method == SIG_SVB_ZD ? SigRule{325, 155, 128} : sig_method == SIG_EX_ZD ? SigRule{950, 130, 256} : SigRule{100, 100, 0};
}
constexpr uint32_t STAGE_BLOCKS = 4;         // a batch whose reads take more than this many blocks each is "long": none of them can fit a fused budget
constexpr uint32_t NARROW_MAX = 8192;        // fused budgets up to here run the uint32_t break-mask kernels, larger ones the uint64_t ones
constexpr uint32_t BLOB_MAX = 64 * 1024;     // the svb-zd blob kernels' LDS ceiling
constexpr uint32_t MIXED_BUDGET = 8192;      // the fused budget the host layer names for a long batch with enough short reads in it

inline uint32_t round16(uint64_t x) { return (uint32_t)((x + 15) & ~15ull); }

// LDS bytes of the fused kernels' payload buffer: the caller's budget or the rule's, at most the bound and one block, in 16-byte units
inline uint32_t fused_cap(int sig_method, uint32_t max_payload, uint32_t lds_payload_cap, uint32_t blk) {
    const SigRule r = sig_rule(sig_method);
    uint32_t cap = lds_payload_cap ? lds_payload_cap : (uint32_t)((uint64_t)max_payload * r.keep / r.bound) + r.head;
    if (cap > max_payload) cap = max_payload;
    if (cap > blk) cap = blk;
    return round16(cap);
}
// every read certainly longer than any fused budget?  (min payload ~ 1.25 B/sample of a 3.25 B/sample bound)
inline bool batch_is_long(int sig_method, uint32_t max_payload, uint32_t blk) { return (uint64_t)max_payload * 100 / sig_rule(sig_method).bound > (uint64_t)STAGE_BLOCKS * blk; }
// ... then the whole batch is staged (a caller that names an LDS budget knows its batch is mixed: short reads fused, the rest on the overflow list)
inline bool all_staged(int sig_method, uint32_t max_payload, uint32_t lds_payload_cap, uint32_t blk) { return !lds_payload_cap && batch_is_long(sig_method, max_payload, blk); }
// LDS bytes for `group` svb-zd blobs back to back (max_payload is the 3.25 bytes/sample bound)
inline uint32_t svb_blob_cap(uint32_t max_payload, uint32_t lds_payload_cap, uint32_t group) {
    const SigRule r = sig_rule(SIG_SVB_ZD);
    uint64_t cap = lds_payload_cap ? lds_payload_cap : (uint64_t)max_payload * r.keep / r.bound + r.head;
    cap *= group;
    return round16(cap > BLOB_MAX ? BLOB_MAX : cap);
}
inline bool wide(uint32_t cap) { return cap > NARROW_MAX; }
// what a read is expected to take per sample when the host layer counts the reads that fit MIXED_BUDGET (raw samples: their two bytes)
inline double fit_per_sample(int sig_method) { return sig_method == SIG_SVB_ZD || sig_method == SIG_EX_ZD ? sig_rule(sig_method).keep / 100.0 : 2.0; }
}   // namespace s5plan
