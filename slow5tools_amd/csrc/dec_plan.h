// dec_plan.h — the launch rules of the decode half of the press path (decode_kernels.hip, order_launch.hip, host_api.hip): every decision that
// launch_inflate, s5gpu_decode_dev, s5gpu_decode_scratch_bytes and the host layer's decode_np_framed take from numbers.  Plain C++, no HIP and
// no state (option values are parameters): tests/test_dec_plan.py compiles it on its own and compares every rule with its arithmetic restated.
#pragma once
#include <stdint.h>

#include "enc_plan.h"

// waves per SIMD the parallel inflate kernels are budgeted for (their launch bound), and with it the scratch worth bringing
#ifndef S5_IP_WAVES
#define S5_IP_WAVES 6
#endif
// a batch holds short records (s5gpu_decode_args.max_pay_cap <= S5_IP_SHORT_PAY): the 256-entry waiting list, 24 waves per CU
#ifndef S5_IP_SHORT_PAY
#define S5_IP_SHORT_PAY 32768u
#endif

namespace s5plan {
constexpr int REC_ZLIB = 1, REC_ZSTD = 2;        // = S5GPU_REC_* ...
constexpr uint32_t IP_SPAN = 4096;               // ... = s5::IP_SPAN (inflate_par_dev.h), NT (dev_common.h) and ZW_REC / 4 (zstd_dev.h):
constexpr uint32_t WG = 256;                     // decode_kernels.hip asserts all of them
constexpr uint32_t ZW_WORDS = 36;                // words per record of the zstd weights pass
constexpr uint32_t IP_WAVES = S5_IP_WAVES, SHORT_PAY = S5_IP_SHORT_PAY;

// "from this many records on" (the order list's order_min, the weights pass's zstd_pre_min): 0 = never
inline bool from_count(uint32_t n_recs, uint32_t min_recs) { return min_recs && n_recs >= min_recs; }
// words of scratch the weights pass of a zstd batch takes
inline uint64_t zstd_pre_words(uint32_t n_recs, uint32_t zstd_pre_min) { return from_count(n_recs, zstd_pre_min) ? (uint64_t)n_recs * ZW_WORDS : 0; }

// The waiting list's size follows what was compressed and how long the records are (inflate_par_dev.h): short svb-zd / ex-zd records take
// the 256-entry list; long ones (several hundred waiting matches per window in their key bytes: 14.7 ms per 8192 records of
// merged_expected_zlib_svb.blow5 with 768 entries, 23.3 with 256), raw-signal records and callers that do not say (max_pay_cap = 0) the
// 768-entry one.  (An ex-zd slot is sized for its worst case, 9.5 bytes per sample against svb-zd's 3.25: the same reads, three times the slot.)
inline bool short_list(int sig_method, uint32_t max_pay_cap) { return max_pay_cap != 0 && max_pay_cap <= SHORT_PAY * (sig_method == SIG_EX_ZD ? 3u : 1u); }

// ---- S5GPU_DEC_NO_PAYLOAD: persistent workgroups, one reused scratch slot each ----
// the decoders that keep no payload: zlib / zstd + svb-zd and zlib + ex-zd; every other pair is decoded in full
inline bool np_served(int rec_method, int sig_method) {
    return (sig_method == SIG_SVB_ZD && (rec_method == REC_ZLIB || rec_method == REC_ZSTD)) || (sig_method == SIG_EX_ZD && rec_method == REC_ZLIB);
}
inline uint64_t np_slot(uint32_t max_pay_cap) { return ((uint64_t)max_pay_cap + 16 + 15) & ~15ull; }   // bytes per slot, a multiple of 16
// a slot size is named, fits 32 bits, and the scratch holds the ticket words and two slots (one main workgroup, one of the fallback's)
inline bool np_args_ok(uint32_t max_pay_cap, uint64_t payload_bytes) {
    const uint64_t slot = np_slot(max_pay_cap);
    return max_pay_cap != 0 && slot <= 0xFFFFFFF0ull && payload_bytes >= 64 + 2 * slot;
}
// scratch worth bringing: one slot per workgroup the device can hold + the fallback decoder's
inline uint64_t np_scratch_bytes(uint32_t max_pay_cap) { return 64 + np_slot(max_pay_cap) * (256ull * IP_WAVES * 4 + 256); }
// ... and what the host layer brings for n records, of the `scratch` that s5gpu_decode_scratch_bytes calls worth bringing: more slots than
// records (and the fallback's) buy nothing, 1 GiB at most, two slots at least
inline uint64_t np_scratch_for(uint64_t scratch, uint32_t max_pay_cap, uint32_t n_recs) {
    const uint64_t slot = np_slot(max_pay_cap), enough = 64 + slot * ((uint64_t)n_recs + 257), floor_ = 64 + 2 * slot, ceil_ = 1ull << 30;
    if (scratch > enough) scratch = enough;
    if (scratch > ceil_) scratch = ceil_;
    if (scratch < floor_) scratch = floor_;
    return scratch;
}
// The kernel variant (np_kernel of decode_kernels.hip): 0 .. 3 = zlib, svb-zd (0, 1) / ex-zd (2, 3) records with the long (even) / short (odd)
// waiting list; 4 = zstd; 5 = short svb-zd records kept in LDS: their payloads all fit the window's storage (the caller names the longest
// compressed record: the kernel takes records of one window — IP_SPAN bytes with the block header — and declines what turns out not to fit).
// For a served pair and a max_pay_cap that np_args_ok took.
inline int np_variant(int rec_method, int sig_method, uint32_t max_pay_cap, uint32_t max_in_len, uint32_t np_lds_payload) {
    const bool zl = rec_method == REC_ZLIB, xz = sig_method == SIG_EX_ZD;
    const bool lds_pay = zl && !xz && np_lds_payload && max_in_len != 0 && max_in_len <= IP_SPAN - 96u;
    return !zl ? 4 : lds_pay ? 5 : (xz ? 2 : 0) + (short_list(sig_method, max_pay_cap) ? 1 : 0);
}
// The launch shape.  More workgroups than the device holds at once (`resident`, asked for the variant that is launched) buy nothing: they
// would only spread the scratch over more of L2.  n_fb: the zlib fallback kernel's workgroups, with slots of their own behind the main ones.
// ticket: records come off a counter; not for a zlib batch of one record per workgroup (get batches: nothing to clear).
struct NpShape { uint64_t n_slots, n_fb, n_main; bool ticket; };
inline NpShape np_shape(int rec_method, uint32_t max_pay_cap, uint64_t payload_bytes, uint32_t resident, uint32_t n_recs) {
    const bool zl = rec_method == REC_ZLIB;
    NpShape s;
    s.n_slots = (payload_bytes - 64) / np_slot(max_pay_cap);
    s.n_fb = zl ? (s.n_slots / 16 < 1 ? 1 : s.n_slots / 16 > 256 ? 256 : s.n_slots / 16) : 0;
    s.n_main = s.n_slots - s.n_fb;
    if (s.n_main > resident) s.n_main = resident;
    if (s.n_main > n_recs) s.n_main = n_recs;
    s.ticket = !(zl && n_recs <= s.n_main);
    return s;
}

// ---- the full decode ----
// svb-zd (1) and ex-zd (2) records under zlib (the default inflate kernel) or zstd: the wave that decompresses a record unpacks it too; 0: k_unpack
inline int fused_unpack(int rec_method, int sig_method, uint32_t unpack_fused, uint32_t inflate_par) {
    const bool rec = (rec_method == REC_ZLIB && inflate_par == 1) || rec_method == REC_ZSTD;
    return !unpack_fused || !rec ? 0 : sig_method == SIG_SVB_ZD ? 1 : sig_method == SIG_EX_ZD ? 2 : 0;
}
// Which kernels inflate: zstd frames, the decoder that is parallel inside a record, or the two older zlib kernels chosen by batch size — a
// lane per record from inflate_simt_min records on (highest throughput), else a wave per record (lowest latency; records without a press too)
enum Inflate { INFLATE_ZSTD, INFLATE_PAR, INFLATE_LANE, INFLATE_WAVE };
inline Inflate inflate_family(int rec_method, uint32_t n_recs, uint32_t inflate_par, uint32_t inflate_simt_min) {
    return rec_method == REC_ZSTD ? INFLATE_ZSTD : rec_method != REC_ZLIB ? INFLATE_WAVE : inflate_par ? INFLATE_PAR : n_recs >= inflate_simt_min ? INFLATE_LANE : INFLATE_WAVE;
}
inline bool par_fallback(uint32_t inflate_par) { return inflate_par == 1; }   // (2, tools: no fallback pass, declined records keep status 8)
// routing is the lane kernel's own need (independent of order_min); tiny batches (tests force the lane kernel on them) go without
inline bool lane_routed(uint32_t n_recs, uint32_t inflate_route) { return n_recs >= 1024 && inflate_route; }

// ---- grids of the persistent kernels ----
inline uint32_t fallback_grid(uint32_t n_recs) { return (n_recs + 63) / 64 < 4096 ? (n_recs + 63) / 64 : 4096; }                 // k_inflate_fallback
inline uint32_t unpack_rest_grid(uint32_t n_recs) { return (n_recs + WG - 1) / WG < 2048 ? (n_recs + WG - 1) / WG : 2048; }     // k_unpack_rest
inline uint32_t long_grid(uint32_t n_recs) { return n_recs < 16384 ? n_recs : 16384; }                                          // k_inflate_long
inline uint32_t lane_grid(uint32_t n_recs) { return (n_recs + 63) / 64; }   // a record per lane: k_zstd_weights, k_inflate_simt
}   // namespace s5plan
