// decode_kernels.hip — gfx950 (CDNA4) kernels of the decode half of the BLOW5 record press path + their launchers: inflate (a wave per
// record, parallel inside a record, a lane per record), zstd, the unpack of payloads into fields and signals, and the svb-zd decode alone.
// What is launched, and with which shape, is decided in dec_plan.h; here the plan becomes kernels from the tables and launches.
#include <stddef.h>
#include <limits.h>

#include <type_traits>
#include <vector>

#include "launch_common.h"
#include "resident_rules.h"
#include "dec_plan.h"
#include "inflate_dev.h"
#include "inflate_simt_dev.h"
#include "inflate_par_dev.h"
#include "zstd_dev.h"
#include "svb_dev.h"
#include "exzd_dev.h"
#define S5_ORDER_LIST_ONLY   // (the lists are read here; order_launch.hip builds them)
#include "order_dev.h"

using namespace s5;

static_assert(s5plan::REC_ZLIB == S5GPU_REC_ZLIB && s5plan::REC_ZSTD == S5GPU_REC_ZSTD && s5plan::SIG_SVB_ZD == S5GPU_SIG_SVB_ZD && s5plan::SIG_EX_ZD == S5GPU_SIG_EX_ZD &&
              s5plan::IP_SPAN == (uint32_t)IP_SPAN && s5plan::WG == (uint32_t)NT && s5plan::ZW_WORDS == ZW_REC / 4, "dec_plan.h restates these");

extern __shared__ __attribute__((aligned(16))) uint8_t smem[];

__device__ __forceinline__ uint64_t ld_le(const uint8_t *p, int nbytes) {
    uint64_t v = 0;
    for (int i = 0; i < nbytes; i++) v |= (uint64_t)p[i] << (8 * i);
    return v;
}

// K4: one record per wave64 (workgroup = 1 wave).  zlib stream -> payload slot; Adler-32 verified.
__global__ __launch_bounds__(64) void k_inflate(s5gpu_decode_args_t a) {
    __shared__ InflShared T;
    const uint32_t r = blockIdx.x;
    const s5gpu_rec_desc_t d = a.desc[r];
    const uint8_t *in = a.in + d.in_off;
    uint8_t *out = a.payload + d.pay_off;
    const int lane = lane_id();
    uint32_t olen = 0;
    int status;
    if (a.rec_method == S5GPU_REC_NONE) {
        status = d.in_len > d.pay_cap ? INF_ERR_OVERFLOW : INF_OK;
        olen = d.in_len;
        if (status == INF_OK)
            for (uint32_t i = lane; i < d.in_len; i += 64) out[i] = in[i];
    } else {
        status = zlib_inflate_wave(T, in, d.in_len, out, d.pay_cap, &olen);   // Adler-32 verified inside
    }
    if (lane == 0) {
        a.fields[r].status = status;
        a.fields[r].payload_len = olen;
    }
}

// The first pay_cap bytes of every zlib record and no more (record heads for the index builder: read_id_len | read_id | ...): one
// record per wave, the wave-per-record decoder stopped early.  d.in_len may cover just the front of the record.
__global__ __launch_bounds__(64) void k_inflate_head(s5gpu_decode_args_t a) {
    __shared__ InflShared T;
    const uint32_t r = blockIdx.x;
    const s5gpu_rec_desc_t d = a.desc[r];
    uint32_t olen = 0;
    const int status = zlib_inflate_wave<true>(T, a.in + d.in_off, d.in_len, a.payload + d.pay_off, d.pay_cap, &olen);
    if (lane_id() == 0) {
        a.fields[r].status = status;
        a.fields[r].payload_len = olen;
    }
}

// K4, parallel inside the record (inflate_par_dev.h): one record per wave64, 64 self-synchronising segment decoders.  Default for
// every batch size; what it declines (status INF_NEED_FALLBACK) the wave-per-record decoder redoes right behind it.
// UNPACK (s5gpu_decode_dev on svb-zd records): the wave that inflated a record also parses it and decodes its signal — the payload
// it just wrote is in L2, the window is free as a stage for the data bytes, and the chain of dependent loads a separate kernel
// starts with (fields -> descriptor -> three length fields of the payload) is gone.  fields.reserved = 1 marks such a record;
// k_unpack_rest does what is left (records the fallback decoder inflated) and clears the marks.
static_assert(offsetof(InflParSharedSvb, win) == 0 && offsetof(InflParSharedSvb, dlut) >= SVB_WSTAGE && offsetof(InflParShared, dlut) >= SVB_WSTAGE,
              "the inflate window and the waiting list behind it (both dead once the record is out) double as the svb-zd stage");
// pay: the record's uncompressed bytes — its payload slot, or the workgroup's scratch slot (S5GPU_DEC_NO_PAYLOAD)
template <bool STAGED = true>     // false: pay lies in LDS already (k_inflate_par_np<.., LP>), nothing is staged
__device__ __forceinline__ int unpack_svbzd_wave(const s5gpu_decode_args_t &a, const s5gpu_rec_desc_t &d, const uint8_t *pay, s5gpu_rec_fields_t &f, uint32_t plen, uint8_t *stage) {
    if (plen < 2) return 7;
    const uint32_t idl = (uint32_t)ld_le(pay, 2), hl = 2 + idl + 4 + 32;
    if ((uint64_t)hl + 8 > plen) return 7;
    const uint64_t L = ld_le(pay + hl, 8);
    const uint8_t *sigp = pay + hl + 8;
    const uint32_t avail = plen - hl - 8;
    if (L > avail || L < 4) return 7;
    const uint32_t n = (uint32_t)ld_le(sigp, 4), nk = svb_key_bytes(n);
    if (!svb_count_fits(n, L)) return 7;
    if (n > d.sig_cap) { if (lane_id() == 0) f.n_samples = n; return 6; }
    const uint8_t *keys = sigp + 4, *data = keys + nk, *dend = sigp + L;
    int16_t *out = a.sig_out + d.sig_off;
    uint32_t total = 0;
    int carry = 0, err = 0;
    for (uint32_t t0 = 0; t0 < n; t0 += SVB_WTILE)
        total += svb_decode_tile_wave<STAGED>(keys + (t0 >> 2), data + total, dend, n, t0, out, carry, err, stage);
    if (__ballot(err != 0) || 4 + nk + total != L) return 7;
    if (lane_id() == 0) {
        f.n_samples = n;
        f.read_id_len = idl;
        f.read_group = (uint32_t)ld_le(pay + 2 + idl, 4);
        uint64_t v[4];
        for (int q = 0; q < 4; q++) v[q] = ld_le(pay + 2 + idl + 4 + 8 * q, 8);
        f.digitisation = __longlong_as_double((long long)v[0]);
        f.offset = __longlong_as_double((long long)v[1]);
        f.range = __longlong_as_double((long long)v[2]);
        f.sampling_rate = __longlong_as_double((long long)v[3]);
        f.aux_off = hl + 8 + (uint32_t)L;
        f.aux_len = plen - (hl + 8 + (uint32_t)L);
    }
    return 0;
}
// ... and an ex-zd one (round 3; exzd_decode_wave): the scratch is the whole table set of the inflate, dead once the record is out
static_assert(sizeof(ExzdWaveScratch) <= sizeof(InflParSharedSvb), "the ex-zd wave scratch overlays the inflate's LDS");
__device__ __forceinline__ int unpack_exzd_wave(const s5gpu_decode_args_t &a, const s5gpu_rec_desc_t &d, const uint8_t *pay, s5gpu_rec_fields_t &f, uint32_t plen, ExzdWaveScratch &X) {
    if (plen < 2) return 7;
    const uint32_t idl = (uint32_t)ld_le(pay, 2), hl = 2 + idl + 4 + 32;
    if ((uint64_t)hl + 8 > plen) return 7;
    const uint64_t L = ld_le(pay + hl, 8);
    const uint32_t avail = plen - hl - 8;
    if (L > avail) return 7;
    uint32_t n = 0;
    const int st = exzd_decode_wave(pay + hl + 8, L, a.sig_out + d.sig_off, d.sig_cap, n, X);
    if (st) { if (st == 6 && lane_id() == 0) f.n_samples = n; return st; }
    if (lane_id() == 0) {
        f.n_samples = n;
        f.read_id_len = idl;
        f.read_group = (uint32_t)ld_le(pay + 2 + idl, 4);
        uint64_t v[4];
        for (int q = 0; q < 4; q++) v[q] = ld_le(pay + 2 + idl + 4 + 8 * q, 8);
        f.digitisation = __longlong_as_double((long long)v[0]);
        f.offset = __longlong_as_double((long long)v[1]);
        f.range = __longlong_as_double((long long)v[2]);
        f.sampling_rate = __longlong_as_double((long long)v[3]);
        f.aux_off = hl + 8 + (uint32_t)L;
        f.aux_len = plen - (hl + 8 + (uint32_t)L);
    }
    return 0;
}
// A launch of no more records than the device holds waves (a `get` batch) is as slow as its slowest record: its first pass walks whole segments
// (inflate_par_dev.h, `tail`)
#ifndef S5_IP_LAT_RECS
#define S5_IP_LAT_RECS 6144u
#endif
__device__ __forceinline__ uint32_t ip_tail_for(uint32_t n_recs) { return n_recs <= S5_IP_LAT_RECS ? 0xFFFFu : IP_TAIL; }
template <int UNPACK, bool SHORT = true>      // UNPACK 0: inflate only; 1: + parse and svb-zd decode; 2: + parse and ex-zd decode
__global__ __launch_bounds__(64, S5_IP_WAVES) void k_inflate_par(s5gpu_decode_args_t a, const uint32_t *ord) {
    __shared__ typename std::conditional<UNPACK != 0 && SHORT, InflParSharedSvb, InflParShared>::type T;   // short svb-zd / ex-zd records: the small waiting list (inflate_par_dev.h)
    const uint32_t r = order_at(ord, blockIdx.x);
    const s5gpu_rec_desc_t d = a.desc[r];
    uint32_t olen = 0;
#ifdef S5_PAR_PROBE   // tools/par_probe.py only (a variant build, tools/variant.sh probe -DS5_PAR_PROBE): cut-offs 91..93 and counters (99) keyed on sig_method
    uint32_t dbg[4] = {0, 0, 0, a.sig_method >= 90 && a.sig_method < 99 ? (uint32_t)(a.sig_method - 90) : a.sig_method >= 81 && a.sig_method < 90 ? (uint32_t)(a.sig_method - 70) : 0u};
    int status = zlib_inflate_par(T, a.in + d.in_off, d.in_len, a.payload + d.pay_off, d.pay_cap, &olen, !UNPACK && a.sig_method >= 81 ? dbg : nullptr, ip_tail_for(a.n_recs));
#else
    int status = zlib_inflate_par(T, a.in + d.in_off, d.in_len, a.payload + d.pay_off, d.pay_cap, &olen, nullptr, ip_tail_for(a.n_recs));
#endif
    uint32_t mark = 0;
    if (UNPACK && status == 0) {
        wave_sync();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        if (UNPACK == 2) status = unpack_exzd_wave(a, d, a.payload + d.pay_off, a.fields[r], olen, *reinterpret_cast<ExzdWaveScratch *>(&T));
        else status = unpack_svbzd_wave(a, d, a.payload + d.pay_off, a.fields[r], olen, reinterpret_cast<uint8_t *>(T.win));
        mark = 1;
    }
    if (lane_id() == 0) {
        a.fields[r].status = status;
        a.fields[r].payload_len = olen;
        if (UNPACK) a.fields[r].reserved = mark;
#ifdef S5_PAR_PROBE
        if (!UNPACK && a.sig_method == 99) { a.fields[r].n_samples = dbg[0]; a.fields[r].read_id_len = dbg[1]; a.fields[r].read_group = dbg[2]; }
#endif
    }
}
__global__ __launch_bounds__(64) void k_inflate_fallback(s5gpu_decode_args_t a) {   // persistent blocks scan the statuses
    __shared__ InflShared T;
    const int lane = lane_id();
    for (uint32_t base = blockIdx.x * 64u; base < a.n_recs; base += gridDim.x * 64u) {
        const uint32_t mine = base + (uint32_t)lane;
        uint64_t need = __ballot(mine < a.n_recs && a.fields[mine].status == INF_NEED_FALLBACK);
        while (need) {
            const uint32_t r = base + (uint32_t)(__ffsll((long long)need) - 1);
            need &= need - 1;
            const s5gpu_rec_desc_t d = a.desc[r];
            uint32_t olen = 0;
            const int status = zlib_inflate_wave(T, a.in + d.in_off, d.in_len, a.payload + d.pay_off, d.pay_cap, &olen);
            if (lane == 0) {
                a.fields[r].status = status;
                a.fields[r].payload_len = olen;
            }
            wave_sync();
        }
    }
}

// ---- S5GPU_DEC_NO_PAYLOAD: fields + signals only, the uncompressed record never has to reach HBM ----
// The caller of a signal consumer (`get`, the decode side of a basecaller feed) has no use for the uncompressed record, and writing
// it out costs as much HBM traffic as the whole rest of the decode (5.1 KB written + read back per 4000-sample record against
// Z + 2N = 11.5 KB: PMC, profiles/r02_pmc_decode_traffic.txt).  Persistent workgroups, one scratch slot each, reused record after
// record: the slot's lines stay in the XCD's L2 (a workgroup never leaves its CU), the record is inflated into it and unpacked
// out of it by the same wave.  Records come off a ticket counter, so workgroups that drew long records simply draw fewer.
struct NpParams {
    uint8_t *scratch;      // slot i at scratch + i * slot
    uint32_t slot;         // bytes per slot (a multiple of 16)
    uint32_t cap;          // payload bytes a slot takes (slot - 16)
    uint32_t *ticket;      // [0]: next record of the main kernel
    uint32_t first_fb;     // first slot of the fallback kernel's workgroups
    const uint32_t *ord;   // launch order (longest records first), or nullptr
};
#ifdef S5_NP_TRIPWIRE
// Tripwire of the no-payload decode (tools only): an independent Adler-32 of the scratch slot — byte loads, one lane's running sums at a time
// folded by a wave reduction, nothing shared with the inflate's dword / dot-product pass — and the record's trailer.
__device__ __forceinline__ uint32_t np_trailer(const uint8_t *in, uint32_t in_len) {
    const uint8_t *t = in + in_len - 4;
    return ((uint32_t)t[0] << 24) | ((uint32_t)t[1] << 16) | ((uint32_t)t[2] << 8) | t[3];
}
template <bool BYPASS>     // BYPASS: agent-scope atomic byte loads (around this CU's L1); otherwise the plain loads the unpack uses
__device__ __forceinline__ uint32_t np_slot_adler(const uint8_t *pay, uint32_t n) {
    // lane l owns bytes [l * c, (l + 1) * c): A_l = sum x, B_l = sum (len_l - i) x_i; the lanes combine as Adler-32 concatenation
    const uint32_t c = (n + 63u) / 64u, lo = min(n, (uint32_t)lane_id() * c), hi = min(n, lo + c);
    uint64_t sa = 0, sb = 0;
    for (uint32_t i = lo; i < hi; i++) {
        const uint32_t x = BYPASS ? (uint32_t)__hip_atomic_load(pay + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : (uint32_t)pay[i];
        sa += x; sb += (uint64_t)(n - i) * x;
    }
    for (int d = 32; d >= 1; d >>= 1) { sa += __shfl_xor(sa, d); sb += __shfl_xor(sb, d); }
    const uint32_t A = (uint32_t)((1 + sa) % 65521u), B = (uint32_t)((n + sb) % 65521u);
    return (B << 16) | A;
}
// decode the svb-zd blob of the slot again — lane l the l-th 64th of the samples, scalar code per lane: its first data byte from a plain
// sum over the keys in front of it, its first sample from the deltas in front of it (a wave prefix sum is the one primitive shared with the
// unpack) — and compare with what the unpack stored.  Called only on a record the unpack decoded (status 0): its count, keys and data
// bytes are known to fit the blob, so the reads below stay inside it
__device__ __forceinline__ int np_signal_check(const s5gpu_decode_args_t &a, const s5gpu_rec_desc_t &d, const uint8_t *pay, uint32_t plen) {
    const uint32_t idl = (uint32_t)ld_le(pay, 2), hl = 2 + idl + 4 + 32;
    const uint8_t *sigp = pay + hl + 8;
    const uint32_t n = (uint32_t)ld_le(sigp, 4), nk = (n + 3) >> 2;
    const uint8_t *keys = sigp + 4, *data = keys + nk;
    const int16_t *out = a.sig_out + d.sig_off;
    const uint32_t c = ((n + 63u) / 64u + 3u) & ~3u;                 // samples per lane, a multiple of 4: lanes start on a key byte
    const uint32_t lo = min(n, (uint32_t)lane_id() * c), hi = min(n, lo + c);
    uint32_t at = 0;
    for (uint32_t k = 0; k < (lo >> 2); k++) { const uint32_t kb = keys[k]; at += 4u + (kb & 3u) + ((kb >> 2) & 3u) + ((kb >> 4) & 3u) + (kb >> 6); }
    int sum = 0;
    {
        uint32_t q = at;
        for (uint32_t i = lo; i < hi; i++) {
            const uint32_t code = (keys[i >> 2] >> (2 * (i & 3))) & 3u;
            uint32_t zz = 0;
            for (uint32_t k = 0; k <= code; k++) zz |= (uint32_t)data[q + k] << (8 * k);
            q += code + 1;
            sum += (int)(zz >> 1) ^ -(int)(zz & 1);
        }
    }
    int acc = (int)(wave_incl_add((uint32_t)sum) - (uint32_t)sum);
    int bad = 0;
    for (uint32_t i = lo; i < hi; i++) {
        const uint32_t code = (keys[i >> 2] >> (2 * (i & 3))) & 3u;
        uint32_t zz = 0;
        for (uint32_t k = 0; k <= code; k++) zz |= (uint32_t)data[at + k] << (8 * k);
        at += code + 1;
        acc += (int)(zz >> 1) ^ -(int)(zz & 1);
        if (__hip_atomic_load(out + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != (int16_t)acc) bad = 1;
    }
    return __ballot(bad != 0) ? 1 : 0;
}
#endif
__device__ __forceinline__ void np_write_fields(const s5gpu_decode_args_t &a, uint32_t r, int status, uint32_t olen) {
    if (lane_id() == 0) {
        a.fields[r].status = status;
        a.fields[r].payload_len = olen;
        a.fields[r].reserved = 0;
    }
}
// LP (round 6; svb-zd records of a batch whose payloads fit SH::LDS_PAY): the record is inflated into the window's own LDS storage and unpacked
// from there — no scratch slot, no byte of the uncompressed record in HBM (zlib_inflate_par<.., LDSOUT>).  What that inflate declines (a
// second window or block, a stored block, a longer record) goes to the fallback kernel's slot like any other declined record.
template <bool EXZD, bool SHORT, bool LP, class SH>
__device__ __forceinline__ void np_records(const s5gpu_decode_args_t &a, NpParams np, SH &T) {
    static_assert(!LP || (SHORT && !EXZD), "");
    uint8_t *pay;
    if constexpr (LP) pay = reinterpret_cast<uint8_t *>(T.win);
    else pay = np.scratch + (uint64_t)blockIdx.x * np.slot;
    // (round 6 measured the NEXT record's ticket drawn during the inflate and its descriptor fetched under the unpack: 25.34 against 24.62 ms per
    // 1 M records — the two round trips it hides are not what the wave waits for, and the loop-carried descriptor costs registers)
    for (;;) {
        uint32_t r = blockIdx.x;
        if (np.ticket) {                               // (a batch no larger than the grid: workgroup b takes record b, no ticket)
            if (lane_id() == 0) r = atomicAdd(&np.ticket[0], 1u);
            r = __builtin_amdgcn_readfirstlane(r);
        }
        if (r >= a.n_recs) return;
        r = order_at(np.ord, r);
        const s5gpu_rec_desc_t d = a.desc[r];
        uint32_t olen = 0;
#ifdef S5_PAR_PROBE   // tools/np_probe_pmc.sh (variant build): the cut-offs of tools/par_probe.py in the no-payload kernels, keyed on the top byte of a.flags
        uint32_t dbg[4] = {0, 0, 0, a.flags >> 24};
        int status = zlib_inflate_par<SH, LP>(T, a.in + d.in_off, d.in_len, pay, np.cap, &olen, dbg[3] ? dbg : nullptr, np.ticket ? IP_TAIL : 0xFFFFu);
        if (dbg[3] && dbg[3] != 9u) status = 100;         // (nothing to unpack; 9: the whole inflate, no unpack)
        else if (dbg[3] == 9u && status == 0) status = 100;
#else
        int status = zlib_inflate_par<SH, LP>(T, a.in + d.in_off, d.in_len, pay, np.cap, &olen, nullptr, np.ticket ? IP_TAIL : 0xFFFFu);   // (no ticket: a batch of one record per workgroup)
#endif
#ifdef S5_IP_PAD
        if (d.in_len == 0xFFFFFFFFu) T.pad[lane_id()] = 1;   // (keeps the padding alive)
#endif
        if (status == 0) {
            wave_sync();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
#ifdef S5_NP_TRIPWIRE   // tools/np_tripwire.py (a variant build): is the slot still what the inflate verified when the unpack reads it, and afterwards?
            const uint32_t want_ad = np_trailer(a.in + d.in_off, d.in_len);
            {   // 20: the slot differs from what the inflate verified, seen through L1 and around it; 23: only through L1 (stale lines of
                // the slot's previous record); 24: only around it
                const bool bad_l1 = np_slot_adler<false>(pay, olen) != want_ad, bad_l2 = np_slot_adler<true>(pay, olen) != want_ad;
                if (bad_l1 || bad_l2) status = bad_l1 && bad_l2 ? 20 : bad_l1 ? 23 : 24;
            }
#endif
            if (status == 0) {
#ifdef S5_IPROBE
                const unsigned long long t0_ = __builtin_readcyclecounter();
#endif
                if (EXZD) status = unpack_exzd_wave(a, d, pay, a.fields[r], olen, *reinterpret_cast<ExzdWaveScratch *>(&T));
                else status = unpack_svbzd_wave<!LP>(a, d, pay, a.fields[r], olen, reinterpret_cast<uint8_t *>(T.win));
#ifdef S5_IPROBE
                if (lane_id() == 0) atomicAdd(&g_iprobe[13], (unsigned long long)__builtin_readcyclecounter() - t0_);
#endif
            }
#ifdef S5_NP_TRIPWIRE
            if (status == 0) {
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");                      // the samples just stored are read back around L1
                wave_sync();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
                if (np_slot_adler<false>(pay, olen) != want_ad || np_slot_adler<true>(pay, olen) != want_ad) status = 21;   // changed while the unpack was reading it
                else if (!EXZD && np_signal_check(a, d, pay, olen)) status = 22;       // the slot is intact and the samples written differ from it: the unpack read wrong
            }
#endif
        }
        np_write_fields(a, r, status, olen);
        if (!np.ticket) return;
        wave_sync();                                   // the next record's window load overwrites the stage
    }
}
template <bool EXZD, bool SHORT = true>
__global__ __launch_bounds__(64, S5_IP_WAVES) void k_inflate_par_np(s5gpu_decode_args_t a, NpParams np) {
    __shared__ typename std::conditional<SHORT, InflParSharedSvb, InflParShared>::type T;
    np_records<EXZD, SHORT, false>(a, np, T);
}
// (8192 bytes of LDS per wave = 20 waves per CU, five per SIMD: 96 registers.  Left to itself the compiler plans this kernel for four waves
// per SIMD and 120 registers — 16 waves per CU, which measured 14 % slower on the slot form)
__global__ __launch_bounds__(64, 5) void k_inflate_par_np_lp(s5gpu_decode_args_t a, NpParams np) {
    __shared__ InflParSharedLp T;
    np_records<false, true, true>(a, np, T);
}
// ... what the parallel decoder declined: the wave-per-record decoder, into its own scratch slot, and the unpack right behind it
static_assert(offsetof(InflShared, llut) == offsetof(InflShared, ring) + INF_OW && INF_OW + sizeof(InflShared::llut) >= SVB_WSTAGE,
              "the output ring and the table behind it double as the svb-zd stage");
__global__ __launch_bounds__(64) void k_inflate_fallback_np(s5gpu_decode_args_t a, NpParams np) {
    __shared__ InflShared T;
    const int lane = lane_id();
    uint8_t *pay = np.scratch + (uint64_t)(np.first_fb + blockIdx.x) * np.slot;
    for (uint32_t base = blockIdx.x * 64u; base < a.n_recs; base += gridDim.x * 64u) {
        const uint32_t mine = base + (uint32_t)lane;
        uint64_t need = __ballot(mine < a.n_recs && a.fields[mine].status == INF_NEED_FALLBACK);
        while (need) {
            const uint32_t r = base + (uint32_t)(__ffsll((long long)need) - 1);
            need &= need - 1;
            const s5gpu_rec_desc_t d = a.desc[r];
            uint32_t olen = 0;
            int status = zlib_inflate_wave(T, a.in + d.in_off, d.in_len, pay, np.cap, &olen);
            if (status == 0) {
                wave_sync();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
                if (a.sig_method == S5GPU_SIG_EX_ZD) status = unpack_exzd_wave(a, d, pay, a.fields[r], olen, *reinterpret_cast<ExzdWaveScratch *>(&T));
                else status = unpack_svbzd_wave(a, d, pay, a.fields[r], olen, T.ring);
            }
            np_write_fields(a, r, status, olen);
            wave_sync();
        }
    }
}
// zstd records, a pass in front of the decoders: the first Huffman tree description of every frame, one frame per lane (zstd_dev.h)
__global__ __launch_bounds__(64) void k_zstd_weights(s5gpu_decode_args_t a, uint8_t *ws) {
    __shared__ uint32_t L[64 * ZW_LANE_DW];
    const uint32_t r = blockIdx.x * 64u + threadIdx.x;
    if (r >= a.n_recs) return;
    const s5gpu_rec_desc_t d = a.desc[r];
    zstd_first_tree_lane(L + threadIdx.x * ZW_LANE_DW, a.in + d.in_off, d.in_len, ws + (uint64_t)r * ZW_REC);
}
__global__ __launch_bounds__(64) void k_zstd_inflate_np(s5gpu_decode_args_t a, NpParams np, const uint8_t *ws) {
    __shared__ __attribute__((aligned(16))) ZstdShared T;
    uint8_t *pay = np.scratch + (uint64_t)blockIdx.x * np.slot;
    for (;;) {
        uint32_t r = 0;
        if (lane_id() == 0) r = atomicAdd(&np.ticket[0], 1u);
        r = __builtin_amdgcn_readfirstlane(r);
        if (r >= a.n_recs) return;
        const s5gpu_rec_desc_t d = a.desc[r];
        uint32_t olen = 0;
        int status = zstd_decode_wave(T, a.in + d.in_off, d.in_len, pay, np.cap, &olen, ws ? ws + (uint64_t)r * ZW_REC : nullptr);
        if (status == 0) {
            wave_sync();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
            status = unpack_svbzd_wave(a, d, pay, a.fields[r], olen, reinterpret_cast<uint8_t *>(T.huf));
        }
        np_write_fields(a, r, status, olen);
        wave_sync();
    }
}

// K4 for the zstd record press: one frame per wave64 (zstd_dev.h).  UNPACK: as k_inflate_par<1> — the wave parses the record and
// decodes its svb-zd signal right away (the Huffman table's storage is the stage), k_unpack_rest clears the marks
static_assert(sizeof(ZstdShared::huf) + sizeof(ZstdShared::ll_e) >= SVB_WSTAGE && offsetof(ZstdShared, ll_e) == sizeof(ZstdShared::huf),
              "the Huffman table and the table behind it double as the svb-zd stage");
#ifndef S5_ZI_W
#define S5_ZI_W 4
#endif
static_assert(sizeof(ExzdWaveScratch) <= sizeof(ZstdShared), "the ex-zd wave scratch overlays the zstd decoder's LDS");
template <int UNPACK>      // 0: decompress only; 1: + parse and svb-zd decode; 2: + parse and ex-zd decode
__global__ __launch_bounds__(64, S5_ZI_W) void k_zstd_inflate(s5gpu_decode_args_t a, const uint32_t *ord, const uint8_t *ws) {
    __shared__ __attribute__((aligned(16))) ZstdShared T;
    const uint32_t r = order_at(ord, blockIdx.x);
    const s5gpu_rec_desc_t d = a.desc[r];
    uint32_t olen = 0;
    int status = zstd_decode_wave(T, a.in + d.in_off, d.in_len, a.payload + d.pay_off, d.pay_cap, &olen, ws ? ws + (uint64_t)r * ZW_REC : nullptr);
    uint32_t mark = 0;
    if (UNPACK && status == 0) {
        wave_sync();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        if (UNPACK == 2) status = unpack_exzd_wave(a, d, a.payload + d.pay_off, a.fields[r], olen, *reinterpret_cast<ExzdWaveScratch *>(&T));
        else status = unpack_svbzd_wave(a, d, a.payload + d.pay_off, a.fields[r], olen, reinterpret_cast<uint8_t *>(T.huf));
        mark = 1;
    }
    if (lane_id() == 0) {
        a.fields[r].status = status;
        a.fields[r].payload_len = olen;
        if (UNPACK) a.fields[r].reserved = mark;
    }
}

// K4, throughput form: one record per LANE (inflate_simt_dev.h); 64 records per workgroup, tables in dynamic LDS.
// Routing of a big zlib batch: a wave takes as long as its longest record and the batch as long as its longest wave, so with the read
// lengths of a real run (log-normal, a tail of 100x the median) the lane kernel alone loses to the wave kernel (tools/mixed_lengths.py).
// So the records are counting-sorted by compressed length (order_dev.h, long_bucket = ROUTE_LONG_BUCKET): a wave then holds records of one
// bucket, the longest waves start first, and records of 32 KiB and more (a lane would need > 30 ms for one) go to the wave-per-record
// kernel, which runs beside the lane kernel.
// ROUTED: the records come through that list (`ord`, longest first), and only the part of the list behind the n_long longest records is
// this kernel's.
template <bool ROUTED>
__global__ __launch_bounds__(64) void k_inflate_simt(s5gpu_decode_args_t a, const uint32_t *ord) {
    uint32_t r = blockIdx.x * 64 + threadIdx.x;
    if (ROUTED && !ord[ORD_FLAG]) {                   // flag != 0: one length class, none of it long; the list was not built (file order)
        const uint32_t n_long = ord[ORD_NLONG];
        if (r >= a.n_recs - n_long) return;
        r = ord[ORD_LIST + n_long + r];
    } else if (r >= a.n_recs) return;
    LaneTables &T = reinterpret_cast<LaneTables *>(smem)[threadIdx.x];
    const s5gpu_rec_desc_t d = a.desc[r];
    uint32_t olen = 0;
    const int status = zlib_inflate_lane(T, a.in + d.in_off, d.in_len, a.payload + d.pay_off, d.pay_cap, &olen);
    a.fields[r].status = status;
    a.fields[r].payload_len = olen;
}
// ... and the wave-per-record kernel over the n_long longest records of the same list (persistent blocks; without a list n_long is 0)
__global__ __launch_bounds__(64) void k_inflate_long(s5gpu_decode_args_t a, const uint32_t *ord) {
    __shared__ InflShared T;
    const uint32_t n_long = ord[ORD_NLONG];
    for (uint32_t i = blockIdx.x; i < n_long; i += gridDim.x) {
        const uint32_t r = ord[ORD_LIST + i];
        const s5gpu_rec_desc_t d = a.desc[r];
        uint32_t olen = 0;
        const int status = zlib_inflate_wave(T, a.in + d.in_off, d.in_len, a.payload + d.pay_off, d.pay_cap, &olen);
        if (lane_id() == 0) {
            a.fields[r].status = status;
            a.fields[r].payload_len = olen;
        }
        wave_sync();
    }
}

// K2 + field parse: payload -> primary fields + int16 raw_signal (slow5_rec_depress_parse, a7/a8)
__device__ __forceinline__ void unpack_record_wg(const s5gpu_decode_args_t &a, uint32_t r, uint32_t *ws, uint8_t *svb_stage, int &s_err) {
    const int tid = threadIdx.x;
    s5gpu_rec_fields_t &f = a.fields[r];
    if (f.status != 0) return;
    const s5gpu_rec_desc_t d = a.desc[r];
    const uint8_t *pay = a.payload + d.pay_off;
    const uint32_t plen = f.payload_len;
    if (tid == 0) s_err = 0;
    __syncthreads();
    int bad = 0;
    uint32_t idl = 0, hl = 0;
    if (plen < 2) bad = 1;
    if (!bad) {
        idl = (uint32_t)ld_le(pay, 2);
        hl = 2 + idl + 4 + 32;
        if ((uint64_t)hl + 8 > plen) bad = 1;
    }
    if (bad) { if (tid == 0) f.status = 7; return; }
    const uint64_t L = ld_le(pay + hl, 8);
    const uint8_t *sigp = pay + hl + 8;
    const uint32_t avail = plen - hl - 8;
    uint32_t n, sig_bytes;
    int16_t *out = a.sig_out + d.sig_off;
    if (a.sig_method == S5GPU_SIG_SVB_ZD) {
        if (L > avail || L < 4) { if (tid == 0) f.status = 7; return; }
        n = (uint32_t)ld_le(sigp, 4);
        const uint32_t nk = svb_key_bytes(n);
        if (!svb_count_fits(n, L)) { if (tid == 0) f.status = 7; return; }
        sig_bytes = (uint32_t)L;
        if (n > d.sig_cap) { if (tid == 0) { f.status = 6; f.n_samples = n; } return; }
        const uint8_t *keys = sigp + 4, *data = keys + nk, *dend = sigp + L;
        uint32_t total = 0;
        int carry = 0, err = 0;
        for (uint32_t t0 = 0; t0 < n; t0 += SVB_TILE)
            total += svb_decode_tile(keys + (t0 >> 2), data + total, dend, n, t0, out, carry, err, ws, svb_stage);
        if (err) s_err = 1;
        __syncthreads();
        if (s_err || 4 + nk + total != L) { if (tid == 0) f.status = 7; return; }
    } else if (a.sig_method == S5GPU_SIG_EX_ZD) {
        if (L > avail) { if (tid == 0) f.status = 7; return; }
        sig_bytes = (uint32_t)L;
        const int st = exzd_decode_wg(sigp, L, out, d.sig_cap, &n, *reinterpret_cast<ExzdScratch *>(smem), ws);
        if (st) { if (tid == 0) { f.status = st; if (st == 6) f.n_samples = n; } return; }
    } else {
        if (L > avail / 2) { if (tid == 0) f.status = 7; return; }
        n = (uint32_t)L;
        sig_bytes = 2 * n;
        if (n > d.sig_cap) { if (tid == 0) { f.status = 6; f.n_samples = n; } return; }
        uint8_t *o8 = reinterpret_cast<uint8_t *>(out);
        for (uint32_t i = tid; i < sig_bytes; i += NT) o8[i] = sigp[i];
    }
    if (tid == 0) {
        f.n_samples = n;
        f.read_id_len = idl;
        f.read_group = (uint32_t)ld_le(pay + 2 + idl, 4);
        uint64_t v[4];
        for (int q = 0; q < 4; q++) v[q] = ld_le(pay + 2 + idl + 4 + 8 * q, 8);
        f.digitisation = __longlong_as_double((long long)v[0]);
        f.offset = __longlong_as_double((long long)v[1]);
        f.range = __longlong_as_double((long long)v[2]);
        f.sampling_rate = __longlong_as_double((long long)v[3]);
        f.aux_off = hl + 8 + sig_bytes;
        f.aux_len = plen - (hl + 8 + sig_bytes);
        f.reserved = 0;   // the contract of unpack_fused: whatever the caller's array held, 0 at the end
    }
}

#ifndef S5_UNP_WG
#define S5_UNP_WG 5
#endif
__global__ __launch_bounds__(NT, S5_UNP_WG) void k_unpack(s5gpu_decode_args_t a) {
    __shared__ uint32_t ws[16];
    __shared__ __attribute__((aligned(16))) uint8_t svb_stage[SVB_STAGE];
    __shared__ int s_err;
    unpack_record_wg(a, blockIdx.x, ws, svb_stage, s_err);
}
// ... behind k_inflate_par<1 | 2>: only the records that kernel did not unpack itself (fields.reserved == 0: the ones the fallback
// decoder inflated); persistent workgroups look at 256 records at a time, and every mark is cleared on the way
__global__ __launch_bounds__(NT) void k_unpack_rest(s5gpu_decode_args_t a) {
    __shared__ uint32_t ws[16];
    __shared__ __attribute__((aligned(16))) uint8_t svb_stage[SVB_STAGE];
    __shared__ int s_err;
    __shared__ uint32_t list[NT], cnt;
    const int tid = threadIdx.x;
    for (uint32_t base = blockIdx.x * NT; base < a.n_recs; base += gridDim.x * NT) {
        if (tid == 0) cnt = 0;
        __syncthreads();
        const uint32_t mine = base + (uint32_t)tid;
        if (mine < a.n_recs) {
            if (a.fields[mine].reserved) a.fields[mine].reserved = 0;
            else list[atomicAdd(&cnt, 1u)] = mine;
        }
        __syncthreads();
        const uint32_t c = cnt;
        for (uint32_t i = 0; i < c; i++) {
            unpack_record_wg(a, list[i], ws, svb_stage, s_err);
            __syncthreads();
        }
        __syncthreads();
    }
}

// K2 alone: svb-zd blob -> int16 (slow5_ptr_depress_solo(SVB_ZD)); in = blobs, fields.n_samples/status out
__global__ __launch_bounds__(NT) void k_svbzd_decode(s5gpu_decode_args_t a) {
    __shared__ uint32_t ws[16];
    __shared__ __attribute__((aligned(16))) uint8_t svb_stage[SVB_STAGE];
    __shared__ int s_err;
    const uint32_t r = blockIdx.x;
    const int tid = threadIdx.x;
    s5gpu_rec_fields_t &f = a.fields[r];
    const s5gpu_rec_desc_t d = a.desc[r];
    const uint8_t *blob = a.in + d.in_off;
    if (tid == 0) s_err = 0;
    __syncthreads();
    if (d.in_len < 4) { if (tid == 0) f.status = 7; return; }
    const uint32_t n = (uint32_t)ld_le(blob, 4), nk = svb_key_bytes(n);
    if (!svb_count_fits(n, d.in_len)) { if (tid == 0) f.status = 7; return; }
    if (n > d.sig_cap) { if (tid == 0) { f.status = 6; f.n_samples = n; } return; }
    const uint8_t *keys = blob + 4, *data = keys + nk, *dend = blob + d.in_len;
    int16_t *out = a.sig_out + d.sig_off;
    uint32_t total = 0;
    int carry = 0, err = 0;
    for (uint32_t t0 = 0; t0 < n; t0 += SVB_TILE)
        total += svb_decode_tile(keys + (t0 >> 2), data + total, dend, n, t0, out, carry, err, ws, svb_stage);
    if (err) s_err = 1;
    __syncthreads();
    if (tid == 0) {
        f.status = (s_err || 4 + nk + total != d.in_len) ? 7 : 0;
        f.n_samples = n;
        f.payload_len = d.in_len;
    }
}

// ------------------------------------------------------------------------------------------------
// launchers (C ABI)
// ------------------------------------------------------------------------------------------------
// Small batches (a single slow5_get) take the wave-per-record decoder (lowest latency); from
// g_inflate_simt_min records on, the lane-per-record decoder (highest throughput).
static uint32_t g_unpack_fused = 1;            // s5gpu_decode_dev, zlib + svb-zd: k_inflate_par unpacks the records it inflates (0: always k_unpack)
static uint32_t g_inflate_par = 1;             // zlib records: the decoder that is parallel inside a record (0: the two older kernels, chosen by batch size)
static uint32_t g_inflate_route = 1;           // big zlib batches: sort by length, long records to the wave kernel (below)
static uint32_t g_np_lds_payload = 1;          // no-payload decode of short svb-zd records: the uncompressed record stays in LDS (option "np_lds_payload")
static uint32_t g_inflate_simt_min = 24576;   // measured crossover on 4000-sample reads: 16384 wave 3.0 ms vs lane 4.2 ms, 32768 wave 5.8 vs lane 4.5
// zstd batches of at least this many frames get the weights pass (k_zstd_weights: the first tree description of every frame, a frame per lane)
// in front of the decoder; smaller ones (a `get` of a few reads) are not worth the extra launch.  Option "zstd_pre_min"; 0 = never.
static uint32_t g_zstd_pre_min = 256;
static const S5Option OPTIONS[] = {
    {"inflate_simt_min", &g_inflate_simt_min, 0, LONG_MAX, ~0u},
    {"inflate_route", &g_inflate_route, 0, 1, ~0u},
    {"np_lds_payload", &g_np_lds_payload, 0, 1, ~0u},
    {"unpack_fused", &g_unpack_fused, 0, 1, ~0u},
    {"inflate_par", &g_inflate_par, 0, 2, ~0u},            // 2 (tools): no fallback pass, declined records keep status 8
    {"zstd_pre_min", &g_zstd_pre_min, 0, LONG_MAX, ~0u},   // zstd batches: weights pass from this many frames on (0: never)
};
int deck::set_option(const char *key, long value) { return s5_set_option(OPTIONS, key, value); }

// the lane-per-record kernels take their tables in dynamic LDS, more than 64 KiB of it: the attribute, once per device
static int set_lds_attrs() {
    DeviceFacts *f = device_facts();
    if (f && f->dec_attrs.load(std::memory_order_acquire)) return S5GPU_OK;
    HIP_TRY(hipFuncSetAttribute((const void *)k_inflate_simt<false>, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_MAX));
    HIP_TRY(hipFuncSetAttribute((const void *)k_inflate_simt<true>, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_MAX));
    if (f) f->dec_attrs.store(true, std::memory_order_release);
    return S5GPU_OK;
}
int deck::warm() { return set_lds_attrs(); }   // (the function attributes need the functions: this loads the code object)

// Helper stream + two events for the routed inflate (the long records run beside the lane kernel).  Pooled PER DEVICE: the batch
// API spawns fresh host threads for every multi-device call, so a per-thread helper would leak a stream and two events per call
// and extra device.  A launch takes one from its device's pool (or makes one) and gives it back once its work is enqueued — the
// stream orders whatever the next user puts on it behind that work.  s5gpu_shutdown releases all of them.
struct AuxStream {
    hipStream_t st = nullptr;
    hipEvent_t fork = nullptr, join = nullptr;
    int dev = -1;
};
static std::mutex g_aux_mu;
static std::vector<AuxStream *> g_aux_all, g_aux_free;
static int aux_acquire(AuxStream **out) {
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    {
        std::lock_guard<std::mutex> lk(g_aux_mu);
        for (size_t i = 0; i < g_aux_free.size(); i++)
            if (g_aux_free[i]->dev == dev) { *out = g_aux_free[i]; g_aux_free.erase(g_aux_free.begin() + (long)i); return S5GPU_OK; }
    }
    AuxStream *a = new AuxStream();
    a->dev = dev;
    if (hipStreamCreateWithFlags(&a->st, hipStreamNonBlocking) != hipSuccess || hipEventCreateWithFlags(&a->fork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&a->join, hipEventDisableTiming) != hipSuccess) {
        if (a->st) (void)hipStreamDestroy(a->st);
        if (a->fork) (void)hipEventDestroy(a->fork);
        delete a;
        s5gpu_set_error("helper stream for the routed inflate could not be created");
        return S5GPU_ERR_HIP;
    }
    std::lock_guard<std::mutex> lk(g_aux_mu);
    g_aux_all.push_back(a);
    *out = a;
    return S5GPU_OK;
}
static void aux_release(AuxStream *a, uint32_t gen) {
    std::lock_guard<std::mutex> lk(g_aux_mu);
    if (gen == s5host_generation) g_aux_free.push_back(a);   // (a shutdown in between has destroyed and freed it)
}
void s5kern_release_aux() {   // s5gpu_shutdown (bumps the generation right after)
    std::lock_guard<std::mutex> lk(g_aux_mu);
    for (AuxStream *a : g_aux_all) {
        (void)hipStreamDestroy(a->st);
        (void)hipEventDestroy(a->fork);
        (void)hipEventDestroy(a->join);
        delete a;
    }
    g_aux_all.clear();
    g_aux_free.clear();
}

// Every decode kernel variant is named in one place: a launch (and, for the no-payload forms further down, the occupancy query in front of
// it) cannot end up with another kernel than the one its caller chose.
using InflateKernel = void (*)(s5gpu_decode_args_t, const uint32_t *);
static InflateKernel inflate_par_kernel(int unpack, bool shortrec) {   // inflate only has one shape: SHORT chooses among the unpacking forms' waiting lists
    if (unpack == 2) return shortrec ? k_inflate_par<2, true> : k_inflate_par<2, false>;
    if (unpack == 1) return shortrec ? k_inflate_par<1, true> : k_inflate_par<1, false>;
    return k_inflate_par<0, true>;
}
using ZstdInflateKernel = void (*)(s5gpu_decode_args_t, const uint32_t *, const uint8_t *);
static ZstdInflateKernel zstd_inflate_kernel(int unpack) {
    return unpack == 2 ? k_zstd_inflate<2> : unpack == 1 ? k_zstd_inflate<1> : k_zstd_inflate<0>;
}

static int launch_inflate(const s5gpu_decode_args_t *a, hipStream_t st, int unpack = 0) {   // unpack: the inflating wave also parses + decodes (1 svb-zd, 2 ex-zd)
    std::unique_lock<std::mutex> hold;            // (the order list's: released when the kernels that read the list are enqueued)
    const uint32_t *ord = nullptr;
    switch (s5plan::inflate_family(a->rec_method, a->n_recs, g_inflate_par, g_inflate_simt_min)) {
    case s5plan::INFLATE_ZSTD: {
        uint32_t *ws32 = nullptr;
        { const int rc = s5kern_decode_order(a, st, &ord, hold, s5plan::zstd_pre_words(a->n_recs, g_zstd_pre_min), &ws32); if (rc) return rc; }
        uint8_t *ws = reinterpret_cast<uint8_t *>(ws32);
        if (ws) hipLaunchKernelGGL(k_zstd_weights, dim3(s5plan::lane_grid(a->n_recs)), dim3(64), 0, st, *a, ws);
        hipLaunchKernelGGL(zstd_inflate_kernel(unpack), dim3(a->n_recs), dim3(64), 0, st, *a, ord, ws);
        break;
    }
    case s5plan::INFLATE_PAR: {
        { const int rc = s5kern_decode_order(a, st, &ord, hold); if (rc) return rc; }
        hipLaunchKernelGGL(inflate_par_kernel(unpack, s5plan::short_list(a->sig_method, a->max_pay_cap)), dim3(a->n_recs), dim3(64), 0, st, *a, ord);
        if (s5plan::par_fallback(g_inflate_par)) hipLaunchKernelGGL(k_inflate_fallback, dim3(s5plan::fallback_grid(a->n_recs)), dim3(64), 0, st, *a);
        break;
    }
    case s5plan::INFLATE_LANE: {
        { const int rc = set_lds_attrs(); if (rc) return rc; }
        const uint32_t nb64 = s5plan::lane_grid(a->n_recs);
        // `hold` stays locked until BOTH readers of the list are enqueued, the lane kernel on st and k_inflate_long on the helper stream; the
        // next build on st is ordered behind the helper stream's join event, so the scratch is free again by then, as for the other lists
        if (s5plan::lane_routed(a->n_recs, g_inflate_route)) {
            const int rc = s5kern_routed_order(a, st, &ord, hold);
            if (rc) return rc;
        }
        if (!ord) {                                   // (no routing, or no scratch for this device: file order is always correct)
            hipLaunchKernelGGL(k_inflate_simt<false>, dim3(nb64), dim3(64), 64 * sizeof(LaneTables), st, *a, ord);
        } else {
            AuxStream *ax;
            const uint32_t aux_gen = s5host_generation;
            { const int rc = aux_acquire(&ax); if (rc) return rc; }
            struct AuxGuard { AuxStream *a; uint32_t gen; ~AuxGuard() { aux_release(a, gen); } } aux_guard{ax, aux_gen};   // back to the pool on every way out
            AuxStream &t_aux = *ax;
            // the longest records first, on a second stream, beside the lane kernel
            HIP_TRY(hipEventRecord(t_aux.fork, st));
            HIP_TRY(hipStreamWaitEvent(t_aux.st, t_aux.fork, 0));
            hipLaunchKernelGGL(k_inflate_long, dim3(s5plan::long_grid(a->n_recs)), dim3(64), 0, t_aux.st, *a, ord);
            HIP_TRY(hipEventRecord(t_aux.join, t_aux.st));
            hipLaunchKernelGGL(k_inflate_simt<true>, dim3(nb64), dim3(64), 64 * sizeof(LaneTables), st, *a, ord);
            HIP_TRY(hipStreamWaitEvent(st, t_aux.join, 0));
        }
        break;
    }
    case s5plan::INFLATE_WAVE:
        hipLaunchKernelGGL(k_inflate, dim3(a->n_recs), dim3(64), 0, st, *a);
        break;
    }
    HIP_TRY(hipGetLastError());
    return S5GPU_OK;
}

static int dec_check(const s5gpu_decode_args_t *a, bool need_payload, bool need_sig) {
    if (!a || (a->n_recs && (!a->desc || !a->in || !a->fields || (need_payload && !a->payload) || (need_sig && !a->sig_out)))) return S5GPU_ERR_ARG;
    return S5GPU_OK;
}
extern "C" int s5gpu_inflate_dev(const s5gpu_decode_args_t *a, void *stream_) {
    if (dec_check(a, true, false)) { s5gpu_set_error("s5gpu_inflate_dev: bad arguments"); return S5GPU_ERR_ARG; }
    if (a->n_recs == 0) return S5GPU_OK;
    return launch_inflate(a, (hipStream_t)stream_);
}
extern "C" int s5gpu_inflate_head_dev(const s5gpu_decode_args_t *a, void *stream_) {
    if (dec_check(a, true, false) || (a && a->rec_method != S5GPU_REC_ZLIB)) { s5gpu_set_error("s5gpu_inflate_head_dev: bad arguments (zlib records)"); return S5GPU_ERR_ARG; }
    if (a->n_recs == 0) return S5GPU_OK;
    hipLaunchKernelGGL(k_inflate_head, dim3(a->n_recs), dim3(64), 0, (hipStream_t)stream_, *a);
    HIP_TRY(hipGetLastError());
    return S5GPU_OK;
}
extern "C" int s5gpu_svbzd_decode_dev(const s5gpu_decode_args_t *a, void *stream_) {
    if (dec_check(a, false, true)) { s5gpu_set_error("s5gpu_svbzd_decode_dev: bad arguments"); return S5GPU_ERR_ARG; }
    if (a->n_recs == 0) return S5GPU_OK;
    hipLaunchKernelGGL(k_svbzd_decode, dim3(a->n_recs), dim3(NT), 0, (hipStream_t)stream_, *a);
    HIP_TRY(hipGetLastError());
    return S5GPU_OK;
}

extern "C" uint64_t s5gpu_decode_scratch_bytes(uint32_t max_pay_cap) { return s5plan::np_scratch_bytes(max_pay_cap); }

// the no-payload kernel variants of s5gpu_decode_dev, by the index it computes: 0 .. 3 = zlib, svb-zd (0, 1) / ex-zd (2, 3) records with the long (even)
// / short (odd) waiting list; 5 = short svb-zd records kept in LDS; 4 = zstd, which takes one argument more and so has only an address here
using NpKernel = void (*)(s5gpu_decode_args_t, NpParams);
static NpKernel np_kernel(int variant) {
    switch (variant) {
    case 0: return k_inflate_par_np<false, false>;
    case 1: return k_inflate_par_np<false, true>;
    case 2: return k_inflate_par_np<true, false>;
    case 3: return k_inflate_par_np<true, true>;
    case 5: return k_inflate_par_np_lp;
    default: return nullptr;
    }
}
static const void *np_kernel_addr(int variant) {
    return variant == 4 ? reinterpret_cast<const void *>(k_zstd_inflate_np) : reinterpret_cast<const void *>(np_kernel(variant));
}

// fields + signals only (S5GPU_DEC_NO_PAYLOAD): persistent workgroups, one reused scratch slot each (k_inflate_par_np)
static int launch_no_payload(const s5gpu_decode_args_t *a, hipStream_t st) {
    if (!s5plan::np_served(a->rec_method, a->sig_method)) {
        s5gpu_set_error("s5gpu_decode_dev: S5GPU_DEC_NO_PAYLOAD serves zlib / zstd records with svb-zd signals and zlib records with ex-zd signals");
        return S5GPU_ERR_ARG;
    }
    if (!s5plan::np_args_ok(a->max_pay_cap, a->payload_bytes)) {
        s5gpu_set_error("s5gpu_decode_dev: S5GPU_DEC_NO_PAYLOAD needs max_pay_cap and at least 64 + 2 * (max_pay_cap + 32) bytes of scratch");
        return S5GPU_ERR_ARG;
    }
    const bool zl = a->rec_method == S5GPU_REC_ZLIB;
    const int variant = s5plan::np_variant(a->rec_method, a->sig_method, a->max_pay_cap, a->max_in_len, g_np_lds_payload);
    // the workgroups the device holds at once, asked for the template variant that is launched (the two waiting-list sizes differ in LDS: 24 and 21 waves per CU)
    DeviceFacts *facts = device_facts();
    uint32_t res = facts ? facts->np_resident[variant].load(std::memory_order_relaxed) : 0;
    if (!res) {
        int per_cu = 0, cus = 0;
        { const int rc = device_cus(&cus); if (rc) return rc; }
        HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, np_kernel_addr(variant), 64, 0));
        res = (uint32_t)(per_cu > 0 && cus > 0 ? per_cu * cus : 4096);
        if (facts) facts->np_resident[variant].store(res, std::memory_order_relaxed);
    }
    const s5plan::NpShape shape = s5plan::np_shape(a->rec_method, a->max_pay_cap, a->payload_bytes, res, a->n_recs);
    NpParams np;
    std::unique_lock<std::mutex> hold;
    np.ticket = shape.ticket ? reinterpret_cast<uint32_t *>(a->payload) : nullptr;
    np.scratch = a->payload + 64;
    np.slot = (uint32_t)s5plan::np_slot(a->max_pay_cap);
    np.cap = np.slot - 16;
    np.first_fb = (uint32_t)shape.n_main;
    np.ord = nullptr;
    if (shape.ticket) {
        HIP_TRY(hipMemsetAsync(a->payload, 0, 64, st));
        if (zl) { const int rc = s5kern_decode_order(a, st, &np.ord, hold); if (rc) return rc; }     // tickets in the order of the list: the longest records first
    }
    if (zl) {
        hipLaunchKernelGGL(np_kernel(variant), dim3((uint32_t)shape.n_main), dim3(64), 0, st, *a, np);
        hipLaunchKernelGGL(k_inflate_fallback_np, dim3((uint32_t)shape.n_fb), dim3(64), 0, st, *a, np);
    } else {
        uint32_t *ws32 = nullptr;
        const uint32_t *none = nullptr;
        { const int rc = s5kern_decode_order(a, st, &none, hold, s5plan::zstd_pre_words(a->n_recs, g_zstd_pre_min), &ws32, false); if (rc) return rc; }
        uint8_t *ws = reinterpret_cast<uint8_t *>(ws32);
        if (ws) hipLaunchKernelGGL(k_zstd_weights, dim3(s5plan::lane_grid(a->n_recs)), dim3(64), 0, st, *a, ws);
        hipLaunchKernelGGL(k_zstd_inflate_np, dim3((uint32_t)shape.n_main), dim3(64), 0, st, *a, np, ws);
    }
    HIP_TRY(hipGetLastError());
    return S5GPU_OK;
}

extern "C" int s5gpu_decode_dev(const s5gpu_decode_args_t *a, void *stream_) {
    if (dec_check(a, true, true)) {
        s5gpu_set_error("s5gpu_decode_dev: bad arguments");
        return S5GPU_ERR_ARG;
    }
    if (!s5rules::methods_ok(a->rec_method, a->sig_method)) { s5gpu_set_error("s5gpu_decode_dev: unsupported method"); return S5GPU_ERR_ARG; }
    if (a->n_recs == 0) return S5GPU_OK;
    hipStream_t st = (hipStream_t)stream_;
    if (a->flags & S5GPU_DEC_NO_PAYLOAD) return launch_no_payload(a, st);
    const int fused = s5plan::fused_unpack(a->rec_method, a->sig_method, g_unpack_fused, g_inflate_par);
    int rc = launch_inflate(a, st, fused);
    if (rc) return rc;
    // the workgroup form of the ex-zd decoder keeps one chunk of exceptions and a flag map in (dynamic) LDS; the other signal formats need none
    const size_t xlds = a->sig_method == S5GPU_SIG_EX_ZD ? sizeof(ExzdScratch) : 0;
    if (fused) hipLaunchKernelGGL(k_unpack_rest, dim3(s5plan::unpack_rest_grid(a->n_recs)), dim3(NT), xlds, st, *a);
    else hipLaunchKernelGGL(k_unpack, dim3(a->n_recs), dim3(NT), xlds, st, *a);
    HIP_TRY(hipGetLastError());
    return S5GPU_OK;
}

// variant builds of tools/ only: the phase clocks of a decoder, read and cleared
template <size_t N>
static int probe_read(unsigned long long (&clocks)[N], unsigned long long *out) {
    unsigned long long z[N] = {0};
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(clocks), sizeof z) != hipSuccess) return S5GPU_ERR_HIP;
    if (hipMemcpyToSymbol(HIP_SYMBOL(clocks), z, sizeof z) != hipSuccess) return S5GPU_ERR_HIP;
    return S5GPU_OK;
}
#ifdef S5_IPROBE   // tools/inflate_phases.py (inflate_par_dev.h)
extern "C" int s5gpu_iprobe_read(unsigned long long *out20) { return probe_read(s5::g_iprobe, out20); }
#endif
#ifdef S5_ZPROBE   // tools/zstd_phases.py (zstd_dev.h)
extern "C" int s5gpu_zprobe_read(unsigned long long *out16) { return probe_read(s5::g_zprobe, out16); }
#endif
