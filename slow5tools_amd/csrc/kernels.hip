// kernels.hip — gfx950 (CDNA4) kernels of the BLOW5 record press path + their launchers.
// One read per workgroup (4 x wave64); all intermediates of a read live in LDS; HBM sees the int16
// samples once (coalesced 16-B loads) and the finished record once (coalesced word stores).
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <mutex>
#include <type_traits>
#include <vector>

#include "../../include/slow5gpu.h"
#include "deflate_dev.h"
#include "lz_dev.h"
#include "inflate_dev.h"
#include "inflate_simt_dev.h"
#include "inflate_par_dev.h"
#include "zstd_dev.h"
#include "zstd_enc_dev.h"
#include "svb_dev.h"
#include "exzd_dev.h"
#include "order_dev.h"
#include "event_dev.h"
#include "enc_plan.h"

using namespace s5;

extern "C" void s5gpu_set_error(const char *fmt, ...);
int s5host_set_option(const char *key, long value);   // host_api.hip: options of the host layer
namespace fsk { int set_option(const char *key, long value); }   // fstats_kernels.hip: the file statistics' window, bins and flush point
namespace dfk { int set_option(const char *key, long value); }   // diff_kernels.hip: the difference histogram's window, flush point and grid
namespace dtwk { int path_set_option(const char *key, long value); }   // dtw_path_api.hip: which passes the path call launches
namespace pilek { int set_option(const char *key, long value); }   // pileup_kernels.hip: the pileup's LDS windows, grids, segments, sort and passes
namespace pilek { int hist_set_option(const char *key, long value); }   // contrast_kernels.hip: the level histograms' window and grid
namespace pilek { int site_set_option(const char *key, long value); }   // sites_kernels.hip: which passes the site call launches
namespace refk { int long_set_option(const char *key, long value); }   // refine_long_kernels.hip: which passes the whole-read refine launches
namespace bandk { int set_option(const char *key, long value); }   // band_kernels.hip: which passes the band call launches
extern uint32_t s5host_generation;                    // host_api.hip: bumped by s5gpu_shutdown
static_assert(s5plan::BLK == (uint32_t)DEFL_BLK && s5plan::SIG_SVB_ZD == S5GPU_SIG_SVB_ZD && s5plan::SIG_EX_ZD == S5GPU_SIG_EX_ZD, "enc_plan.h restates these");

#define HIP_TRY(x)                                                                                   \
    do {                                                                                             \
        hipError_t e_ = (x);                                                                         \
        if (e_ != hipSuccess) {                                                                      \
            s5gpu_set_error("%s failed: %s (%s:%d)", #x, hipGetErrorString(e_), __FILE__, __LINE__); \
            return S5GPU_ERR_HIP;                                                                    \
        }                                                                                            \
    } while (0)

extern __shared__ __attribute__((aligned(16))) uint8_t smem[];

constexpr uint32_t S_BYTES = (sizeof(DeflShared) + 15u) & ~15u;
constexpr uint32_t BZ_BYTES = (sizeof(BuildScratch) + 15u) & ~15u;   // deflate_block (round 1-4) and the zstd encoder overlay their build scratch on the bit buffer
constexpr uint32_t B_BYTES = NW * 288u * 4u + 64u;                   // deflate_block2 keeps one histogram per wave in the bit buffer's tail
constexpr uint32_t OVF = 0xFFFFFFFFu;

struct EncParams {
    s5gpu_encode_args_t a;
    uint32_t obuf_words;   // LDS words of the bit buffer
    uint32_t pay_cap;      // LDS bytes of the payload buffer (fused) / staging buffer (staged)
    uint32_t dbg;          // tools/ only (env S5GPU_DEBUG_STAGE): 1 = stop after the payload is built
    uint32_t zseq;         // zstd records: runs as sequences (option "zstd_sequences", default 1; 0 = the literals-only frames of round 1)
    uint32_t tier = 0;     // k_encode_fused: 0 = the only fused launch (a read that does not fit goes on the overflow list); 1 = the first of two (it is
                           // left alone: out_len[r] stays 0); 2 = the second, with a larger LDS budget (reads the first one did are skipped, a read
                           // that does not fit this budget either goes on the list)
};

static uint32_t g_fused_tier2 = 0;      // mixed batches (a caller-named fused budget): LDS budget of a SECOND fused launch (option "fused_tier2"; 0 = one launch, the default:
                                        // measured on the mixed leg, profiles/r04_mixed_tier2.txt — 16 KiB 393 GB/s, 12 KiB 408, one launch 405)
static uint32_t g_zstd_sequences = 1;   // zstd encoder: runs as sequences (zstd_enc_dev.h); 0 = literals-only frames (option "zstd_sequences")

__device__ __forceinline__ uint32_t payload_bound_dev(const s5gpu_read_desc_t &d, int sig_method) {
    const uint32_t n = d.n_samples;
    const uint32_t sig = sig_method == S5GPU_SIG_SVB_ZD ? 4 + ((n + 3) >> 2) + 3 * n
                       : sig_method == S5GPU_SIG_EX_ZD ? 24 + 2 * (((n + 3) >> 2) + 4 * n) + n : 2 * n;   // ex-zd: oracle/exzd.c s5o_exzd_bound
    return d.hdr_len + 8 + sig + d.aux_len;
}

// ------------------------------------------------------------------------------------------------
// payload = hdr | u64 L | signal bytes | aux   (slow5_rec_to_mem's uncompressed record, a4 in SURVEY §8)
// dst may be LDS (fused kernel) or HBM (staged path / no record compression).  cap = bytes dst can
// take; returns OVF (uniform, nothing useful written) if the payload would not fit.
// ------------------------------------------------------------------------------------------------
// EXZD is a compile-time switch: the ex-zd builder lives in its own kernel instantiations, so the svb-zd kernels the
// headline runs on carry none of its code (1 % of their time when it was a run-time branch).
template <bool EXZD = false>
__device__ __forceinline__ uint32_t build_payload(const s5gpu_encode_args_t &a, const s5gpu_read_desc_t &d,
                                                  uint8_t *pay, uint32_t cap, uint32_t *ws, uint32_t *red = nullptr) {
    const int tid = threadIdx.x;
    const uint32_t n = d.n_samples;
    if constexpr (EXZD) {   // red: 8 words of reduction scratch
        const uint32_t fixed_x = d.hdr_len + 8 + d.aux_len;
        if (fixed_x + 16 > cap) return OVF;
        const uint8_t *hdr = a.hdr + d.hdr_off;
        for (uint32_t i = tid; i < d.hdr_len; i += NT) pay[i] = hdr[i];
        uint8_t *lenp = pay + d.hdr_len;
        const uint32_t blen = exzd_encode_wg(a.sig + d.sig_off, n, lenp + 8, ws, red, cap - fixed_x);
        if (blen == EXZD_ERR) return OVF;
        if (tid < 8) lenp[tid] = tid < 4 ? (uint8_t)(blen >> (8 * tid)) : 0;
        if (d.aux_len) {
            const uint8_t *aux = a.aux + d.aux_off;
            uint8_t *ap = lenp + 8 + blen;
            for (uint32_t i = tid; i < d.aux_len; i += NT) ap[i] = aux[i];
        }
        return d.hdr_len + 8 + blen + d.aux_len;
    } else {
    const bool svb = a.sig_method == S5GPU_SIG_SVB_ZD;
    const uint32_t nk = (n + 3) >> 2;
    const uint32_t fixed = d.hdr_len + 8 + (svb ? 4 + nk : 0) + d.aux_len;   // everything but the data bytes
    if (fixed > cap || (svb ? n : 2 * n) > cap - fixed) return OVF;             // cannot fit even at 1 byte/sample
    const uint8_t *hdr = a.hdr + d.hdr_off;
    for (uint32_t i = tid; i < d.hdr_len; i += NT) pay[i] = hdr[i];
    uint8_t *lenp = pay + d.hdr_len;
    uint8_t *sigp = lenp + 8;
    const int16_t *sig = a.sig + d.sig_off;
    uint64_t L;
    uint32_t sig_bytes;
    if (svb) {
        uint8_t *keys = sigp + 4;
        uint8_t *data = keys + nk;
        uint32_t total = 0;
        const uint32_t room = cap - fixed;
        for (uint32_t t0 = 0; t0 < n; t0 += SVB_TILE) {
            const uint32_t t = svb_encode_tile(sig, n, t0, keys + (t0 >> 2), data + total, ws, room - total, true);   // (one read per workgroup: ws is fresh)
            if (t > room - total) return OVF;
            total += t;
        }
        L = 4ull + nk + total;
        sig_bytes = (uint32_t)L;
        if (tid < 4) sigp[tid] = (uint8_t)(n >> (8 * tid));
    } else {
        L = n;
        sig_bytes = 2 * n;
        const uint8_t *src = reinterpret_cast<const uint8_t *>(sig);
        for (uint32_t i = tid; i < sig_bytes; i += NT) sigp[i] = src[i];
    }
    if (tid < 8) lenp[tid] = (uint8_t)(L >> (8 * tid));
    if (d.aux_len) {
        const uint8_t *aux = a.aux + d.aux_off;
        uint8_t *ap = sigp + sig_bytes;
        for (uint32_t i = tid; i < d.aux_len; i += NT) ap[i] = aux[i];
    }
    return d.hdr_len + 8 + sig_bytes + d.aux_len;
    }
}

// The same payload written to HBM (staged path, record compression "none").  The svb-zd bytes of a tile are assembled in
// LDS and leave as aligned dwords: byte-granular stores straight to HBM cost 2.5x the time of the fused kernel's svb stage.
__device__ __forceinline__ uint32_t build_payload_hbm(const s5gpu_encode_args_t &a, const s5gpu_read_desc_t &d, uint8_t *pay,
                                                      uint32_t *ws, uint32_t *tile_keys, uint32_t *tile_data) {
    const int tid = threadIdx.x;
    const uint32_t n = d.n_samples;
    if (a.sig_method == S5GPU_SIG_EX_ZD) return build_payload<true>(a, d, pay, OVF - 1, ws, tile_keys /* 8 words of reduction scratch */);
    if (a.sig_method != S5GPU_SIG_SVB_ZD) return build_payload(a, d, pay, OVF - 1, ws);
    const uint32_t nk = (n + 3) >> 2;
    const uint8_t *hdr = a.hdr + d.hdr_off;
    for (uint32_t i = tid; i < d.hdr_len; i += NT) pay[i] = hdr[i];
    uint8_t *lenp = pay + d.hdr_len;
    uint8_t *sigp = lenp + 8;
    const int16_t *sig = a.sig + d.sig_off;
    uint8_t *keys = sigp + 4;
    uint8_t *data = keys + nk;
    uint32_t total = 0;
    for (uint32_t t0 = 0; t0 < n; t0 += SVB_TILE) {
        const uint32_t t = svb_encode_tile(sig, n, t0, reinterpret_cast<uint8_t *>(tile_keys), reinterpret_cast<uint8_t *>(tile_data), ws, OVF - 1);
        __syncthreads();
        const uint32_t tk = (min(n - t0, (uint32_t)SVB_TILE) + 3) >> 2;
        copy_record_out(tile_keys, tk, keys + (t0 >> 2));
        copy_record_out(tile_data, t, data + total);
        total += t;
        __syncthreads();
    }
    const uint64_t L = 4ull + nk + total;
    if (tid < 4) sigp[tid] = (uint8_t)(n >> (8 * tid));
    if (tid < 8) lenp[tid] = (uint8_t)(L >> (8 * tid));
    if (d.aux_len) {
        const uint8_t *aux = a.aux + d.aux_off;
        uint8_t *ap = sigp + (uint32_t)L;
        for (uint32_t i = tid; i < d.aux_len; i += NT) ap[i] = aux[i];
    }
    return d.hdr_len + 8 + (uint32_t)L + d.aux_len;
}

// bytes at the front of a read's payload that are run-heavy (head + svb key area: mostly zero bytes): the block encoder's hint for how to
// cut a block among its waves (deflate2_dev.h)
__device__ __forceinline__ uint32_t run_heavy_front(const s5gpu_encode_args_t &a, const s5gpu_read_desc_t &d) {
    return a.sig_method == S5GPU_SIG_SVB_ZD ? d.hdr_len + 12u + ((d.n_samples + 3u) >> 2) : 0u;
}

// The fused kernels take the hint as the staged one does.  (History: with the round-4 barrier count it cost them 1 % — 13.42 ms per 1 M
// 4000-sample reads against 13.30, eight workgroups per CU filling a wave's idle time —; after this round's barrier cuts the waves' balance
// is what is left: 12.71 -> 11.94 ms.  Weight of a general slab 2 / 3 / 4 / 5 / 6 / 8: 12.24 / 11.91 / 11.94 / 12.01 / 12.05 / 12.49.)
#ifndef S5_FUSED_HINT
#define S5_FUSED_HINT(a, d) run_heavy_front(a, d)
#endif

// K1+K5+K3+K6 fused: svb-zd -> pack -> one DEFLATE block -> zlib frame.  One read per workgroup, every
// intermediate in LDS.  A read whose payload does not fit the LDS budget (p.pay_cap: long read, or an
// unusually incompressible signal) is appended to the overflow list and redone by the staged kernels.
#ifndef S5_FUSED_WG_PER_CU
#define S5_FUSED_WG_PER_CU 8
#endif
template <typename M, bool EXZD = false, int WPS = S5_FUSED_WG_PER_CU>   // WPS: waves per SIMD the registers are budgeted for (the second fused launch of a
__global__ __launch_bounds__(NT, WPS) void k_encode_fused(EncParams p) {     // mixed batch holds 36 KiB of LDS: four workgroups per CU, so 128 VGPRs)
    const uint32_t r = blockIdx.x;
    if (p.tier == 2 && p.a.out_len[r] != 0) return;   // (uniform) done by the first launch
    DeflShared &S = *reinterpret_cast<DeflShared *>(smem);
    uint32_t *obuf = reinterpret_cast<uint32_t *>(smem + S_BYTES);
    uint8_t *pay = smem + S_BYTES + 4u * p.obuf_words;
    const s5gpu_read_desc_t d = p.a.desc[r];
    deflate2_prepare<NT>(S, obuf, p.obuf_words);     // (cleared under the signal loads; ordered by the barriers of the payload's scans)
    const uint32_t plen = build_payload<EXZD>(p.a, d, pay, p.pay_cap, S.ws, S.red);
    if (plen == OVF) {
        if (threadIdx.x == 0 && p.tier != 1) {
            const uint32_t at = atomicAdd(&p.a.ovf[0], 1u);
            p.a.ovf[1 + at] = r;
        }
        return;
    }
    __syncthreads();
    if (p.dbg == 1) {   // stage-timing aid: svb-zd + pack only
        if (threadIdx.x == 0) p.a.out_len[r] = plen + pay[plen - 1];
        return;
    }
    uint8_t *out = p.a.slots + d.out_off;
    const uint32_t total = zlib_compress_fused<M>(S, obuf, p.obuf_words, pay, plen, out, p.dbg, S5_FUSED_HINT(p.a, d), true);
    if (threadIdx.x == 0) p.a.out_len[r] = total;
}

// The same with ORDERED SINGLE-PASS OUTPUT: no slots, no compaction pass.  Reads are taken in ticket (start) order;
// once a record's size is known its byte offset in the contiguous BLOW5 record stream comes from a decoupled
// look-back over the sizes of the preceding reads, and the record goes straight from LDS to its final place.
// ctl: [0] overflow count (a read that does not fit the LDS budget cannot be placed: the caller must fall back
// to s5gpu_encode_dev + s5gpu_compact_dev), [1] ticket counter, [2] look-back timeout flag.
#ifndef S5_LB_E
#define S5_LB_E 1
#endif
struct StreamParams {
    unsigned long long *state;   // n_reads words, zeroed
    uint32_t *ctl;               // 4 words, zeroed
    uint8_t *stream;
    uint64_t *rec_off;           // n_reads + 1
};
template <typename M, bool EXZD = false>
__global__ __launch_bounds__(NT, S5_FUSED_WG_PER_CU) void k_encode_stream(EncParams p, StreamParams sp) {
    __shared__ uint32_t s_r;
    __shared__ uint64_t s_off;
    DeflShared &S = *reinterpret_cast<DeflShared *>(smem);
    uint32_t *obuf = reinterpret_cast<uint32_t *>(smem + S_BYTES);
    uint8_t *pay = smem + S_BYTES + 4u * p.obuf_words;
#ifdef S5_ES_NOTICKET   // tools: what the ticket counter costs (dispatch order is not a guarantee)
    const uint32_t r = blockIdx.x;
#else
    if (threadIdx.x == 0) s_r = atomicAdd(&sp.ctl[1], 1u);
    __syncthreads();
    const uint32_t r = s_r;
#endif
    const s5gpu_read_desc_t d = p.a.desc[r];
    deflate2_prepare<NT>(S, obuf, p.obuf_words);     // (cleared under the signal loads; ordered by the barriers of the payload's scans)
    const uint32_t plen = build_payload<EXZD>(p.a, d, pay, p.pay_cap, S.ws, S.red);
    uint32_t total = 0;
    if (plen == OVF) {
        if (threadIdx.x == 0) atomicAdd(&sp.ctl[0], 1u);   // size 0 keeps the chain alive; the stream is invalid
    } else {
        __syncthreads();
        ZOut z;
        total = zlib_frame_fused<M>(S, obuf, p.obuf_words, pay, plen, z, 0, EarlySize{sp.state, r}, S5_FUSED_HINT(p.a, d), true);
        if (threadIdx.x == 0) { obuf[0] = total - 8; obuf[1] = 0; }   // u64 size prefix
    }
    if (wave_id() == 0) {
        const uint64_t off = lookback_offset<S5_LB_E>(sp.state, r, total, &sp.ctl[2], plen != OVF);
        if (lane_id() == 0) {
            s_off = off;
            sp.rec_off[r] = off;
            if (r == p.a.n_reads - 1) sp.rec_off[p.a.n_reads] = off + total;
            p.a.out_len[r] = total;
        }
    }
    __syncthreads();
    if (total) copy_record_out(obuf, total, sp.stream + s_off);
}

// Staged path works IN PLACE in the read's slot: the payload is parked at the slot's tail
// (offset slot_cap - payload_bound, 16-B aligned) and the zlib stream grows from the slot's head.  The
// slot bound leaves more room than the worst-case (all-stored) framing overhead, and each 16 KiB block
// is in LDS before its output is written, so the writer never catches the reader.
__device__ __forceinline__ uint32_t park_offset(const s5gpu_read_desc_t &d, int sig_method) {
    return (d.slot_cap - payload_bound_dev(d, sig_method)) & ~15u;
}

// Staged path, step 1: payload straight to HBM.  mode 0: all reads, parked for k_deflate_staged;
// mode 1: record compression "none" — the payload IS the record: [u64 size][payload] at the slot head;
// mode 2: like 0 but only the reads on the overflow list.
#ifndef S5_PACK_WG
#define S5_PACK_WG 8      // (round 3, measured on the long-read leg: 4 / 5 / 6 / 8 workgroups per CU = 23.3 / 22.4 / 22.1 / 22.0 ms)
#endif
__global__ __launch_bounds__(NT, S5_PACK_WG) void k_pack(EncParams p, int mode, const uint32_t *ord) {
    __shared__ uint32_t ws[16];
    __shared__ __attribute__((aligned(16))) uint32_t tile_keys[SVB_TILE / 16 + 4];       // one tile's key bytes (4096 / 4) ...
    __shared__ __attribute__((aligned(16))) uint32_t tile_data[3 * SVB_TILE / 4 + 4];    // ... and data bytes (at most 3 per int16 sample), + the copy's slack
    const uint32_t count = mode == 2 ? p.a.ovf[0] : p.a.n_reads;
    for (uint32_t it = blockIdx.x; it < count; it += gridDim.x) {
        const uint32_t r = mode == 2 ? ovf_at(p.a.ovf, ord, it) : it;
        const s5gpu_read_desc_t d = p.a.desc[r];
        uint8_t *dst = p.a.slots + d.out_off + (mode == 1 ? 8u : park_offset(d, p.a.sig_method));
        const uint32_t plen = build_payload_hbm(p.a, d, dst, ws, tile_keys, tile_data);
        if (threadIdx.x == 0) {
            if (mode == 1) {
                *reinterpret_cast<uint64_t *>(p.a.slots + d.out_off) = plen;
                p.a.out_len[r] = plen + 8;
            } else {
                p.a.out_len[r] = plen;   // payload length, consumed by k_deflate_staged
            }
        }
        __syncthreads();
    }
}

// Staged path, step 2: DEFLATE a parked payload, 16 KiB block at a time through LDS, in place in the read's slot.  Returns the record's
// length (u64 prefix included; uniform); the prefix and out_len[r] are written here.
// Threads of the staged kernel's workgroup.  Its LDS — a 16 KiB block, the block's bit buffer, the tables — allows four workgroups per CU, 16 waves at
// 256 threads where the same code in the fused kernel needs 32; round 4 made deflate_block a template on the thread count and measured 512 (a lane owns
// 32 bytes: 32-bit masks, byte loads, the fused kernel's shape): 64 VGPRs with 51 of them spilled (the block loop's state on top of the fused kernel's),
// and the long-read leg takes 26.9 ms per step against 21.5 (80 VGPRs / 24 waves: 27.7) — profiles/r04_staged_threads.txt.  256 stays.
#ifndef S5_STAGED_TN
#define S5_STAGED_TN 256
#endif
// the next 16 KiB block of a parked payload on its way HBM -> registers (64 bytes per lane at 256 threads)
struct StagedPf { uint4 v[DEFL_BLK / 16 / S5_STAGED_TN]; };
__device__ __forceinline__ void staged_fetch(StagedPf &pf, const uint8_t *src, uint32_t at, uint32_t plen) {
    const uint32_t bl = min(plen - at, (uint32_t)DEFL_BLK);
    const uint4 *s4 = reinterpret_cast<const uint4 *>(src + at);
#pragma unroll
    for (int j = 0; j < DEFL_BLK / 16 / S5_STAGED_TN; j++) {
        const uint32_t i = threadIdx.x + j * S5_STAGED_TN;
        pf.v[j] = i < (bl + 15) / 16 ? s4[i] : uint4{0u, 0u, 0u, 0u};
    }
}
// pf: this record's first block, already on its way; next_src / next_plen: the record this workgroup takes next (nullptr: none) — its first
// block is fetched under this record's last one
__device__ __forceinline__ uint32_t deflate_staged_record(const EncParams &p, uint32_t r, const s5gpu_read_desc_t &d, uint32_t plen, DeflShared &S, uint32_t *obuf, BuildScratch &B, uint8_t *stage,
                                                          StagedPf &pf, const uint8_t *next_src, uint32_t next_plen) {
    const int tid = threadIdx.x;
    uint8_t *out = p.a.slots + d.out_off;
    const uint8_t *src = out + park_offset(d, p.a.sig_method);
    __syncthreads();
    ZOut z;
    z.bitpos = 80;        // u64 size prefix (words 0, 1: written last) + CMF/FLG 78 9c
    z.flushed = 2;        // obuf[0] = stream word 2
    z.carry = 0x9c78u;
    uint32_t adA = 1, adB = 0, done = 0;
    uint32_t *out32 = reinterpret_cast<uint32_t *>(out);
    // Round 5: the NEXT block travels HBM -> registers while this one is encoded (16 KiB = 64 bytes per lane), and goes to LDS when the block
    // buffer is free again: at four workgroups per CU nothing else hides the load.  (Reading ahead is safe in place: the stream only ever
    // overwrites payload that is already in LDS or in these registers.)
    constexpr int NPF = DEFL_BLK / 16 / S5_STAGED_TN;
    do {
        const uint32_t blen = min(plen - done, (uint32_t)DEFL_BLK);
        const bool final = done + blen == plen;
        {   // registers -> LDS, 16 B per lane (park offset and block offsets are 16-B aligned)
            uint4 *d4 = reinterpret_cast<uint4 *>(stage);
#pragma unroll
            for (int j = 0; j < NPF; j++) { const uint32_t i = tid + j * S5_STAGED_TN; if (i < (blen + 15) / 16) d4[i] = pf.v[j]; }
        }
        if (!final) staged_fetch(pf, src, done + blen, plen);
        else if (next_src) staged_fetch(pf, next_src, 0, next_plen);
        __syncthreads();
        const uint32_t front = run_heavy_front(p.a, d);
        deflate_block2<2, S5_STAGED_TN>(S, obuf, p.obuf_words, stage, (int)blen, final, z, adA, adB, 0, EarlySize{nullptr, 0},
                                        front > done ? min(front - done, blen) : 0u);
        done += blen;
        if (!final) {
            // deflate_block2 clears the bit buffer itself and takes the pending partial word from z.carry: the completed words go out,
            // the partial one is read where it stands — one barrier instead of four and no slide
            const uint32_t full = z.bitpos >> 5;
            flush_words<S5_STAGED_TN>(obuf, out32, z, true, full - z.flushed);
            z.carry = obuf[full - z.flushed];      // uniform
            z.flushed = full;
            __syncthreads();        // ... before the next block's histograms overwrite the buffer's tail
        }
    } while (done < plen);
    z.bitpos = (z.bitpos + 7) & ~7u;
    if (tid == 0) put_bits(obuf, z, z.bitpos, __builtin_bswap32((adB << 16) | adA), 32);
    z.bitpos += 32;
    __syncthreads();
    flush_words<S5_STAGED_TN>(obuf, out32, z, true);
    const uint32_t total = z.bitpos >> 3;
    __syncthreads();
    if (tid == 0) {
        *reinterpret_cast<uint64_t *>(out) = (uint64_t)(total - 8);
        p.a.out_len[r] = total;
    }
    return total;
}
#ifndef S5_STAGED_WG
#define S5_STAGED_WG (S5_STAGED_TN >= 512 ? 8 : 4)   // (the second launch bound counts WAVES PER SIMD: four workgroups of 512 threads per CU are eight)
#endif
__global__ __launch_bounds__(S5_STAGED_TN, S5_STAGED_WG) void k_deflate_staged(EncParams p, int use_list, const uint32_t *ord) {
    DeflShared &S = *reinterpret_cast<DeflShared *>(smem);
    uint32_t *obuf = reinterpret_cast<uint32_t *>(smem + S_BYTES);
    BuildScratch &B = *reinterpret_cast<BuildScratch *>(obuf);   // dead whenever the bit buffer is live (deflate_block MODE 2)
    uint8_t *stage = smem + S_BYTES + 4u * p.obuf_words;
    const uint32_t count = use_list ? p.a.ovf[0] : p.a.n_reads;
    // (Fetching the NEXT record's first block under this record's last one was measured too: the second descriptor's registers push the kernel
    // into scratch — 6 VGPRs and 100 SGPRs spilled — and the mixed leg falls from 500 to 485 GB/s.)
    for (uint32_t it = blockIdx.x; it < count; it += gridDim.x) {
        const uint32_t r = use_list ? ovf_at(p.a.ovf, ord, it) : it;
        const s5gpu_read_desc_t d = p.a.desc[r];
        const uint32_t plen = p.a.out_len[r];
        StagedPf pf;
        staged_fetch(pf, p.a.slots + d.out_off + park_offset(d, p.a.sig_method), 0, plen);
        deflate_staged_record(p, r, d, plen, S, obuf, B, stage, pf, nullptr, 0);
    }
}
// (Round 3 tried steps 1 + 2 in ONE workgroup — park the read's payload, barrier, deflate it from there — so that the streaming of one read
// would run under the arithmetic of the others: 23.1 ms per long-read step against 21.7 for the two launches.  At this kernel's 128 VGPRs /
// four workgroups per CU the streaming phase has half the waves k_pack runs with, and what it gains in overlap it loses there.)
// (Round 3 tried ORDERED SINGLE-PASS OUTPUT here as well — tickets, compress in place, publish the size, look-back, move the record to its
// place in the stream, no compaction launch: correct, and 32.3 ms per long-read step against 21.8 + 2.5 for this kernel + k_compact.  A long
// record's size is only known when it is finished, so a workgroup waits for EVERY predecessor of its dispatch wave to finish before it may
// move its record and retire: the spread of completion times becomes idle CUs.  k_encode_stream can publish a size before it packs.)

// Staged path with the LZ77 matcher (lz_dev.h): records whose signal press is "none" (raw int16 samples) and byte ranges of the
// solo zlib press.  LzLong: the parked payload goes through LDS 16 KiB at a time like k_deflate_staged; the previous block stays in
// LDS as the matcher's history, and so does the table of recent positions: one workgroup per CU (150 KiB of LDS).  LzShort: payloads of
// at most 8 KiB (one block, no history, the bit buffer in the table's storage): 38 KiB, four workgroups per CU.  which: 0 = every
// record (LzLong only), 1 = this kernel's share of a batch that runs both (LzShort: payloads <= 8 KiB, LzLong: the others).
constexpr uint32_t LZ_BYTES = (sizeof(LzSharedT<LzLong>) + 15u) & ~15u;
constexpr uint32_t LZS_BYTES = (sizeof(LzSharedT<LzShort>) + 15u) & ~15u;
static_assert(S_BYTES + (DEFL_BLK + 64) + LZ_BYTES <= 160u * 1024u - 256u, "the long shape holds a CU's LDS by itself");
// build = 1 (LzShort, a batch of short raw-signal records only): the payload head | u64 N | int16 samples | aux is put together right here
// in the window — no k_pack launch, no parked copy of the payload through HBM
template <class C>
__global__ __launch_bounds__(C::TN, C::HIST ? 1 : 4) void k_deflate_lz(EncParams p, int use_list, int which, int build) {
    DeflShared &S = *reinterpret_cast<DeflShared *>(smem);
    LzSharedT<C> &X = *reinterpret_cast<LzSharedT<C> *>(smem + S_BYTES + (C::HIST ? 4u * p.obuf_words : 0u));
    uint32_t *obuf = C::HIST ? reinterpret_cast<uint32_t *>(smem + S_BYTES) : X.obuf_alias;
    const uint32_t obuf_words = C::HIST ? p.obuf_words : (uint32_t)(C::BLK + 64) / 4u;
    const int tid = threadIdx.x;
    constexpr uint32_t TN = (uint32_t)C::TN;   // threads of this shape's workgroup (lz_dev.h)
    const uint32_t count = use_list ? p.a.ovf[0] : p.a.n_reads;
    for (uint32_t it = blockIdx.x; it < count; it += gridDim.x) {
        const uint32_t r = use_list ? p.a.ovf[1 + it] : it;
        const s5gpu_read_desc_t d = p.a.desc[r];
        // whose record: by the payload size the descriptor implies (signal press none: head + u64 + 2 bytes per sample + aux) — out_len[r]
        // turns from the payload's length into the record's when a kernel is done with it, so it cannot say
        if (which && (d.hdr_len + 8u + 2u * d.n_samples + d.aux_len <= (uint32_t)LzShort::BLK) != !C::HIST) continue;
        uint32_t plen = 0;
        if (!build) plen = p.a.out_len[r];
        if constexpr (!C::HIST) {
            // build mode assembles the payload in the 8 KiB window: a descriptor that implies more than the caller's max_payload promised
            // (s5gpu_encode_dev is a public call) must not overrun LDS — the read goes on the overflow list and the long shape redoes it
            if (build && d.hdr_len + 8u + 2u * d.n_samples + d.aux_len > (uint32_t)C::BLK) {
                if (tid == 0) { const uint32_t at = atomicAdd(&p.a.ovf[0], 1u); p.a.ovf[1 + at] = r; }
                continue;
            }
        }
        uint8_t *out = p.a.slots + d.out_off;
        const uint8_t *src = out + park_offset(d, p.a.sig_method);
        __syncthreads();
        if constexpr (!C::HIST) {
            if (build) {
                uint8_t *w8 = X.win;
                const uint8_t *hdr = p.a.hdr + d.hdr_off;
                for (uint32_t i = tid; i < d.hdr_len; i += TN) w8[i] = hdr[i];
                if (tid < 8) w8[d.hdr_len + tid] = (uint8_t)((uint64_t)d.n_samples >> (8 * tid));
                // samples: dword loads from the (16-byte aligned) signal, 16-bit stores (the head's 2 + id + 36 + 8 bytes leave the samples 2-byte aligned)
                const uint32_t *s32 = reinterpret_cast<const uint32_t *>(p.a.sig + d.sig_off);
                uint8_t *sp = w8 + d.hdr_len + 8;
                const bool al2 = ((d.hdr_len + 8u) & 1u) == 0;
                for (uint32_t i = tid; i < (d.n_samples + 1) / 2; i += TN) {
                    const uint32_t v = s32[i];
                    if (al2) {
                        reinterpret_cast<uint16_t *>(sp)[2 * i] = (uint16_t)v;
                        if (2 * i + 1 < d.n_samples) reinterpret_cast<uint16_t *>(sp)[2 * i + 1] = (uint16_t)(v >> 16);
                    } else {
                        sp[4 * i] = (uint8_t)v; sp[4 * i + 1] = (uint8_t)(v >> 8);
                        if (2 * i + 1 < d.n_samples) { sp[4 * i + 2] = (uint8_t)(v >> 16); sp[4 * i + 3] = (uint8_t)(v >> 24); }
                    }
                }
                if (d.aux_len) {
                    const uint8_t *aux = p.a.aux + d.aux_off;
                    uint8_t *ap = sp + 2 * d.n_samples;
                    for (uint32_t i = tid; i < d.aux_len; i += TN) ap[i] = aux[i];
                }
                plen = d.hdr_len + 8u + 2u * d.n_samples + d.aux_len;
            }
        }
        {   // a record starts with an empty table (the output must not depend on what this workgroup encoded before)
            uint4 *t4 = reinterpret_cast<uint4 *>(X.table);
            for (uint32_t i = tid; i < sizeof(X.table) / 16; i += TN) t4[i] = make_uint4(0, 0, 0, 0);
        }
        ZOut z;
        z.bitpos = 80;        // u64 size prefix (words 0, 1: written last) + CMF/FLG 78 9c
        z.flushed = 2;        // obuf[0] = stream word 2
        z.carry = 0x9c78u;
        uint32_t adA = 1, adB = 0, done = 0;
        uint32_t *out32 = reinterpret_cast<uint32_t *>(out);
        do {
            const uint32_t blen = min(plen - done, (uint32_t)C::BLK);
            const bool final = done + blen == plen;
            if (!build) {   // HBM -> LDS, 16 B per lane (park offset and block offsets are 16-B aligned)
                const uint4 *s4 = reinterpret_cast<const uint4 *>(src + done);
                uint4 *d4 = reinterpret_cast<uint4 *>(X.win + C::WOFF);
                for (uint32_t i = tid; i < (blen + 15) / 16; i += TN) d4[i] = s4[i];
            }
            __syncthreads();
            deflate_block_lz<C>(S, X, obuf, obuf_words, (int)blen, done ? (uint32_t)C::WOFF : 0u, done, final, z, adA, adB);
            done += blen;
            if (!final) {
                if constexpr (C::HIST) {
                    flush_words<C::TN>(obuf, out32, z, false);
                    z.carry = obuf[0];
                    const uint4 *c4 = reinterpret_cast<const uint4 *>(X.win + C::WOFF);   // the block becomes the next one's history
                    uint4 *h4 = reinterpret_cast<uint4 *>(X.win);
                    for (uint32_t i = tid; i < C::BLK / 16; i += TN) h4[i] = c4[i];
                    __syncthreads();
                }
            }
        } while (done < plen);
        z.bitpos = (z.bitpos + 7) & ~7u;
        if (tid == 0) put_bits(obuf, z, z.bitpos, __builtin_bswap32((adB << 16) | adA), 32);
        z.bitpos += 32;
        __syncthreads();
        flush_words<C::TN>(obuf, out32, z, true);
        const uint32_t total = z.bitpos >> 3;
        __syncthreads();
        if (tid == 0) {
            *reinterpret_cast<uint64_t *>(out) = (uint64_t)(total - 8);
            p.a.out_len[r] = total;
        }
    }
}

// zstd record press, fused: payload in LDS -> literals-only zstd frame (zstd_enc_dev.h).  Same shape as k_encode_fused.
template <bool EXZD>
#ifndef S5_ZF_WG
#define S5_ZF_WG 7      // (round 3, measured: 6 / 7 / 8 workgroups per CU = 8.10 / 7.43 / 7.62 ms per 262 k reads)
#endif
__global__ __launch_bounds__(NT, S5_ZF_WG) void k_zstd_fused(EncParams p) {
    const uint32_t r = blockIdx.x;
    if (p.tier == 2 && p.a.out_len[r] != 0) return;   // (uniform) done by the first launch
    DeflShared &S = *reinterpret_cast<DeflShared *>(smem);
    uint32_t *obuf = reinterpret_cast<uint32_t *>(smem + S_BYTES);
    uint8_t *pay = smem + S_BYTES + 4u * p.obuf_words;
    const s5gpu_read_desc_t d = p.a.desc[r];
    const uint32_t plen = build_payload<EXZD>(p.a, d, pay, p.pay_cap, S.ws, S.red);
    if (plen == OVF) {
        if (threadIdx.x == 0 && p.tier != 1) {
            const uint32_t at = atomicAdd(&p.a.ovf[0], 1u);
            p.a.ovf[1 + at] = r;
        }
        return;
    }
    __syncthreads();
    if (p.dbg == 9) { if (threadIdx.x == 0) p.a.out_len[r] = plen; return; }   // payload only
    uint32_t split = 0;   // literals-only frames of an svb-zd record: head + key bytes in a block of their own (with sequences the key bytes' runs are matches)
    if (!EXZD && !p.zseq && p.a.sig_method == S5GPU_SIG_SVB_ZD) {
        const uint32_t at = d.hdr_len + 12 + ((d.n_samples + 3) >> 2);
        if (at >= 256 && at + 256 <= plen && at <= (uint32_t)DEFL_BLK) split = at;
    }
    const uint32_t total = zstd_record<false>(S, obuf, p.obuf_words, pay, nullptr, plen, p.a.slots + d.out_off, p.dbg, split, split ? d.hdr_len + 12 : 0u, p.zseq != 0);
    if (threadIdx.x == 0) p.a.out_len[r] = total;
}
// ... and staged: a parked payload, 16 KiB block at a time through LDS (k_deflate_staged's twin)
#ifndef S5_ZS_WG
#define S5_ZS_WG 3
#endif
__global__ __launch_bounds__(NT, S5_ZS_WG) void k_zstd_staged(EncParams p, int use_list) {
    DeflShared &S = *reinterpret_cast<DeflShared *>(smem);
    uint32_t *obuf = reinterpret_cast<uint32_t *>(smem + S_BYTES);
    uint8_t *stage = smem + S_BYTES + 4u * p.obuf_words;
    const uint32_t count = use_list ? p.a.ovf[0] : p.a.n_reads;
    for (uint32_t it = blockIdx.x; it < count; it += gridDim.x) {
        const uint32_t r = use_list ? p.a.ovf[1 + it] : it;
        const s5gpu_read_desc_t d = p.a.desc[r];
        uint8_t *out = p.a.slots + d.out_off;
        const uint32_t plen = p.a.out_len[r];
        __syncthreads();
        const uint32_t total = zstd_record<true>(S, obuf, p.obuf_words, out + park_offset(d, p.a.sig_method), stage, plen, out, 0, 0, 0, p.zseq != 0);
        if (threadIdx.x == 0) p.a.out_len[r] = total;
    }
}

// K1 alone (BASELINE config 2): svb-zd blob of each read at slots + out_off.  The blob is assembled in LDS
// (p.pay_cap bytes) and leaves as coalesced 16-B stores; a read whose blob does not fit is written
// straight to HBM byte-wise (correct for any length, slower).
__global__ __launch_bounds__(NT) void k_svbzd_encode(EncParams p) {
    __shared__ uint32_t ws[16];
    const uint32_t r = blockIdx.x;
    const int tid = threadIdx.x;
    const s5gpu_read_desc_t d = p.a.desc[r];
    const int16_t *sig = p.a.sig + d.sig_off;
    uint8_t *blob = p.a.slots + d.out_off;
    const uint32_t n = d.n_samples, nk = (n + 3) >> 2;
    uint32_t total = 0;
    bool in_lds = (uint64_t)4 + nk + n <= p.pay_cap;
    if (in_lds) {
        uint8_t *keys = smem + 4, *data = keys + nk;
        const uint32_t room = p.pay_cap - 4 - nk;
        for (uint32_t t0 = 0; t0 < n; t0 += SVB_TILE) {
            const uint32_t t = svb_encode_tile(sig, n, t0, keys + (t0 >> 2), data + total, ws, room - total);
            if (t > room - total) { in_lds = false; break; }   // uniform
            total += t;
        }
    }
    if (in_lds) {
        if (tid < 4) smem[tid] = (uint8_t)(n >> (8 * tid));
        __syncthreads();
        const uint32_t len = 4 + nk + total;
        const uint4 *s4 = reinterpret_cast<const uint4 *>(smem);
        uint4 *d4 = reinterpret_cast<uint4 *>(blob);   // slot is 16-B aligned and has >= 16 spare bytes
        for (uint32_t i = tid; i < (len + 15) / 16; i += NT) d4[i] = s4[i];
        if (tid == 0) p.a.out_len[r] = len;
        return;
    }
    __syncthreads();
    uint8_t *keys = blob + 4, *data = keys + nk;
    total = 0;
    for (uint32_t t0 = 0; t0 < n; t0 += SVB_TILE) total += svb_encode_tile(sig, n, t0, keys + (t0 >> 2), data + total, ws, OVF);
    if (tid == 0) {
        *reinterpret_cast<uint32_t *>(blob) = n;
        p.a.out_len[r] = 4 + nk + total;
    }
}

// K1 with ORDERED SINGLE-PASS OUTPUT (round 3): blobs are assembled in LDS as in k_svbzd_encode, their lengths are known there, a decoupled
// look-back (tickets = start order, as k_encode_stream) gives their place in the contiguous blob stream, and they leave LDS for that
// place: 2N read + S written, against 2N + S + (S read + S written) of slots + compaction.
// A workgroup takes S5_SVS_G consecutive reads per ticket and holds all their blobs in LDS, back to back as they will lie in the stream,
// before it looks back: one ticket, one state word and one copy per group.  (One read per workgroup ran at 11.5 ms per 1 M reads against
// 3.1 without ticket and look-back: a million atomics on ONE counter take 8 ms on this part whatever else the kernel does — the full
// encoder takes its million tickets over 13.7 ms and loses 0.3 ms to them.  Reads of a group done one after the other, each with its
// own look-back, chain the workgroups instead: a group's first read would wait for the previous group's last.)
#ifndef S5_SVS_G
#define S5_SVS_G 4
#endif
#ifndef S5_SVS_E
#define S5_SVS_E 1
#endif
#ifndef S5_SVS_WG
#define S5_SVS_WG 4
#endif
__global__ __launch_bounds__(NT, S5_SVS_WG) void k_svbzd_stream(EncParams p, StreamParams sp) {
    __shared__ uint32_t ws[16];
    __shared__ uint32_t s_g;
    __shared__ uint64_t s_off;
    const int tid = threadIdx.x;
#ifdef S5_SVS_NOTICKET   // tools: what the ticket counter costs (dispatch order is not a guarantee)
    const uint32_t g = blockIdx.x;
#else
    if (tid == 0) s_g = atomicAdd(&sp.ctl[1], 1u);
    __syncthreads();
    const uint32_t g = s_g;
#endif
    const uint32_t r0 = g * S5_SVS_G;
    uint32_t lens[S5_SVS_G];
    uint32_t pos = 0, failed = 0;
    // A group of single-tile reads (<= 4096 samples each: a lane holds a read's tile in registers) learns ALL its lengths before it
    // writes a byte and publishes their sum at once, long before it looks back — so a successor that finishes first finds the size
    // there and does not wait for this workgroup.  Publishing at the end instead makes the launch retire in order: 5.9 ms per 1 M reads,
    // 4.9 this way, 3.5 without the look-back (-DS5_SVS_NOLB).  Looking back early as well (wave 0, under the other waves' writes) or
    // through wider windows (S5_SVS_E) only added traffic on the state words: 6.7 and 5.4 ms.
    bool early = r0 + S5_SVS_G <= p.a.n_reads;
    s5gpu_read_desc_t ds[S5_SVS_G];
#pragma unroll
    for (int k = 0; k < S5_SVS_G; k++) {
        ds[k] = p.a.desc[min(r0 + k, p.a.n_reads - 1)];
        early = early && ds[k].n_samples <= (uint32_t)SVB_TILE;
    }
    if (early) {
        SvbTileLane T[S5_SVS_G];
        uint32_t off[S5_SVS_G], need = 0;
#pragma unroll
        for (int k = 0; k < S5_SVS_G; k++) svb_tile_classify(p.a.sig + ds[k].sig_off, ds[k].n_samples, 0, T[k]);
#pragma unroll
        for (int k = 0; k < S5_SVS_G; k++) {
            uint32_t total;
            off[k] = block_excl_add(T[k].nbytes, ws, total);
            lens[k] = 4 + ((ds[k].n_samples + 3) >> 2) + total;
            need += lens[k];
        }
        if (need <= p.pay_cap) {
            if (tid == 0) __hip_atomic_store(&sp.state[g], (1ull << 62) | need, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
            for (int k = 0; k < S5_SVS_G; k++) {
                uint8_t *blob = smem + pos, *keys = blob + 4;
                const uint32_t n = ds[k].n_samples;
                svb_tile_write(T[k], keys, keys + ((n + 3) >> 2) + off[k]);
                if (tid < 4) blob[tid] = (uint8_t)(n >> (8 * tid));
                pos += lens[k];
            }
        } else {
            early = false;          // does not fit as a whole: read by read below (what fits goes out, the rest is reported)
        }
    }
#pragma unroll
    for (int k = 0; k < S5_SVS_G; k++) {
        if (early) continue;                          // uniform
        lens[k] = 0;
        const uint32_t r = r0 + k;
        if (r >= p.a.n_reads) continue;               // uniform
        const s5gpu_read_desc_t d = p.a.desc[r];
        const int16_t *sig = p.a.sig + d.sig_off;
        const uint32_t n = d.n_samples, nk = (n + 3) >> 2;
        uint32_t total = 0;
        bool ok = (uint64_t)pos + 4 + nk + n <= p.pay_cap;
        if (ok) {
            uint8_t *blob = smem + pos, *keys = blob + 4, *data = keys + nk;
            const uint32_t room = p.pay_cap - pos - 4 - nk;
            for (uint32_t t0 = 0; t0 < n; t0 += SVB_TILE) {
                const uint32_t t = svb_encode_tile(sig, n, t0, keys + (t0 >> 2), data + total, ws, room - total);
                if (t > room - total) { ok = false; break; }   // uniform
                total += t;
            }
            if (ok && tid < 4) blob[tid] = (uint8_t)(n >> (8 * tid));
        }
        if (ok) lens[k] = 4 + nk + total;             // a blob that does not fit: length 0 keeps the chain alive, ctl[0] tells the caller
        else failed++;
        pos += lens[k];
    }
    if (wave_id() == 0) {
#ifdef S5_SVS_NOLB    // tools: what the kernel costs without the look-back (offsets are wrong)
        const uint64_t off = (uint64_t)g * S5_SVS_NOLB;
#else
        const uint64_t off = lookback_offset<S5_SVS_E>(sp.state, g, pos, &sp.ctl[2], early);
#endif
        if (lane_id() == 0) {
            if (failed) atomicAdd(&sp.ctl[0], failed);
            s_off = off;
            uint64_t o = off;
#pragma unroll
            for (int k = 0; k < S5_SVS_G; k++)
                if (r0 + k < p.a.n_reads) { sp.rec_off[r0 + k] = o; p.a.out_len[r0 + k] = lens[k]; o += lens[k]; }
            if (r0 + S5_SVS_G >= p.a.n_reads) sp.rec_off[p.a.n_reads] = o;
        }
    }
    __syncthreads();
    if (pos) copy_record_out(reinterpret_cast<const uint32_t *>(smem), pos, sp.stream + s_off);
}

// ------------------------------------------------------------------------------------------------
// decode
// ------------------------------------------------------------------------------------------------
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
#ifndef S5_IP_WAVES
#define S5_IP_WAVES 6
#endif
// A launch of no more records than the device holds waves (a `get` batch) is as slow as its slowest record: its first pass walks whole segments
// (inflate_par_dev.h, `tail`)
#ifndef S5_IP_LAT_RECS
#define S5_IP_LAT_RECS 6144u
#endif
__device__ __forceinline__ uint32_t ip_tail_for(uint32_t n_recs) { return n_recs <= S5_IP_LAT_RECS ? 0xFFFFu : IP_TAIL; }
// SHORT: the caller's batch holds short records (s5gpu_decode_args.max_pay_cap <= S5_IP_SHORT_PAY): the 256-entry waiting list, 24 waves per CU
#ifndef S5_IP_SHORT_PAY
#define S5_IP_SHORT_PAY 32768u
#endif
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

// read_group rewrite of the merge worker (src/merge.c:51) on decoded payloads: 4 bytes at base + off[i]
// dst[0, bytes) = src[0, bytes), both 16-byte aligned, bytes rounded up to 16 by the caller's buffers.  What it is for: results going back to a
// PINNED HOST buffer (device-visible under the same address) as ordinary stores of a kernel on the batch's own stream — the copy engines the
// hipMemcpyAsync path uses are shared by every stream of the process, and a small download queued behind ANOTHER batch's 32 MB upload
// waits for all of it (round 6, tools/hook_trace.py: 0.72 ms for 520 bytes with two batches in flight, 0.14 alone).
__global__ __launch_bounds__(NT) void k_copy16(uint4 *__restrict__ dst, const uint4 *__restrict__ src, uint64_t n16) {
    for (uint64_t i = (uint64_t)blockIdx.x * NT + threadIdx.x; i < n16; i += (uint64_t)gridDim.x * NT) dst[i] = src[i];
}
__global__ __launch_bounds__(NT) void k_patch_u32(uint8_t *base, const uint64_t *off, const uint32_t *val, uint32_t n) {
    const uint32_t i = blockIdx.x * NT + threadIdx.x;
    if (i >= n) return;
    uint8_t *p = base + off[i];
    const uint32_t v = val[i];
    p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24);
}

// ------------------------------------------------------------------------------------------------
// qts rounding of decoded signals in place (slow5tools degrade: slow5_rec_qts_round, src/degrade.c:255)
// ------------------------------------------------------------------------------------------------
// y = round x to the nearest multiple of 2^b, ties toward +inf, in int32; a y past 32767 steps down by 2^b (it keeps its b trailing
// zeros and stays an int16).  The fixtures pin the non-negative samples only (every sample of tests/golden/ref/raw/degrade lies in
// 271..1464, where round-half-up and round-half-away-from-zero agree).  Negative ties and the top clamp are OUR CHOICE: ties go toward
// +inf on both sides of zero (-6 at b = 2 gives -4), and 32767 at b = 1 gives 32766, not -32768.
__device__ __forceinline__ int32_t qts1(int32_t x, int32_t half, int32_t keep, int32_t step) {
    int32_t y = (x + half) & keep;   // == ((x + half) >> b) << b in two's complement
    if (y > 32767) y -= step;
    return y;
}
__device__ __forceinline__ uint32_t qts2(uint32_t w, int32_t half, int32_t keep, int32_t step) {
    const int32_t lo = qts1((int32_t)(int16_t)(w & 0xFFFFu), half, keep, step), hi = qts1((int32_t)w >> 16, half, keep, step);
    return ((uint32_t)lo & 0xFFFFu) | ((uint32_t)hi << 16);
}
__device__ __forceinline__ uint4 qts8(uint4 v, int32_t half, int32_t keep, int32_t step) {
    v.x = qts2(v.x, half, keep, step); v.y = qts2(v.y, half, keep, step);
    v.z = qts2(v.z, half, keep, step); v.w = qts2(v.w, half, keep, step);
    return v;
}
// Where the records' samples are: sig_off (u64) and n_samples (u32) of record i at off + i * off_stride / len + i * len_stride, so
// the same kernel reads plain arrays (s5gpu_qts_round_dev) and the descriptor tables the pipelines already hold on the device.
struct QtsRecs {
    const uint8_t *off, *len;
    uint32_t off_stride, len_stride, n;
    __device__ __forceinline__ uint64_t o(uint32_t i) const { return *(const uint64_t *)(off + (uint64_t)i * off_stride); }
    __device__ __forceinline__ uint32_t l(uint32_t i) const { return *(const uint32_t *)(len + (uint64_t)i * len_stride); }
};
// The records lie in order (sig_off[i] + n_samples[i] <= sig_off[i + 1], every sig_off a multiple of 8).  The samples between the first
// record's start and the last one's end are cut into as many equal runs of whole 8-sample chunks as the grid has waves, whatever the
// records' lengths: one 2 M-sample read is spread over the whole GPU as evenly as a batch of thousands of 4 k-sample reads.  A wave finds
// the record under its run's start by a 64-way search (each lane probes one point), then walks the records of its run: 16-byte loads and
// stores over the whole chunks, one 2-byte load / store per sample of a record's last partial chunk.  Nothing outside [sig_off,
// sig_off + n_samples) of a record is read or written.
constexpr int QTS_UNROLL = 4;
__global__ __launch_bounds__(NT) void k_qts_round(int16_t *__restrict__ sig, QtsRecs R, uint32_t bits) {
    const uint32_t lane = lane_id();
    const int32_t step = 1 << bits, half = step >> 1, keep = -step;
    const uint64_t nwaves = (uint64_t)gridDim.x * NW, w = (uint64_t)blockIdx.x * NW + wave_id();
    const uint64_t s0 = R.o(0), s1 = R.o(R.n - 1) + R.l(R.n - 1);
    const uint64_t chunks = s1 > s0 ? (s1 - s0 + 7) / 8 : 0;
    const uint64_t A = s0 + 8 * (w * chunks / nwaves), B = s0 + 8 * ((w + 1) * chunks / nwaves);
    if (A >= B) return;
    // the last record that starts at or before A: off[lo] <= A < off[hi] (hi = n: past the end)
    uint32_t lo = 0, hi = R.n;
    while (hi - lo > 1) {
        const uint32_t span = hi - lo;
        const uint32_t p = lo + (uint32_t)((uint64_t)span * lane / 64);            // lane 0 probes lo itself (true)
        const bool le = R.o(p) <= A;
        const uint64_t m = __ballot(le);                                            // monotone in the lane: lanes 0..k set
        const uint32_t k = 63 - __builtin_clzll(m);
        const uint32_t nlo = __shfl(p, k);
        const uint32_t nhi = k == 63 ? hi : __shfl(p, k + 1);
        lo = nlo; hi = nhi;
    }
    for (uint32_t r = lo; r < R.n; r++) {
        const uint64_t o = R.o(r);
        if (o >= B) break;
        const uint64_t e = o + R.l(r);
        const uint64_t a = o > A ? o : A, z = e < B ? e : B;
        if (a >= z) continue;
        uint4 *p = (uint4 *)(sig + a);
        const uint64_t nf = (z - a) / 8;
        uint64_t k = lane;
        for (; k + 64 * (QTS_UNROLL - 1) < nf; k += 64 * QTS_UNROLL) {   // all loads in flight before the first store
            uint4 v[QTS_UNROLL];
#pragma unroll
            for (int u = 0; u < QTS_UNROLL; u++) v[u] = p[k + 64 * u];
#pragma unroll
            for (int u = 0; u < QTS_UNROLL; u++) p[k + 64 * u] = qts8(v[u], half, keep, step);
        }
        for (; k < nf; k += 64) p[k] = qts8(p[k], half, keep, step);
        const uint32_t t = (uint32_t)((z - a) & 7);                     // only at a record's end (A and B are whole chunks)
        if (lane < t) {
            int16_t *q = sig + a + 8 * nf + lane;
            *q = (int16_t)qts1(*q, half, keep, step);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// compaction: slots -> contiguous record stream (the ordered fwrite of src/view.c:296-299)
// ------------------------------------------------------------------------------------------------
constexpr int SCAN_CH = NT * 4;
__device__ __forceinline__ uint64_t block_excl_add64(uint64_t v, uint64_t *ws, uint64_t &total) {
    uint64_t incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        uint64_t t = __shfl_up(incl, d);
        if (lane_id() >= d) incl += t;
    }
    if (lane_id() == 63) ws[wave_id()] = incl;
    __syncthreads();
    uint64_t base = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < NW; w++) {
        uint64_t x = ws[w];
        if (w < wave_id()) base += x;
        tot += x;
    }
    __syncthreads();
    total = tot;
    return base + incl - v;
}
__global__ __launch_bounds__(NT) void k_scan_partial(const uint32_t *len, uint32_t n, uint64_t *partial) {
    __shared__ uint64_t ws[NW];
    const uint32_t b0 = blockIdx.x * SCAN_CH + threadIdx.x * 4;
    uint64_t s = 0;
    for (int q = 0; q < 4; q++) if (b0 + q < n) s += len[b0 + q];
    uint64_t tot;
    block_excl_add64(s, ws, tot);
    if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}
__global__ __launch_bounds__(NT) void k_scan_top(uint64_t *partial, uint32_t nb) {
    __shared__ uint64_t ws[NW];
    uint64_t carry = 0;
    for (uint32_t base = 0; base < nb; base += NT) {
        const uint32_t i = base + threadIdx.x;
        const uint64_t v = i < nb ? partial[i] : 0;
        uint64_t tot;
        const uint64_t ex = block_excl_add64(v, ws, tot);
        if (i < nb) partial[i] = carry + ex;
        carry += tot;
    }
    if (threadIdx.x == 0) partial[nb] = carry;
}
__global__ __launch_bounds__(NT) void k_scan_final(const uint32_t *len, uint32_t n, const uint64_t *partial, uint64_t *off) {
    __shared__ uint64_t ws[NW];
    const uint32_t b0 = blockIdx.x * SCAN_CH + threadIdx.x * 4;
    uint32_t l[4];
    uint64_t s = 0;
    for (int q = 0; q < 4; q++) { l[q] = b0 + q < n ? len[b0 + q] : 0; s += l[q]; }
    uint64_t tot;
    uint64_t ex = partial[blockIdx.x] + block_excl_add64(s, ws, tot);
    for (int q = 0; q < 4; q++) {
        if (b0 + q < n) off[b0 + q] = ex;
        ex += l[q];
    }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) off[n] = partial[gridDim.x];
}
__global__ __launch_bounds__(NT) void k_compact(const s5gpu_read_desc_t *desc, const uint8_t *slots, const uint32_t *len,
                                                const uint64_t *off, uint8_t *stream) {
    const uint32_t r = blockIdx.x;
    const uint8_t *src = slots + desc[r].out_off;
    uint8_t *dst = stream + off[r];
    const uint32_t n = len[r];
    // dst is only byte-aligned (BLOW5 framing has no padding): head bytes up to dst's next 16-byte boundary, then 16-byte stores fed by UNALIGNED
    // 16-byte loads (global memory takes them; round 4: the dword form with its two loads and a funnel shift per store ran at 3.6 TB/s of
    // read + write on mixed lengths), tail bytes
    const uint32_t head = min(n, (uint32_t)((16 - ((uintptr_t)dst & 15)) & 15));
    if (threadIdx.x < head) dst[threadIdx.x] = src[threadIdx.x];
    typedef uint32_t u4u __attribute__((ext_vector_type(4), aligned(1)));
    typedef uint32_t u4a __attribute__((ext_vector_type(4)));
    const uint32_t nv = (n - head) >> 4;
    u4a *d16 = reinterpret_cast<u4a *>(dst + head);
    const uint8_t *s8 = src + head;
    for (uint32_t i = threadIdx.x; i < nv; i += NT) d16[i] = *reinterpret_cast<const u4u *>(s8 + 16u * i);
    const uint32_t tail0 = head + 16 * nv;
    if (threadIdx.x < n - tail0) dst[tail0 + threadIdx.x] = src[tail0 + threadIdx.x];
}

// ------------------------------------------------------------------------------------------------
// synthetic workload (bit-identical to oracle/synth.c)
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ int64_t ih4(uint64_t h) {
    return (int64_t)((h & 0xFFFF) + ((h >> 16) & 0xFFFF) + ((h >> 32) & 0xFFFF) + (h >> 48)) - 131070;
}
__global__ __launch_bounds__(NT) void k_synth(int16_t *sig, uint64_t n_reads, uint64_t n, uint64_t stride, uint64_t seed,
                                              uint64_t first) {
    const uint64_t gid = (uint64_t)blockIdx.x * NT + threadIdx.x;
    if (gid >= n_reads * n) return;
    const uint64_t r = gid / n, i = gid - r * n;
    const uint64_t key = mix64(seed + (first + r) * 0xD1342543DE82EF95ull);
    uint64_t j = i;   // walk back to the event boundary (forced at multiples of 128)
    for (;;) {
        if ((j & 127) == 0) break;
        const uint64_t h = mix64(key ^ (j * 4 + 1));
        if ((((h >> 32) * 10ull) >> 32) == 0) break;
        j--;
    }
    int64_t L = 520 + ((ih4(mix64(key ^ (j * 4 + 2))) * 1663) >> 20);
    L = L < 200 ? 200 : L > 1100 ? 1100 : L;
    const int64_t v = L + ((ih4(mix64(key ^ (i * 4 + 0))) * 277) >> 20);
    sig[r * stride + i] = (int16_t)(v < -32768 ? -32768 : v > 32767 ? 32767 : v);
}
__global__ __launch_bounds__(NT) void k_synth_hdr(uint8_t *hdr, uint64_t n_reads, uint64_t first) {
    const uint64_t r = (uint64_t)blockIdx.x * NT + threadIdx.x;
    if (r >= n_reads) return;
    uint8_t *h = hdr + r * 74;
    const uint64_t idx = first + r;
    const char *hex = "0123456789abcdef";
    h[0] = 36; h[1] = 0;
    uint8_t *id = h + 2;
    for (int k = 0; k < 8; k++) id[k] = hex[(idx >> (4 * (7 - k))) & 15];
    const char *mid = "-0000-4000-8000-";
    for (int k = 0; k < 16; k++) id[8 + k] = mid[k];
    for (int k = 0; k < 12; k++) id[24 + k] = hex[(idx >> (4 * (11 - k))) & 15];
    uint8_t *q = h + 38;
    for (int k = 0; k < 4; k++) q[k] = 0;   // read_group 0
    const double vals[4] = {8192.0, 23.0, 1467.61, 4000.0};
    for (int k = 0; k < 4; k++) {
        const uint64_t bits = (uint64_t)__double_as_longlong(vals[k]);
        for (int b = 0; b < 8; b++) q[4 + 8 * k + b] = (uint8_t)(bits >> (8 * b));
    }
}


// ------------------------------------------------------------------------------------------------
// launchers (C ABI)
// ------------------------------------------------------------------------------------------------
extern "C" uint64_t s5gpu_payload_bound(uint32_t n, uint32_t hdr_len, uint32_t aux_len, int sig_method) {
    const uint64_t sig = sig_method == S5GPU_SIG_SVB_ZD ? 4ull + (n + 3ull) / 4 + 3ull * n
                       : sig_method == S5GPU_SIG_EX_ZD ? 24ull + 2 * ((n + 3ull) / 4 + 4ull * n) + n : 2ull * n;
    return hdr_len + 8ull + sig + aux_len;
}
extern "C" uint64_t s5gpu_slot_bound(uint32_t n, uint32_t hdr_len, uint32_t aux_len, int rec_method, int sig_method) {
    const uint64_t p = s5gpu_payload_bound(n, hdr_len, aux_len, sig_method);
    // stored blocks: 5 bytes + <1 byte of alignment per 16 KiB block; 8 prefix + 2 header + 4 adler; word slack
    // zstd: 8 prefix + 9 frame header + 3 per <= 16 KiB block (raw at worst) + the word flush
    const uint64_t z = rec_method == S5GPU_REC_ZLIB ? p + 6 * (p / DEFL_BLK + 1) + 14 : rec_method == S5GPU_REC_ZSTD ? p + 4 * (p / DEFL_BLK + 1) + 24 : p + 8;
    return (z + 16 + 15) & ~15ull;
}

static uint32_t g_order_min = 8192;            // batches of at least this many records are launched longest first (option "order_min"; 0 = never)
// Scratch of the launch-order list: one buffer per (device, stream) — work on one stream is ordered, so the buffer of a stream is free again
// when the next call on that stream is enqueued — grown on demand, released by s5gpu_shutdown.  One pool and one lock PER DEVICE: the
// multi-device batch calls run one host thread per device, and those must not serialise on each other's list builds.  A buffer that is
// outgrown is retired, not freed (hipFree waits for the device — and an earlier launch on the stream may still read the old list): the
// retired ones are freed once an event recorded on their stream at that moment has completed (round 5; before: at shutdown), and a device keeps
// entries for at most ORD_MAX_STREAMS streams, the least recently used one making room.
struct OrderBuf {
    uint32_t *p = nullptr;
    size_t words = 0;
    hipStream_t st = nullptr;
    uint64_t used = 0;             // the pool's use counter when this stream last asked: the least recently used entry goes first
};
struct RetiredBuf {
    uint32_t *p;
    hipEvent_t ev;                 // recorded on the buffer's stream when it was outgrown: once it has completed nobody reads the buffer any more
};
constexpr int ORD_MAX_DEV = 64;
constexpr size_t ORD_MAX_STREAMS = 32;   // entries kept per device; a process that makes streams by the thousand does not keep a buffer for each
struct OrderPool {
    std::mutex mu;
    std::vector<OrderBuf> live;
    std::vector<RetiredBuf> retired;
    uint64_t tick = 0;
};
static OrderPool g_ord[ORD_MAX_DEV];
void s5kern_release_order() {                 // s5gpu_shutdown
    int cur = 0;
    const bool have_cur = hipGetDevice(&cur) == hipSuccess;
    for (int dev = 0; dev < ORD_MAX_DEV; dev++) {
        OrderPool &P = g_ord[dev];
        std::lock_guard<std::mutex> lk(P.mu);
        if (P.live.empty() && P.retired.empty()) continue;
        (void)hipSetDevice(dev);
        for (OrderBuf &b : P.live) if (b.p) (void)hipFree(b.p);
        for (RetiredBuf &q : P.retired) { (void)hipFree(q.p); if (q.ev) (void)hipEventDestroy(q.ev); }
        P.live.clear();
        P.retired.clear();
    }
    if (have_cur) (void)hipSetDevice(cur);
}
// the (device, stream)'s scratch with room for `need` words, and the pool's lock in `hold`
static int order_scratch(hipStream_t st, size_t need, uint32_t **out, std::unique_lock<std::mutex> &hold) {
    *out = nullptr;
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    if (dev < 0 || dev >= ORD_MAX_DEV) return S5GPU_OK;          // (file order is always correct)
    OrderPool &P = g_ord[dev];
    hold = std::unique_lock<std::mutex>(P.mu);
    // retired buffers whose last reader has finished go back to the device (round 5: they used to wait for s5gpu_shutdown)
    for (size_t i = 0; i < P.retired.size();) {
        if (!P.retired[i].ev || hipEventQuery(P.retired[i].ev) == hipSuccess) {
            if (P.retired[i].ev) { (void)hipFree(P.retired[i].p); (void)hipEventDestroy(P.retired[i].ev); P.retired[i] = P.retired.back(); P.retired.pop_back(); continue; }
        }
        i++;
    }
    OrderBuf *hit = nullptr;
    for (OrderBuf &b : P.live) if (b.st == st) { hit = &b; break; }
    if (!hit) {
        if (P.live.size() >= ORD_MAX_STREAMS) {
            // the stream not seen for the longest time gives up its entry.  Its handle may be gone (the caller destroyed it), so no event can be
            // recorded on it: hipFree waits for the device, which is correct whatever became of the stream — and rare (the 33rd stream)
            size_t lru = 0;
            for (size_t i = 1; i < P.live.size(); i++) if (P.live[i].used < P.live[lru].used) lru = i;
            if (P.live[lru].p) (void)hipFree(P.live[lru].p);
            P.live[lru] = P.live.back();
            P.live.pop_back();
        }
        P.live.emplace_back();
        hit = &P.live.back();
        hit->st = st;
    }
    hit->used = ++P.tick;
    if (hit->words < need) {
        const size_t w = need + need / 2;
        uint32_t *q = nullptr;
        if (hipMalloc((void **)&q, w * sizeof(uint32_t)) != hipSuccess) { hold.unlock(); s5gpu_set_error("no device memory for the launch-order list"); return S5GPU_ERR_NOMEM; }
        if (hit->p) {
            RetiredBuf r{hit->p, nullptr};
            if (hipEventCreateWithFlags(&r.ev, hipEventDisableTiming) != hipSuccess || hipEventRecord(r.ev, st) != hipSuccess) {
                if (r.ev) { (void)hipEventDestroy(r.ev); r.ev = nullptr; }      // no event: the buffer waits for s5gpu_shutdown, as before
            }
            P.retired.push_back(r);
        }
        hit->p = q;
        hit->words = w;
    }
    *out = hit->p;
    return S5GPU_OK;
}
// The one builder behind every length-ordered list (order_dev.h): the (device, stream)'s scratch, then the four kernels with `key` on `st`.
// *out = nullptr when no list is wanted (`list` = false) or none can be had (no scratch: file order is always correct).  `hold` keeps the
// device's pool locked until the caller has enqueued the kernels that read the list: two threads that share a stream (the default stream,
// say) must not interleave "build my list" / "build yours" / "read mine".
// `extra_words` more words of the same scratch (16-byte aligned, behind the list) come back in *extra — the zstd decoders' weights pass; they are
// handed out whether or not a list is built
template <class Key>
static int build_order(const Key &key, uint32_t n, bool list, uint32_t long_bucket, hipStream_t st, const uint32_t **out,
                       std::unique_lock<std::mutex> &hold, size_t extra_words = 0, uint32_t **extra = nullptr) {
    *out = nullptr;
    if (extra) *extra = nullptr;
    if (!list && !(extra && extra_words)) return S5GPU_OK;
    const size_t list_words = list ? (((size_t)ORD_LIST + n + 3) & ~(size_t)3) : 0;
    uint32_t *p = nullptr;
    { const int rc = order_scratch(st, list_words + (extra ? extra_words : 0), &p, hold); if (rc) return rc; }
    if (!p) return S5GPU_OK;
    if (list) {
        const uint32_t nb = (n + NT - 1) / NT;
        hipLaunchKernelGGL(k_order_zero, dim3(1), dim3(NT), 0, st, p);
        hipLaunchKernelGGL(k_order_count<Key>, dim3(nb), dim3(NT), 0, st, key, p);
        hipLaunchKernelGGL(k_order_scan, dim3(1), dim3(128), 0, st, p, long_bucket);
        hipLaunchKernelGGL(k_order_scatter<Key>, dim3(nb), dim3(NT), 0, st, key, p);
        *out = p;
    }
    if (extra && extra_words) *extra = p + list_words;
    return S5GPU_OK;
}
// the decode side's launch order: batches of at least order_min records (want_order = false: no list at all, only the extra words)
static int launch_order(const s5gpu_decode_args_t *a, hipStream_t st, const uint32_t **out, std::unique_lock<std::mutex> &hold,
                        size_t extra_words = 0, uint32_t **extra = nullptr, bool want_order = true) {
    const bool order = want_order && g_order_min && a->n_recs >= g_order_min;
    return build_order(OrderByInLen{a->desc, a->n_recs}, a->n_recs, order, 0, st, out, hold, extra_words, extra);
}
// zstd batches of at least this many frames get the weights pass (k_zstd_weights: the first tree description of every frame, a frame per lane)
// in front of the decoder; smaller ones (a `get` of a few reads) are not worth the extra launch.  Option "zstd_pre_min"; 0 = never.
static uint32_t g_zstd_pre_min = 256;
static size_t zstd_pre_words(const s5gpu_decode_args_t *a) {
    return g_zstd_pre_min && a->n_recs >= g_zstd_pre_min ? (size_t)a->n_recs * (ZW_REC / 4) : 0;
}
// ... the encode side's: the overflow list of a mixed batch (how many reads are on it is only known on the device: the grids cover n_reads)
static int launch_eorder(const s5gpu_encode_args_t *a, hipStream_t st, const uint32_t **out, std::unique_lock<std::mutex> &hold) {
    const bool order = g_order_min && a->n_reads >= g_order_min;
    return build_order(OrderOvfBySamples{a->desc, a->ovf}, a->n_reads, order, 0, st, out, hold);
}
// ... the digest's: decoded records by canonical length (digest_kernels.hip); a batch of one wave's worth of records needs no order
int s5kern_digest_order(const digk::DigRecs &R, hipStream_t st, const uint32_t **out, std::unique_lock<std::mutex> &hold) {
    return build_order(OrderByCanonLen{R.desc, R.fields, R.n}, R.n, R.n > 16, 0, st, out, hold);
}
// ... the event detector's: decoded reads by n_eff (event_kernels.hip); a batch of one wave's worth of reads needs no order
int s5kern_event_order(const sigk::SigRecs &R, hipStream_t st, const uint32_t **out, std::unique_lock<std::mutex> &hold) {
    return build_order(OrderBySigLen{R}, R.n, R.n > 64, 0, st, out, hold);
}

static bool rec_method_ok(int m) { return m == S5GPU_REC_NONE || m == S5GPU_REC_ZLIB || m == S5GPU_REC_ZSTD; }
static bool sig_method_ok(int m) { return m == S5GPU_SIG_NONE || m == S5GPU_SIG_SVB_ZD || m == S5GPU_SIG_EX_ZD; }
static int enc_check(const s5gpu_encode_args_t *a) {
    if (!a || (a->n_reads && (!a->desc || !a->sig || !a->hdr || !a->slots || !a->out_len))) return S5GPU_ERR_ARG;
    return rec_method_ok(a->rec_method) && sig_method_ok(a->sig_method) ? S5GPU_OK : S5GPU_ERR_ARG;
}

// What a launch of an encode kernel carries.  The budget rules are enc_plan.h's; here they become EncParams and bytes of LDS.
static EncParams enc_params(const s5gpu_encode_args_t *a, bool dbg = false) {   // dbg: S5GPU_DEBUG_STAGE is honoured (s5gpu_encode_dev only)
    EncParams p;
    p.a = *a;
    p.dbg = dbg && getenv("S5GPU_DEBUG_STAGE") ? (uint32_t)atoi(getenv("S5GPU_DEBUG_STAGE")) : 0;
    p.zseq = g_zstd_sequences;
    p.obuf_words = 0; p.pay_cap = 0;
    return p;
}
// the staged kernels: one block of payload staged behind the bit buffer (which the build scratch overlays); returns the LDS bytes
static size_t staged_shape(EncParams &p) {
    p.obuf_words = (DEFL_BLK + 64) / 4; p.pay_cap = DEFL_BLK;
    return S_BYTES + 4ull * p.obuf_words + DEFL_BLK;
}
// the fused kernels: `cap` bytes of payload; the bit buffer holds a payload's worth and at least the kernel's build scratch (`floor`)
static size_t fused_shape(EncParams &p, uint32_t cap, uint32_t floor) {
    p.obuf_words = (cap + 64 > floor ? cap + 64 : floor) / 4; p.pay_cap = cap;
    return S_BYTES + 4ull * p.obuf_words + cap;
}
// the single-pass kernels' outputs and look-back state, the state cleared on `st`
static int stream_params(StreamParams *sp, uint32_t n_reads, uint8_t *stream_out, uint64_t *rec_off, uint64_t *state, uint32_t *ctl, hipStream_t st) {
    *sp = StreamParams{reinterpret_cast<unsigned long long *>(state), ctl, stream_out, rec_off};
    HIP_TRY(hipMemsetAsync(state, 0, 8ull * n_reads, st));
    HIP_TRY(hipMemsetAsync(ctl, 0, 16, st));
    return S5GPU_OK;
}

// Every encode kernel variant is named in one place, as the decode ones further down: a launch takes its kernel from these tables, and
// set_lds_attrs walks the same tables, so a variant that can be launched cannot be missing the attribute.
using EncodeKernel = void (*)(EncParams);
using StreamKernel = void (*)(EncParams, StreamParams);
static const EncodeKernel ENCODE_FUSED[] = {k_encode_fused<uint32_t, false>, k_encode_fused<uint32_t, true>, k_encode_fused<uint64_t, false>, k_encode_fused<uint64_t, true>,
                                            k_encode_fused<uint64_t, false, 4>};   // the last: registers for the four workgroups per CU a second launch's LDS allows
static const StreamKernel ENCODE_STREAM[] = {k_encode_stream<uint32_t, false>, k_encode_stream<uint32_t, true>, k_encode_stream<uint64_t, false>, k_encode_stream<uint64_t, true>};
static const EncodeKernel ZSTD_FUSED[] = {k_zstd_fused<false>, k_zstd_fused<true>};
static EncodeKernel encode_fused_kernel(bool wide, bool exzd, bool four_per_cu = false) { return ENCODE_FUSED[four_per_cu ? 4 : 2 * wide + exzd]; }   // (four_per_cu: wide svb-zd only)
static StreamKernel encode_stream_kernel(bool wide, bool exzd) { return ENCODE_STREAM[2 * wide + exzd]; }
static EncodeKernel zstd_fused_kernel(bool exzd) { return ZSTD_FUSED[exzd]; }
// the other kernels that may be launched with more than 64 KiB of dynamic LDS
static const void *const LDS_KERNELS[] = {(const void *)k_deflate_staged, (const void *)k_deflate_lz<LzLong>, (const void *)k_deflate_lz<LzShort>, (const void *)k_zstd_staged,
                                          (const void *)k_svbzd_encode, (const void *)k_svbzd_stream, (const void *)k_inflate_simt<false>, (const void *)k_inflate_simt<true>};

// What is known about a device, per ordinal; found out by the first call that needs it there (the batch API runs host threads on several
// devices at once: atomics, and two threads that find out the same thing at the same time do no harm).  An ordinal past the table has no
// record and is served uncached: asked every time, never taken for another device.
constexpr int DEV_MAX = 64;
struct DeviceFacts {
    std::atomic<bool> attrs{false};        // hipFuncAttributeMaxDynamicSharedMemorySize is set on every kernel of the tables above
    std::atomic<int> cus{0};               // compute units
    std::atomic<uint32_t> np_resident[6];  // workgroups the device holds at once, per no-payload decode variant (np_kernel); 0 = not asked yet
} static g_dev[DEV_MAX];
static DeviceFacts *device_facts() {       // the current device's
    int dev = -1;
    return hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < DEV_MAX ? &g_dev[dev] : nullptr;
}
static int device_cus(int *cus) {          // (<= 0 where the runtime does not say: not kept)
    DeviceFacts *f = device_facts();
    *cus = f ? f->cus.load(std::memory_order_relaxed) : 0;
    if (*cus > 0) return S5GPU_OK;
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    HIP_TRY(hipDeviceGetAttribute(cus, hipDeviceAttributeMultiprocessorCount, dev));
    if (f && *cus > 0) f->cus.store(*cus, std::memory_order_relaxed);
    return S5GPU_OK;
}
static int set_lds_attrs() {
    DeviceFacts *f = device_facts();
    if (f && f->attrs.load(std::memory_order_acquire)) return S5GPU_OK;
    constexpr int LDS_MAX = 160 * 1024 - 256;
    for (EncodeKernel k : ENCODE_FUSED) HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, LDS_MAX));
    for (StreamKernel k : ENCODE_STREAM) HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, LDS_MAX));
    for (EncodeKernel k : ZSTD_FUSED) HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, LDS_MAX));
    for (const void *k : LDS_KERNELS) HIP_TRY(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_MAX));
    if (f) f->attrs.store(true, std::memory_order_release);
    return S5GPU_OK;
}

// The LZ77 kernels over parked payloads (out_len[r] = payload length): payloads of at most 8 KiB on LzShort (4 workgroups per CU), the rest on
// LzLong (1 per CU).  max_payload == 0: unknown (the solo press does not say): both run, each takes its share.
static void launch_lz(EncParams p, uint32_t n, uint32_t max_payload, hipStream_t st, bool build = false) {
    staged_shape(p);
    const bool any_long = max_payload == 0 || max_payload > (uint32_t)LzShort::BLK;
    const uint32_t gs = n < 8192 ? n : 8192;
    hipLaunchKernelGGL(k_deflate_lz<LzShort>, dim3(gs), dim3(NT), S_BYTES + LZS_BYTES, st, p, 0, any_long ? 1 : 0 /* which = 0: every record is short */,
                       build && !any_long ? 1 : 0);
    if (any_long) {
        const uint32_t gl = n < 2048 ? n : 2048;
        hipLaunchKernelGGL(k_deflate_lz<LzLong>, dim3(gl), dim3(LzLong::TN), S_BYTES + 4ull * p.obuf_words + LZ_BYTES, st, p, 0, 1, 0);
    }
}

extern "C" int s5gpu_encode_dev(const s5gpu_encode_args_t *a, void *stream_) {
    int rc = enc_check(a);
    if (rc) { s5gpu_set_error("s5gpu_encode_dev: bad arguments"); return rc; }
    if (a->n_reads == 0) return S5GPU_OK;
    if ((rc = set_lds_attrs())) return rc;
    hipStream_t st = (hipStream_t)stream_;
    EncParams p = enc_params(a, true);
    if (a->rec_method == S5GPU_REC_NONE) {
        hipLaunchKernelGGL(k_pack, dim3(a->n_reads), dim3(NT), 0, st, p, 1, nullptr);
        HIP_TRY(hipGetLastError());
        return S5GPU_OK;
    }
    if (!a->ovf) { s5gpu_set_error("s5gpu_encode_dev: args.ovf (n_reads + 1 words of device scratch) is required"); return S5GPU_ERR_ARG; }
    // LDS budget of the fused kernel (enc_plan.h): 1.55 bytes per sample by default; with ~4 KiB of tables that is ~17 KiB per 4000-sample
    // read -> 8 workgroups per CU.  Anything that does not fit is redone by the staged kernels (correct for any input, slower).
    const uint32_t cap = s5plan::fused_cap(a->sig_method, a->max_payload, a->lds_payload_cap, DEFL_BLK);
    if (a->rec_method == S5GPU_REC_ZLIB && a->sig_method == S5GPU_SIG_NONE) {
        // raw int16 samples: the redundancy is repeated sample pairs at any distance, not runs — the LZ77 matcher (lz_dev.h)
        staged_shape(p);
        // raw-signal records: a batch of short ones (payloads of one 8 KiB block) builds its payloads inside the matcher's kernel
        const bool all_short = a->max_payload != 0 && a->max_payload <= (uint32_t)LzShort::BLK;
        if (!all_short) hipLaunchKernelGGL(k_pack, dim3(a->n_reads), dim3(NT), 0, st, p, 0, nullptr);
        else HIP_TRY(hipMemsetAsync(a->ovf, 0, 4, st));
        launch_lz(p, a->n_reads, a->max_payload, st, all_short);
        if (all_short) {   // reads whose descriptors belie max_payload (the short shape put them on the overflow list): parked + the long shape; usually none
            const uint32_t g = a->n_reads < 1024 ? a->n_reads : 1024;
            hipLaunchKernelGGL(k_pack, dim3(g), dim3(NT), 0, st, p, 2, nullptr);
            hipLaunchKernelGGL(k_deflate_lz<LzLong>, dim3(g), dim3(LzLong::TN), S_BYTES + 4ull * p.obuf_words + LZ_BYTES, st, p, 1, 0, 0);
        }
        HIP_TRY(hipGetLastError());
        return S5GPU_OK;
    }
    if (!s5plan::all_staged(a->sig_method, a->max_payload, a->lds_payload_cap, DEFL_BLK)) {
        HIP_TRY(hipMemsetAsync(a->ovf, 0, 4, st));
        const bool xz = a->sig_method == S5GPU_SIG_EX_ZD, zs = a->rec_method == S5GPU_REC_ZSTD;
        if (zs) {
            const size_t lds = fused_shape(p, cap, BZ_BYTES);
            hipLaunchKernelGGL(zstd_fused_kernel(xz), dim3(a->n_reads), dim3(NT), lds, st, p);
        } else {
            // A caller that names an LDS budget has a batch of mixed lengths.  Option "fused_tier2" (round 4, off by default) gives it TWO fused
            // launches — the named budget at eight workgroups per CU for the short reads, then up to one 16 KiB DEFLATE block for the reads in
            // between, which the staged kernels take through HBM twice; only what fits neither goes on the overflow list.  The first launch leaves
            // out_len[r] = 0 for a read it does not take, the second skips the ones it took.  Measured (profiles/r04_mixed_tier2.txt): the second
            // launch runs at four workgroups per CU (36 KiB of LDS) and takes 3.4 ms for the reads the staged kernels did in 3.6 — nothing gained.
            uint32_t cap2 = a->lds_payload_cap && g_fused_tier2 > cap ? g_fused_tier2 : 0u;
            if (cap2 > a->max_payload) cap2 = (a->max_payload + 15u) & ~15u;
            if (cap2 > (uint32_t)DEFL_BLK) cap2 = DEFL_BLK;
            if (cap2 <= cap) cap2 = 0;
            if (cap2) { HIP_TRY(hipMemsetAsync(a->out_len, 0, 4ull * a->n_reads, st)); p.tier = 1; }
            const size_t lds = fused_shape(p, cap, B_BYTES);
            hipLaunchKernelGGL(encode_fused_kernel(s5plan::wide(cap), xz), dim3(a->n_reads), dim3(NT), lds, st, p);
            if (cap2) {
                p.tier = 2;
                const size_t lds2 = fused_shape(p, cap2, B_BYTES);
                const bool wide2 = s5plan::wide(cap2);   // (wide svb-zd: the variant with registers for the four workgroups per CU its LDS allows)
                hipLaunchKernelGGL(encode_fused_kernel(wide2, xz, wide2 && !xz), dim3(a->n_reads), dim3(NT), lds2, st, p);
                p.tier = 0;
            }
        }
        // overflow reads (usually none: the two launches below then exit at once)
        const size_t st_lds = staged_shape(p);
        const uint32_t g = a->n_reads < 8192 ? a->n_reads : 8192;   // persistent loops over the list; enough workgroups for the CUs to balance
        // the reads on the list, longest first (a caller that names an LDS budget has a mixed batch; otherwise the list is usually empty)
        const uint32_t *eord = nullptr;
        std::unique_lock<std::mutex> hold;
        if (a->lds_payload_cap) { const int rc2 = launch_eorder(a, st, &eord, hold); if (rc2) return rc2; }
        hipLaunchKernelGGL(k_pack, dim3(g), dim3(NT), 0, st, p, 2, eord);
        if (zs) hipLaunchKernelGGL(k_zstd_staged, dim3(g), dim3(NT), st_lds, st, p, 1);
        else hipLaunchKernelGGL(k_deflate_staged, dim3(g), dim3(S5_STAGED_TN), st_lds, st, p, 1, eord);
    } else {
        const size_t st_lds = staged_shape(p);
        hipLaunchKernelGGL(k_pack, dim3(a->n_reads), dim3(NT), 0, st, p, 0, nullptr);
        if (a->rec_method == S5GPU_REC_ZSTD) hipLaunchKernelGGL(k_zstd_staged, dim3(a->n_reads), dim3(NT), st_lds, st, p, 0);
        else hipLaunchKernelGGL(k_deflate_staged, dim3(a->n_reads), dim3(S5_STAGED_TN), st_lds, st, p, 0, nullptr);
    }
    HIP_TRY(hipGetLastError());
    return S5GPU_OK;
}

extern "C" int s5gpu_encode_stream_dev(const s5gpu_encode_args_t *a, uint8_t *stream_out, uint64_t *rec_off, uint64_t *state,
                                       uint32_t *ctl, void *stream_) {
    if (!a || !a->desc || !a->sig || !a->hdr || !a->out_len || !stream_out || !rec_off || !state || !ctl ||
        a->rec_method != S5GPU_REC_ZLIB || !sig_method_ok(a->sig_method)) {
        s5gpu_set_error("s5gpu_encode_stream_dev: bad arguments (zlib record press only)");
        return S5GPU_ERR_ARG;
    }
    if (a->n_reads == 0) return S5GPU_OK;
    int rc;
    if ((rc = set_lds_attrs())) return rc;
    hipStream_t st = (hipStream_t)stream_;
    EncParams p = enc_params(a);
    StreamParams sp;
    if ((rc = stream_params(&sp, a->n_reads, stream_out, rec_off, state, ctl, st))) return rc;
    const uint32_t cap = s5plan::fused_cap(a->sig_method, a->max_payload, a->lds_payload_cap, DEFL_BLK);
    const size_t lds = fused_shape(p, cap, B_BYTES);
    hipLaunchKernelGGL(encode_stream_kernel(s5plan::wide(cap), a->sig_method == S5GPU_SIG_EX_ZD), dim3(a->n_reads), dim3(NT), lds, st, p, sp);
    HIP_TRY(hipGetLastError());
    return S5GPU_OK;
}

// step 1 of the staged path on its own (k_pack, mode 0): every read's payload parked in its slot's tail, out_len = payload length — what
// s5gpu_deflate_parked_dev takes.  A caller that works through a long job chunk by chunk can put the two steps of successive chunks on
// different streams: the streaming step of one chunk and the compaction of another run under the arithmetic of a third.
extern "C" int s5gpu_pack_parked_dev(const s5gpu_encode_args_t *a, void *stream_) {
    int rc = enc_check(a);
    if (rc) { s5gpu_set_error("s5gpu_pack_parked_dev: bad arguments"); return rc; }
    if (a->n_reads == 0) return S5GPU_OK;
    EncParams p = enc_params(a);
    staged_shape(p);
    hipLaunchKernelGGL(k_pack, dim3(a->n_reads), dim3(NT), 0, (hipStream_t)stream_, p, 0, nullptr);
    HIP_TRY(hipGetLastError());
    return S5GPU_OK;
}

extern "C" int s5gpu_deflate_parked_dev(const s5gpu_encode_args_t *a, void *stream_) {
    int rc = enc_check(a);
    if (rc) { s5gpu_set_error("s5gpu_deflate_parked_dev: bad arguments"); return rc; }
    if (a->n_reads == 0) return S5GPU_OK;
    if ((rc = set_lds_attrs())) return rc;
    EncParams p = enc_params(a);
    const size_t lds = staged_shape(p);
    if (a->rec_method == S5GPU_REC_ZSTD) hipLaunchKernelGGL(k_zstd_staged, dim3(a->n_reads), dim3(NT), lds, (hipStream_t)stream_, p, 0);
    else if (a->sig_method == S5GPU_SIG_NONE)   // byte ranges of unknown kind (the solo zlib press): the LZ77 matcher
        launch_lz(p, a->n_reads, a->max_payload, (hipStream_t)stream_);
    else hipLaunchKernelGGL(k_deflate_staged, dim3(a->n_reads), dim3(S5_STAGED_TN), lds, (hipStream_t)stream_, p, 0, nullptr);
    HIP_TRY(hipGetLastError());
    return S5GPU_OK;
}

// Small batches (a single slow5_get) take the wave-per-record decoder (lowest latency); from
// g_inflate_simt_min records on, the lane-per-record decoder (highest throughput).
static uint32_t g_unpack_fused = 1;            // s5gpu_decode_dev, zlib + svb-zd: k_inflate_par unpacks the records it inflates (0: always k_unpack)
static uint32_t g_inflate_par = 1;             // zlib records: the decoder that is parallel inside a record (0: the two older kernels, chosen by batch size)
static uint32_t g_inflate_route = 1;           // big zlib batches: sort by length, long records to the wave kernel (below)
static uint32_t g_np_lds_payload = 1;          // no-payload decode of short svb-zd records: the uncompressed record stays in LDS (option "np_lds_payload")
static uint32_t g_inflate_simt_min = 24576;   // measured crossover on 4000-sample reads: 16384 wave 3.0 ms vs lane 4.2 ms, 32768 wave 5.8 vs lane 4.5
// the options of this file: values lo .. hi are taken, and the bits of `keep` kept
static const struct Option { const char *name; uint32_t *var; long lo, hi; uint32_t keep; } OPTIONS[] = {
    {"inflate_simt_min", &g_inflate_simt_min, 0, LONG_MAX, ~0u},
    {"inflate_route", &g_inflate_route, 0, 1, ~0u},
    {"np_lds_payload", &g_np_lds_payload, 0, 1, ~0u},
    {"fused_tier2", &g_fused_tier2, 0, DEFL_BLK, ~15u},
    {"zstd_sequences", &g_zstd_sequences, 0, 1, ~0u},
    {"unpack_fused", &g_unpack_fused, 0, 1, ~0u},
    {"inflate_par", &g_inflate_par, 0, 2, ~0u},            // 2 (tools): no fallback pass, declined records keep status 8
    {"zstd_pre_min", &g_zstd_pre_min, 0, LONG_MAX, ~0u},   // zstd batches: weights pass from this many frames on (0: never)
    {"order_min", &g_order_min, 0, LONG_MAX, ~0u},         // big zlib batches: longest records first from this many records on (0: never)
};
extern "C" int s5gpu_set_option(const char *key, long value) {
    for (const Option &o : OPTIONS)
        if (key && strcmp(key, o.name) == 0 && value >= o.lo && value <= o.hi) { *o.var = (uint32_t)value & o.keep; return S5GPU_OK; }
    if (s5host_set_option(key, value) == S5GPU_OK || fsk::set_option(key, value) == S5GPU_OK || dfk::set_option(key, value) == S5GPU_OK ||
        dtwk::path_set_option(key, value) == S5GPU_OK || pilek::set_option(key, value) == S5GPU_OK || pilek::hist_set_option(key, value) == S5GPU_OK ||
        pilek::site_set_option(key, value) == S5GPU_OK || refk::long_set_option(key, value) == S5GPU_OK || bandk::set_option(key, value) == S5GPU_OK)
        return S5GPU_OK;
    s5gpu_set_error("s5gpu_set_option: unknown option");
    return S5GPU_ERR_ARG;
}
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
    std::unique_lock<std::mutex> hold;            // (build_order's: released when the kernels that read the list are enqueued)
    if (a->rec_method == S5GPU_REC_ZSTD) {
        const uint32_t *ord = nullptr;
        uint32_t *ws32 = nullptr;
        { const int rc = launch_order(a, st, &ord, hold, zstd_pre_words(a), &ws32); if (rc) return rc; }
        uint8_t *ws = reinterpret_cast<uint8_t *>(ws32);
        if (ws) hipLaunchKernelGGL(k_zstd_weights, dim3((a->n_recs + 63) / 64), dim3(64), 0, st, *a, ws);
        hipLaunchKernelGGL(zstd_inflate_kernel(unpack), dim3(a->n_recs), dim3(64), 0, st, *a, ord, ws);
    } else if (a->rec_method == S5GPU_REC_ZLIB && g_inflate_par) {
        // the waiting list's size follows what was compressed and how long the records are (inflate_par_dev.h): short svb-zd / ex-zd
        // records take the 256-entry list; long ones (several hundred waiting matches per window in their key bytes: 14.7 ms per 8192
        // records of merged_expected_zlib_svb.blow5 with 768 entries, 23.3 with 256), raw-signal records and callers that do not say
        // (max_pay_cap = 0) the 768-entry one
        // (an ex-zd slot is sized for its worst case, 9.5 bytes per sample against svb-zd's 3.25: the same reads, three times the slot)
        const bool shortrec = a->max_pay_cap != 0 && a->max_pay_cap <= S5_IP_SHORT_PAY * (a->sig_method == S5GPU_SIG_EX_ZD ? 3u : 1u);
        const uint32_t *ord = nullptr;
        { const int rc = launch_order(a, st, &ord, hold); if (rc) return rc; }
        hipLaunchKernelGGL(inflate_par_kernel(unpack, shortrec), dim3(a->n_recs), dim3(64), 0, st, *a, ord);
        const uint32_t g = (a->n_recs + 63) / 64 < 4096 ? (a->n_recs + 63) / 64 : 4096;
        if (g_inflate_par == 1) hipLaunchKernelGGL(k_inflate_fallback, dim3(g), dim3(64), 0, st, *a);
    } else if (a->rec_method == S5GPU_REC_ZLIB && a->n_recs >= g_inflate_simt_min) {
        { const int rc = set_lds_attrs(); if (rc) return rc; }
        const uint32_t nb64 = (a->n_recs + 63) / 64;
        const uint32_t *ord = nullptr;
        // routing is the lane kernel's own need (independent of order_min); tiny batches (tests force the lane kernel on them) go without.
        // `hold` stays locked until BOTH readers of the list are enqueued, the lane kernel on st and k_inflate_long on the helper stream; the
        // next build on st is ordered behind the helper stream's join event, so the scratch is free again by then, as for the other lists
        if (a->n_recs >= 1024 && g_inflate_route) {
            const int rc = build_order(OrderByInLen{a->desc, a->n_recs}, a->n_recs, true, ROUTE_LONG_BUCKET, st, &ord, hold);
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
            hipLaunchKernelGGL(k_inflate_long, dim3(a->n_recs < 16384 ? a->n_recs : 16384), dim3(64), 0, t_aux.st, *a, ord);
            HIP_TRY(hipEventRecord(t_aux.join, t_aux.st));
            hipLaunchKernelGGL(k_inflate_simt<true>, dim3(nb64), dim3(64), 64 * sizeof(LaneTables), st, *a, ord);
            HIP_TRY(hipStreamWaitEvent(st, t_aux.join, 0));
        }
    } else {
        hipLaunchKernelGGL(k_inflate, dim3(a->n_recs), dim3(64), 0, st, *a);
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

extern "C" int s5gpu_svbzd_encode_dev(const s5gpu_encode_args_t *a, void *stream_) {
    int rc = enc_check(a);
    if (rc) { s5gpu_set_error("s5gpu_svbzd_encode_dev: bad arguments"); return rc; }
    if (a->n_reads == 0) return S5GPU_OK;
    if ((rc = set_lds_attrs())) return rc;
    EncParams p = enc_params(a);
    p.pay_cap = s5plan::svb_blob_cap(a->max_payload, a->lds_payload_cap, 1);   // LDS for one blob
    hipLaunchKernelGGL(k_svbzd_encode, dim3(a->n_reads), dim3(NT), p.pay_cap, (hipStream_t)stream_, p);
    HIP_TRY(hipGetLastError());
    return S5GPU_OK;
}

extern "C" int s5gpu_svbzd_encode_stream_dev(const s5gpu_encode_args_t *a, uint8_t *stream_out, uint64_t *rec_off, uint64_t *state,
                                             uint32_t *ctl, void *stream_) {
    if (!a || !a->desc || !a->sig || !a->out_len || !stream_out || !rec_off || !state || !ctl) {
        s5gpu_set_error("s5gpu_svbzd_encode_stream_dev: bad arguments");
        return S5GPU_ERR_ARG;
    }
    if (a->n_reads == 0) return S5GPU_OK;
    int rc;
    if ((rc = set_lds_attrs())) return rc;
    hipStream_t st = (hipStream_t)stream_;
    EncParams p = enc_params(a);
    p.pay_cap = s5plan::svb_blob_cap(a->max_payload, a->lds_payload_cap, S5_SVS_G);   // a group's blobs back to back
    StreamParams sp;
    if ((rc = stream_params(&sp, a->n_reads, stream_out, rec_off, state, ctl, st))) return rc;
    hipLaunchKernelGGL(k_svbzd_stream, dim3((a->n_reads + S5_SVS_G - 1) / S5_SVS_G), dim3(NT), p.pay_cap + 16, st, p, sp);   // + the copy's look-ahead word
    HIP_TRY(hipGetLastError());
    return S5GPU_OK;
}

extern "C" uint64_t s5gpu_decode_scratch_bytes(uint32_t max_pay_cap) {
    const uint64_t slot = ((uint64_t)max_pay_cap + 16 + 15) & ~15ull;
    return 64 + slot * (256ull * S5_IP_WAVES * 4 + 256);
}

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

extern "C" int s5gpu_decode_dev(const s5gpu_decode_args_t *a, void *stream_) {
    if (dec_check(a, true, true)) {
        s5gpu_set_error("s5gpu_decode_dev: bad arguments");
        return S5GPU_ERR_ARG;
    }
    if (!rec_method_ok(a->rec_method) || !sig_method_ok(a->sig_method)) { s5gpu_set_error("s5gpu_decode_dev: unsupported method"); return S5GPU_ERR_ARG; }
    if (a->n_recs == 0) return S5GPU_OK;
    hipStream_t st = (hipStream_t)stream_;
    if (a->flags & S5GPU_DEC_NO_PAYLOAD) {
        // fields + signals only: persistent workgroups, one reused scratch slot each (k_inflate_par_np)
        const bool np_xz = a->sig_method == S5GPU_SIG_EX_ZD && a->rec_method == S5GPU_REC_ZLIB;
        if (!np_xz && (a->sig_method != S5GPU_SIG_SVB_ZD || (a->rec_method != S5GPU_REC_ZLIB && a->rec_method != S5GPU_REC_ZSTD))) {
            s5gpu_set_error("s5gpu_decode_dev: S5GPU_DEC_NO_PAYLOAD serves zlib / zstd records with svb-zd signals and zlib records with ex-zd signals");
            return S5GPU_ERR_ARG;
        }
        const uint64_t slot = ((uint64_t)a->max_pay_cap + 16 + 15) & ~15ull;
        if (a->max_pay_cap == 0 || slot > 0xFFFFFFF0ull || a->payload_bytes < 64 + 2 * slot) {
            s5gpu_set_error("s5gpu_decode_dev: S5GPU_DEC_NO_PAYLOAD needs max_pay_cap and at least 64 + 2 * (max_pay_cap + 32) bytes of scratch");
            return S5GPU_ERR_ARG;
        }
        const uint64_t n_slots = (a->payload_bytes - 64) / slot;
        const bool zl = a->rec_method == S5GPU_REC_ZLIB;
        uint64_t n_fb = zl ? (n_slots / 16 < 1 ? 1 : n_slots / 16 > 256 ? 256 : n_slots / 16) : 0;
        uint64_t n_main = n_slots - n_fb;
        // more workgroups than the device holds at once buy nothing: they would only spread the scratch over more of L2.  The count is
        // asked for the template variant that is launched (the two waiting-list sizes differ in LDS: 24 and 21 waves per CU)
        const bool shortrec_np = a->max_pay_cap <= S5_IP_SHORT_PAY * (np_xz ? 3u : 1u);
        // svb-zd records whose payloads all fit the window's storage: inflated into LDS, unpacked from there (k_inflate_par_np<.., LP>)
        // (the caller names the longest compressed record: the kernel takes records of one window — IP_SPAN bytes with the block header — and
        // declines what turns out not to fit)
        const bool lds_pay = zl && !np_xz && g_np_lds_payload && a->max_in_len != 0 && a->max_in_len <= (uint32_t)IP_SPAN - 96u;
        const int variant = !zl ? 4 : lds_pay ? 5 : (np_xz ? 2 : 0) + (shortrec_np ? 1 : 0);
        DeviceFacts *facts = device_facts();
        uint32_t res = facts ? facts->np_resident[variant].load(std::memory_order_relaxed) : 0;
        if (!res) {
            int per_cu = 0, cus = 0;
            { const int rc = device_cus(&cus); if (rc) return rc; }
            HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, np_kernel_addr(variant), 64, 0));
            res = (uint32_t)(per_cu > 0 && cus > 0 ? per_cu * cus : 4096);
            if (facts) facts->np_resident[variant].store(res, std::memory_order_relaxed);
        }
        const uint64_t resident = res;
        if (n_main > resident) n_main = resident;
        if (n_main > a->n_recs) n_main = a->n_recs;
        NpParams np;
        std::unique_lock<std::mutex> hold;
        np.ticket = reinterpret_cast<uint32_t *>(a->payload);
        np.scratch = a->payload + 64;
        np.slot = (uint32_t)slot;
        np.cap = (uint32_t)slot - 16;
        np.first_fb = (uint32_t)n_main;
        np.ord = nullptr;
        if (zl && a->n_recs <= n_main) np.ticket = nullptr;   // one record per workgroup: no ticket counter, nothing to clear (get batches)
        else {
            HIP_TRY(hipMemsetAsync(a->payload, 0, 64, st));
            if (zl) { const int rc = launch_order(a, st, &np.ord, hold); if (rc) return rc; }     // tickets in the order of the list: the longest records first
        }
        if (zl) {
            hipLaunchKernelGGL(np_kernel(variant), dim3((uint32_t)n_main), dim3(64), 0, st, *a, np);
            hipLaunchKernelGGL(k_inflate_fallback_np, dim3((uint32_t)n_fb), dim3(64), 0, st, *a, np);
        } else {
            uint32_t *ws32 = nullptr;
            const uint32_t *none = nullptr;
            { const int rc = launch_order(a, st, &none, hold, zstd_pre_words(a), &ws32, false); if (rc) return rc; }
            uint8_t *ws = reinterpret_cast<uint8_t *>(ws32);
            if (ws) hipLaunchKernelGGL(k_zstd_weights, dim3((a->n_recs + 63) / 64), dim3(64), 0, st, *a, ws);
            hipLaunchKernelGGL(k_zstd_inflate_np, dim3((uint32_t)n_main), dim3(64), 0, st, *a, np, ws);
        }
        HIP_TRY(hipGetLastError());
        return S5GPU_OK;
    }
    // svb-zd records under zlib (default inflate kernel) or zstd: the wave that decompresses a record unpacks it too
    // ... and ex-zd records (round 3)
    const int fused = !g_unpack_fused ? 0
                    : a->sig_method == S5GPU_SIG_SVB_ZD && ((a->rec_method == S5GPU_REC_ZLIB && g_inflate_par == 1) || a->rec_method == S5GPU_REC_ZSTD) ? 1
                    : a->sig_method == S5GPU_SIG_EX_ZD && ((a->rec_method == S5GPU_REC_ZLIB && g_inflate_par == 1) || a->rec_method == S5GPU_REC_ZSTD) ? 2 : 0;
    int rc = launch_inflate(a, st, fused);
    if (rc) return rc;
    // the workgroup form of the ex-zd decoder keeps one chunk of exceptions and a flag map in (dynamic) LDS; the other signal formats need none
    const size_t xlds = a->sig_method == S5GPU_SIG_EX_ZD ? sizeof(ExzdScratch) : 0;
    if (fused) hipLaunchKernelGGL(k_unpack_rest, dim3((a->n_recs + NT - 1) / NT < 2048 ? (a->n_recs + NT - 1) / NT : 2048), dim3(NT), xlds, st, *a);
    else hipLaunchKernelGGL(k_unpack, dim3(a->n_recs), dim3(NT), xlds, st, *a);
    HIP_TRY(hipGetLastError());
    return S5GPU_OK;
}

// the scan of s5gpu_compact_dev, also on its own: off[i] = len[0] + ... + len[i-1], off[n] = total (the line offsets of skim_api.hip)
int s5_scan_lengths(const uint32_t *len, uint32_t n, uint64_t *off, uint64_t *tmp, hipStream_t st) {
    if (n == 0) return S5GPU_OK;
    const uint32_t nb = (n + SCAN_CH - 1) / SCAN_CH;
    hipLaunchKernelGGL(k_scan_partial, dim3(nb), dim3(NT), 0, st, len, n, tmp);
    hipLaunchKernelGGL(k_scan_top, dim3(1), dim3(NT), 0, st, tmp, nb);
    hipLaunchKernelGGL(k_scan_final, dim3(nb), dim3(NT), 0, st, len, n, tmp, off);
    HIP_TRY(hipGetLastError());
    return S5GPU_OK;
}

extern "C" int s5gpu_compact_dev(uint32_t n, const s5gpu_read_desc_t *desc, const uint8_t *slots, const uint32_t *out_len,
                                 uint64_t *rec_off, uint8_t *stream, uint64_t *tmp, void *stream_) {
    if (n == 0) return S5GPU_OK;
    if (!desc || !slots || !out_len || !rec_off || !stream || !tmp) return S5GPU_ERR_ARG;
    hipStream_t st = (hipStream_t)stream_;
    { const int rc = s5_scan_lengths(out_len, n, rec_off, tmp, st); if (rc) return rc; }
    hipLaunchKernelGGL(k_compact, dim3(n), dim3(NT), 0, st, desc, slots, out_len, rec_off, stream);
    HIP_TRY(hipGetLastError());
    return S5GPU_OK;
}

// slot r (desc[r].out_off in `slots`, len[r] bytes) -> dst + off[r]: k_compact with the destinations given (the text assembly of ascii_api.hip)
extern "C" int s5gpu_scatter_slots_dev(uint32_t n, const s5gpu_read_desc_t *desc, const uint8_t *slots, const uint32_t *len, const uint64_t *off, uint8_t *dst,
                                       void *stream_) {
    if (n == 0) return S5GPU_OK;
    if (!desc || !slots || !len || !off || !dst) return S5GPU_ERR_ARG;
    hipLaunchKernelGGL(k_compact, dim3(n), dim3(NT), 0, (hipStream_t)stream_, desc, slots, len, off, dst);
    HIP_TRY(hipGetLastError());
    return S5GPU_OK;
}

// device (or device-visible pinned host) to device / pinned host, by a kernel on `stream_`: dst and src 16-byte aligned, room for bytes rounded up to 16
extern "C" int s5gpu_copy_dev(void *dst, const void *src, uint64_t bytes, void *stream_) {
    if (bytes == 0) return S5GPU_OK;
    if (!dst || !src || (((uintptr_t)dst | (uintptr_t)src) & 15)) return S5GPU_ERR_ARG;
    const uint64_t n16 = (bytes + 15) / 16;
    const uint64_t want = (n16 + NT - 1) / NT;
    hipLaunchKernelGGL(k_copy16, dim3((uint32_t)(want < 2048 ? want : 2048)), dim3(NT), 0, (hipStream_t)stream_, (uint4 *)dst, (const uint4 *)src, n16);
    HIP_TRY(hipGetLastError());
    return S5GPU_OK;
}

extern "C" int s5gpu_patch_u32_dev(uint8_t *base, const uint64_t *off, const uint32_t *val, uint32_t n, void *stream_) {
    if (n == 0) return S5GPU_OK;
    if (!base || !off || !val) return S5GPU_ERR_ARG;
    hipLaunchKernelGGL(k_patch_u32, dim3((n + NT - 1) / NT), dim3(NT), 0, (hipStream_t)stream_, base, off, val, n);
    HIP_TRY(hipGetLastError());
    return S5GPU_OK;
}

// k_qts_round: four workgroups of four waves per CU of the current device (the runs are equal, so a wave that is done leaves nothing behind)
int s5_qts_round_strided(int16_t *sig, uint32_t n, const void *sig_off, uint32_t off_stride, const void *n_samples, uint32_t len_stride,
                         uint32_t bits, hipStream_t st) {
    if (bits < 1 || bits > 16) { s5gpu_set_error("qts rounding: bits %u outside 1..16", bits); return S5GPU_ERR_ARG; }
    if (n == 0) return S5GPU_OK;
    if (!sig || !sig_off || !n_samples) { s5gpu_set_error("qts rounding: NULL argument"); return S5GPU_ERR_ARG; }
    int cu = 0;
    { const int rc = device_cus(&cu); if (rc) return rc; }
    if (cu <= 0) cu = 256;
    QtsRecs R = {(const uint8_t *)sig_off, (const uint8_t *)n_samples, off_stride, len_stride, n};
    hipLaunchKernelGGL(k_qts_round, dim3(4 * cu), dim3(NT), 0, st, sig, R, bits);
    HIP_TRY(hipGetLastError());
    return S5GPU_OK;
}
extern "C" int s5gpu_qts_round_dev(int16_t *sig, uint32_t n, const uint64_t *sig_off, const uint32_t *n_samples, uint32_t bits, void *stream_) {
    return s5_qts_round_strided(sig, n, sig_off, sizeof(uint64_t), n_samples, sizeof(uint32_t), bits, (hipStream_t)stream_);
}

// ---- s5gpu_warmup: the code objects of this file and of ascii_kernels.hip are loaded by their first launch ----
__global__ void k_noop(uint32_t *p) { if (p) p[0] = 0; }
int s5ascii_warm(hipStream_t st);              // ascii_kernels.hip
int s5host_warm_contexts();   // host_api.hip
#include <time.h>
static void s5_trace(const char *what) {   // S5GPU_TRACE=1 (tools): milliseconds since this thread's previous trace point (as host_ctx.h's)
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
extern "C" int s5gpu_warmup(void) {
    int rc;
    s5_trace("warmup: start");
    if (s5gpu_devices_in_use() == 0 && (rc = s5gpu_init(0))) return rc;
    s5_trace("warmup: runtime + device up");
    if ((rc = set_lds_attrs())) return rc;     // (the function attributes need the functions: this loads the code object)
    s5_trace("warmup: function attributes set (code object loaded)");
    hipLaunchKernelGGL(k_noop, dim3(1), dim3(64), 0, nullptr, (uint32_t *)nullptr);
    HIP_TRY(hipGetLastError());
    if ((rc = s5ascii_warm(nullptr))) return rc;
    s5_trace("warmup: first launches enqueued");
    if ((rc = s5host_warm_contexts())) return rc;   // the batch calls' streams (round 5: 2 x 21 ms that the first batch call of a `get` used to pay)
    s5_trace("warmup: contexts (streams) created");
    HIP_TRY(hipStreamSynchronize(nullptr));
    s5_trace("warmup: done");
    return S5GPU_OK;
}

extern "C" int s5gpu_synth_dev(int16_t *sig, uint64_t n_reads, uint64_t n, uint64_t stride, uint64_t seed, uint64_t first,
                               void *stream_) {
    if (!sig || stride < n) return S5GPU_ERR_ARG;
    const uint64_t tot = n_reads * n;
    if (tot == 0) return S5GPU_OK;
    const uint64_t nb = (tot + NT - 1) / NT;
    if (nb > 0x7FFFFFFFull) return S5GPU_ERR_ARG;
    hipLaunchKernelGGL(k_synth, dim3((uint32_t)nb), dim3(NT), 0, (hipStream_t)stream_, sig, n_reads, n, stride, seed, first);
    HIP_TRY(hipGetLastError());
    return S5GPU_OK;
}
extern "C" int s5gpu_synth_hdr_dev(uint8_t *hdr, uint64_t n_reads, uint64_t first, void *stream_) {
    if (!hdr) return S5GPU_ERR_ARG;
    if (n_reads == 0) return S5GPU_OK;
    hipLaunchKernelGGL(k_synth_hdr, dim3((uint32_t)((n_reads + NT - 1) / NT)), dim3(NT), 0, (hipStream_t)stream_, hdr, n_reads, first);
    HIP_TRY(hipGetLastError());
    return S5GPU_OK;
}

// variant builds of tools/ only: the phase clocks of a decoder or the matcher, read and cleared
template <size_t N>
static int probe_read(unsigned long long (&clocks)[N], unsigned long long *out) {
    unsigned long long z[N] = {0};
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(clocks), sizeof z) != hipSuccess) return S5GPU_ERR_HIP;
    if (hipMemcpyToSymbol(HIP_SYMBOL(clocks), z, sizeof z) != hipSuccess) return S5GPU_ERR_HIP;
    return S5GPU_OK;
}
#ifdef S5_LZPROBE   // tools/lz_phases.py (lz_dev.h)
extern "C" int s5gpu_lzprobe_read(unsigned long long *out16) { return probe_read(s5::g_lzprobe, out16); }
#endif
#ifdef S5_IPROBE   // tools/inflate_phases.py (inflate_par_dev.h)
extern "C" int s5gpu_iprobe_read(unsigned long long *out20) { return probe_read(s5::g_iprobe, out20); }
#endif
#ifdef S5_ZPROBE   // tools/zstd_phases.py (zstd_dev.h)
extern "C" int s5gpu_zprobe_read(unsigned long long *out16) { return probe_read(s5::g_zprobe, out16); }
#endif
