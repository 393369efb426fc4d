// encode_kernels.hip — gfx950 (CDNA4) kernels of the encode half of the BLOW5 record press path + their launchers.
// One read per workgroup (4 x wave64); all intermediates of a read live in LDS; HBM sees the int16
// samples once (coalesced 16-B loads) and the finished record once (coalesced word stores).
#include <limits.h>

#include "launch_common.h"
#include "resident_rules.h"
#include "deflate_dev.h"
#include "lz_dev.h"
#include "zstd_enc_dev.h"
#include "svb_dev.h"
#include "exzd_dev.h"
#define S5_ORDER_LIST_ONLY   // (the overflow list is read here; order_launch.hip builds it)
#include "order_dev.h"
#include "enc_plan.h"

using namespace s5;

static_assert(s5plan::BLK == (uint32_t)DEFL_BLK && s5plan::SIG_SVB_ZD == S5GPU_SIG_SVB_ZD && s5plan::SIG_EX_ZD == S5GPU_SIG_EX_ZD, "enc_plan.h restates these");

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
// launchers (C ABI)
// ------------------------------------------------------------------------------------------------
static int enc_check(const s5gpu_encode_args_t *a) {
    if (!a || (a->n_reads && (!a->desc || !a->sig || !a->hdr || !a->slots || !a->out_len))) return S5GPU_ERR_ARG;
    return s5rules::methods_ok(a->rec_method, a->sig_method) ? S5GPU_OK : S5GPU_ERR_ARG;
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

// Every encode kernel variant is named in one place, as the decode ones in decode_kernels.hip: a launch takes its kernel from these tables, and
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
                                          (const void *)k_svbzd_encode, (const void *)k_svbzd_stream};

static int set_lds_attrs() {               // once per device (launch_common.h: DeviceFacts)
    DeviceFacts *f = device_facts();
    if (f && f->enc_attrs.load(std::memory_order_acquire)) return S5GPU_OK;
    for (EncodeKernel k : ENCODE_FUSED) HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, LDS_MAX));
    for (StreamKernel k : ENCODE_STREAM) HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, LDS_MAX));
    for (EncodeKernel k : ZSTD_FUSED) HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, LDS_MAX));
    for (const void *k : LDS_KERNELS) HIP_TRY(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_MAX));
    if (f) f->enc_attrs.store(true, std::memory_order_release);
    return S5GPU_OK;
}
int enck::warm() { return set_lds_attrs(); }   // (the function attributes need the functions: this loads the code object)

static const S5Option OPTIONS[] = {
    {"fused_tier2", &g_fused_tier2, 0, DEFL_BLK, ~15u},
    {"zstd_sequences", &g_zstd_sequences, 0, 1, ~0u},
};
int enck::set_option(const char *key, long value) { return s5_set_option(OPTIONS, key, value); }

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
        if (a->lds_payload_cap) { const int rc2 = s5kern_encode_order(a, st, &eord, hold); if (rc2) return rc2; }
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
        a->rec_method != S5GPU_REC_ZLIB || !s5rules::sig_method_ok(a->sig_method)) {
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

#ifdef S5_LZPROBE   // tools/lz_phases.py (a variant build; lz_dev.h): the phase clocks of the matcher, read and cleared
extern "C" int s5gpu_lzprobe_read(unsigned long long *out16) {
    unsigned long long z[16] = {0};
    if (hipMemcpyFromSymbol(out16, HIP_SYMBOL(s5::g_lzprobe), sizeof z) != hipSuccess) return S5GPU_ERR_HIP;
    return hipMemcpyToSymbol(HIP_SYMBOL(s5::g_lzprobe), z, sizeof z) != hipSuccess ? S5GPU_ERR_HIP : S5GPU_OK;
}
#endif
