// batch_kernels.hip — what a batch needs around its encode or decode: copies and patches on the batch's own stream, qts rounding, the scan and
// compaction of slots into a record stream, the synthetic workload; and what the library keeps per process: the per-device facts,
// s5gpu_set_option (every unit's options, chained) and s5gpu_warmup (every code object of the press path loaded before the first batch).
#include "launch_common.h"
#include "dev_common.h"
#include "enc_plan.h"

using namespace s5;

// dst[0, bytes) = src[0, bytes), both 16-byte aligned, bytes rounded up to 16 by the caller's buffers.  What it is for: results going back to a
// PINNED HOST buffer (device-visible under the same address) as ordinary stores of a kernel on the batch's own stream — the copy engines the
// hipMemcpyAsync path uses are shared by every stream of the process, and a small download queued behind ANOTHER batch's 32 MB upload
// waits for all of it (round 6, tools/hook_trace.py: 0.72 ms for 520 bytes with two batches in flight, 0.14 alone).
__global__ __launch_bounds__(NT) void k_copy16(uint4 *__restrict__ dst, const uint4 *__restrict__ src, uint64_t n16) {
    for (uint64_t i = (uint64_t)blockIdx.x * NT + threadIdx.x; i < n16; i += (uint64_t)gridDim.x * NT) dst[i] = src[i];
}
// read_group rewrite of the merge worker (src/merge.c:51) on decoded payloads: 4 bytes at base + off[i]
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
    const uint64_t z = rec_method == S5GPU_REC_ZLIB ? p + 6 * (p / s5plan::BLK + 1) + 14 : rec_method == S5GPU_REC_ZSTD ? p + 4 * (p / s5plan::BLK + 1) + 24 : p + 8;
    return (z + 16 + 15) & ~15ull;
}

static DeviceFacts g_dev[DEV_MAX];         // (launch_common.h)
DeviceFacts *device_facts() {
    int dev = -1;
    return hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < DEV_MAX ? &g_dev[dev] : nullptr;
}
int device_cus(int *cus) {
    DeviceFacts *f = device_facts();
    *cus = f ? f->cus.load(std::memory_order_relaxed) : 0;
    if (*cus > 0) return S5GPU_OK;
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    HIP_TRY(hipDeviceGetAttribute(cus, hipDeviceAttributeMultiprocessorCount, dev));
    if (f && *cus > 0) f->cus.store(*cus, std::memory_order_relaxed);
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

int s5host_set_option(const char *key, long value);   // host_api.hip: options of the host layer
namespace fsk { int set_option(const char *key, long value); }   // fstats_kernels.hip: the file statistics' window, bins and flush point
namespace dfk { int set_option(const char *key, long value); }   // diff_kernels.hip: the difference histogram's window, flush point and grid
namespace dtwk { int path_set_option(const char *key, long value); }   // dtw_path_api.hip: which passes the path call launches
namespace pilek { int set_option(const char *key, long value); }   // pileup_kernels.hip: the pileup's LDS windows, grids, segments, sort and passes
namespace pilek { int hist_set_option(const char *key, long value); }   // contrast_kernels.hip: the level histograms' window and grid
namespace pilek { int site_set_option(const char *key, long value); }   // sites_kernels.hip: which passes the site call launches
namespace refk { int long_set_option(const char *key, long value); }   // refine_long_kernels.hip: which passes the whole-read refine launches
namespace pilek { int fold_set_option(const char *key, long value); }   // fold_kernels.hip: the fold's class table in LDS, and its grid
namespace bandk { int set_option(const char *key, long value); }   // band_kernels.hip: which passes the band call launches
// every unit owns its options; a key nobody takes, or a value outside its key's range, is unknown
extern "C" int s5gpu_set_option(const char *key, long value) {
    if (deck::set_option(key, value) == S5GPU_OK || enck::set_option(key, value) == S5GPU_OK || ordk::set_option(key, value) == S5GPU_OK ||
        s5host_set_option(key, value) == S5GPU_OK || fsk::set_option(key, value) == S5GPU_OK || dfk::set_option(key, value) == S5GPU_OK ||
        dtwk::path_set_option(key, value) == S5GPU_OK || pilek::set_option(key, value) == S5GPU_OK || pilek::hist_set_option(key, value) == S5GPU_OK ||
        pilek::site_set_option(key, value) == S5GPU_OK || refk::long_set_option(key, value) == S5GPU_OK || bandk::set_option(key, value) == S5GPU_OK ||
        pilek::fold_set_option(key, value) == S5GPU_OK)
        return S5GPU_OK;
    s5gpu_set_error("s5gpu_set_option: unknown option");
    return S5GPU_ERR_ARG;
}

// ---- s5gpu_warmup: a code object is loaded by the first use of one of its functions; the four of the press path and ascii_kernels.hip's here ----
__global__ void k_noop(uint32_t *p) { if (p) p[0] = 0; }
int s5ascii_warm(hipStream_t st);              // ascii_kernels.hip
int s5host_warm_contexts();   // host_api.hip
extern "C" int s5gpu_warmup(void) {
    int rc;
    s5_trace("warmup: start");
    if (s5gpu_devices_in_use() == 0 && (rc = s5gpu_init(0))) return rc;
    s5_trace("warmup: runtime + device up");
    if ((rc = enck::warm()) || (rc = deck::warm()) || (rc = ordk::warm())) return rc;
    s5_trace("warmup: function attributes set (code object loaded)");
    hipLaunchKernelGGL(k_noop, dim3(1), dim3(64), 0, nullptr, (uint32_t *)nullptr);   // (this file's)
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
