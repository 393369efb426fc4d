// fstats_kernels.hip — what is in a whole file's signal (docs/codecs.md §4.13): one s5gpu_file_stats_t per file stays on the device and
// k_file_stats adds every batch the decoder leaves behind to it.  Every member is an integer sum, min, max, OR or AND, so the result does not
// depend on the launch shape or on the order of the adds.  The construction rules are those of signal_kernels.hip:
//   1. the sample count of a record is SigRecs::n_eff (0 for a failed record, never past the record's slot), nothing else;
//   2. every index is a masked bit field: LDS bins of (value - window) & (bins - 1) behind the range test, acc->hist of (x + 32768) & 0xFFFF,
//      read groups of rg & 255 behind rg < 256, length classes of a count of leading zeros;
//   3. every loop's trip count is fixed by n_eff, the record count or the bin count; the flush points depend on n_eff alone;
//   4. nothing waits on data: the only synchronisation is the workgroup barrier around a flush, reached by all threads or by none.
#include <stddef.h>
#include <string.h>

#include "dev_common.h"
#include "fstats_dev.h"

extern "C" void s5gpu_set_error(const char *fmt, ...);

using namespace s5;

static_assert(sizeof(s5gpu_file_stats_t) == 528720 && offsetof(s5gpu_file_stats_t, min) == 40 && offsetof(s5gpu_file_stats_t, or_bits) == 48 &&
                  offsetof(s5gpu_file_stats_t, len_min) == 56 && offsetof(s5gpu_file_stats_t, len_hist) == 64 &&
                  offsetof(s5gpu_file_stats_t, hist) == 4432,
              "include/slow5gpu.h fixes this layout; k_file_stats_reset writes words 5 - 7 by number");

namespace {

fsk::Opts g_opts = {-1, fsk::MAX_BINS, 0xFFFFFFFFu};
uint32_t g_grid = fsk::MAX_GRID;   // option "fstats_grid"

__device__ __forceinline__ void add64(uint64_t *p, uint64_t v) { atomicAdd(reinterpret_cast<unsigned long long *>(p), (unsigned long long)v); }

// f(x) for every sample of p[0, n): 16-byte loads over the whole groups of 8 (p is 16-byte aligned when vec), 2-byte loads over the rest
template <class F>
__device__ __forceinline__ void for_each_sample(const int16_t *p, uint32_t n, bool vec, F f) {
    const uint32_t nv = vec ? n >> 3 : 0u;
    const uint4 *v = reinterpret_cast<const uint4 *>(p);
    for (uint32_t k = threadIdx.x; k < nv; k += NT) {
        const uint4 u = v[k];
        f((int)(int16_t)(u.x & 0xFFFFu)); f((int)(int16_t)(u.x >> 16));
        f((int)(int16_t)(u.y & 0xFFFFu)); f((int)(int16_t)(u.y >> 16));
        f((int)(int16_t)(u.z & 0xFFFFu)); f((int)(int16_t)(u.z >> 16));
        f((int)(int16_t)(u.w & 0xFFFFu)); f((int)(int16_t)(u.w >> 16));
    }
    for (uint32_t i = (nv << 3) + threadIdx.x; i < n; i += NT) f((int)p[i]);
}

template <class T, class Op>
__device__ __forceinline__ T wave_all(T v, Op op) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = op(v, __shfl_xor(v, d));
    return v;
}

}  // namespace

// The empty accumulator: zeros but for the identities of min / max, AND and len_min (words 5, 6 and 7 of the struct).
__global__ __launch_bounds__(NT) void k_file_stats_reset(uint64_t *__restrict__ w) {
    constexpr uint32_t WORDS = sizeof(s5gpu_file_stats_t) / 8;
    for (uint32_t k = blockIdx.x * NT + threadIdx.x; k < WORDS; k += gridDim.x * NT) {
        uint64_t v = 0;
        if (k == 5) v = (uint64_t)32767u | ((uint64_t)(uint32_t)-32768 << 32);      // min | max
        if (k == 6) v = (uint64_t)0xFFFFu << 32;                                     // or_bits | and_bits
        if (k == 7) v = 0xFFFFFFFFull;                                               // len_min | len_max
        w[k] = v;
    }
}

__global__ void k_file_stats_add_failed(s5gpu_file_stats_t *acc, uint32_t k) {
    if (blockIdx.x == 0 && threadIdx.x == 0) add64(&acc->n_failed, k);
}

// A workgroup walks the records blockIdx.x, blockIdx.x + gridDim.x, ...; all its threads share a record's samples.  Moments, extremes and
// bit masks stay in registers until the end; read counts, length classes and read groups go through small LDS tables (thread 0); samples
// inside the window [lo, lo + bins) are counted in LDS, COPIES counters per bin so that the lanes of a wave that meet on one value (raw
// signal puts most of a wave on a few dozen values) spread over adjacent banks; samples outside it are global atomics.
__global__ __launch_bounds__(NT) void k_file_stats(sigk::SigRecs R, fsk::Opts O, s5gpu_file_stats_t *__restrict__ acc) {
    extern __shared__ __attribute__((aligned(16))) uint32_t fs_win[];     // O.bins * COPIES counters
    __shared__ uint32_t s_len[64], s_rgr[256], s_lo;
    __shared__ unsigned long long s_rgs[256];
    const uint32_t bins = O.bins, bmask = bins - 1u;
    for (uint32_t t = threadIdx.x; t < bins * fsk::COPIES; t += NT) fs_win[t] = 0;
    if (threadIdx.x < 64u) s_len[threadIdx.x] = 0;
    s_rgr[threadIdx.x & 255u] = 0;
    s_rgs[threadIdx.x & 255u] = 0;
    if (wave_id() == 0) {
        uint32_t lo = O.win_lo < 0 ? 0u : (uint32_t)O.win_lo;
        if (O.win_lo < 0) {                                               // the mean of the first samples of this workgroup's first record
            int32_t st;
            const uint32_t n0 = R.n_eff(blockIdx.x, &st), m = n0 < 64u ? n0 : 64u;
            int v = (uint32_t)lane_id() < m ? (int)R.sig[R.o(blockIdx.x) + (uint32_t)lane_id()] : 0;
            v = wave_all(v, [](int a, int b) { return a + b; });
            const int centre = 32768 + (m ? v / (int)m : 512);
            lo = centre > (int)(bins >> 1) ? (uint32_t)centre - (bins >> 1) : 0u;
        }
        if (lo > 65536u - bins) lo = 65536u - bins;
        if (lane_id() == 0) s_lo = lo;
    }
    __syncthreads();
    const uint32_t lo = s_lo, copy = threadIdx.x & (fsk::COPIES - 1u);

    auto flush = [&]() {                                                  // (called by every thread of the workgroup or by none)
        __syncthreads();
        for (uint32_t b = threadIdx.x; b < bins; b += NT) {
            uint4 *c = reinterpret_cast<uint4 *>(fs_win + b * fsk::COPIES);
            const uint4 u = *c;
            const uint64_t t = (uint64_t)u.x + u.y + u.z + u.w;
            if (t) {
                add64(&acc->hist[(lo + b) & 0xFFFFu], t);
                *c = make_uint4(0, 0, 0, 0);
            }
        }
        __syncthreads();
    };

    long long s = 0;
    unsigned long long ss = 0;
    int mn = 32767, mx = -32768;
    uint32_t orb = 0, andb = 0xFFFFu, len_min = 0xFFFFFFFFu, len_max = 0;
    uint64_t reads = 0, failed = 0, samples = 0, other = 0, since = 0;    // the same in every thread: they depend on n_eff and the fields alone
    for (uint32_t i = blockIdx.x; i < R.n; i += gridDim.x) {
        int32_t st;
        const uint32_t n = R.n_eff(i, &st);
        if (st != 0) { failed++; continue; }
        const uint32_t rg = R.fields[i].read_group;
        reads++;
        samples += n;
        len_min = n < len_min ? n : len_min;
        len_max = n > len_max ? n : len_max;
        if (rg >= 256u) other++;
        if (threadIdx.x == 0) {
            atomicAdd(&s_len[(n ? 32u - (uint32_t)__builtin_clz(n) : 0u) & 63u], 1u);
            if (rg < 256u) { atomicAdd(&s_rgr[rg & 255u], 1u); atomicAdd(&s_rgs[rg & 255u], (unsigned long long)n); }
        }
        if (n == 0) continue;
        if (bins && since + n > (uint64_t)O.flush) { flush(); since = 0; }  // n < 2^32: the counters of one read cannot wrap
        since += n;
        const uint64_t o = R.o(i);
        for_each_sample(R.sig + o, n, (o & 7u) == 0, [&](int x) {
            mn = min(mn, x); mx = max(mx, x);
            s += x; ss += (uint32_t)(x * x);
            const uint32_t u = (uint32_t)x & 0xFFFFu, b = (uint32_t)(x + 32768) & 0xFFFFu, d = b - lo;
            orb |= u; andb &= u;
            if (d < bins) atomicAdd(&fs_win[(d & bmask) * fsk::COPIES + copy], 1u);
            else add64(&acc->hist[b], 1);
        });
    }
    flush();
    if (threadIdx.x < 33u && s_len[threadIdx.x]) add64(&acc->len_hist[threadIdx.x], s_len[threadIdx.x]);
    if (s_rgr[threadIdx.x & 255u]) {
        add64(&acc->rg_reads[threadIdx.x & 255u], s_rgr[threadIdx.x & 255u]);
        add64(&acc->rg_samples[threadIdx.x & 255u], s_rgs[threadIdx.x & 255u]);
    }
    s = wave_all(s, [](long long a, long long b) { return a + b; });
    ss = wave_all(ss, [](unsigned long long a, unsigned long long b) { return a + b; });
    mn = wave_all(mn, [](int a, int b) { return a < b ? a : b; });
    mx = wave_all(mx, [](int a, int b) { return a > b ? a : b; });
    orb = wave_all(orb, [](uint32_t a, uint32_t b) { return a | b; });
    andb = wave_all(andb, [](uint32_t a, uint32_t b) { return a & b; });
    if (lane_id() == 0 && mn <= mx) {                                     // this wave saw a sample
        add64(reinterpret_cast<uint64_t *>(&acc->sum), (uint64_t)s);
        add64(&acc->sumsq, ss);
        atomicMin(&acc->min, mn);
        atomicMax(&acc->max, mx);
        atomicOr(&acc->or_bits, orb);
        atomicAnd(&acc->and_bits, andb);
    }
    if (threadIdx.x == 0) {
        if (reads) {
            add64(&acc->n_reads, reads);
            atomicMin(&acc->len_min, len_min);
            atomicMax(&acc->len_max, len_max);
        }
        if (failed) add64(&acc->n_failed, failed);
        if (samples) add64(&acc->n_samples, samples);
        if (other) add64(&acc->rg_other, other);
    }
}

// The floor tools/fstats_time.py holds k_file_stats against: every 16 bytes of p[0, bytes) loaded once, a lane per 16 bytes, and folded into one
// word per wave so that no load can be dropped.  s5tool_read_floor_dev is a hook of that tool, not part of the C ABI of include/slow5gpu.h.
__global__ __launch_bounds__(NT) void k_read_floor(const uint4 *__restrict__ p, uint64_t n16, uint32_t *__restrict__ out) {
    uint32_t x = 0;
    for (uint64_t k = (uint64_t)blockIdx.x * NT + threadIdx.x; k < n16; k += (uint64_t)gridDim.x * NT) {
        const uint4 u = p[k];
        x ^= u.x ^ u.y ^ u.z ^ u.w;
    }
    x = wave_all(x, [](uint32_t a, uint32_t b) { return a ^ b; });
    if (lane_id() == 0) atomicXor(out, x);
}

int fsk::set_option(const char *key, long value) {
    if (!key) return S5GPU_ERR_ARG;
    if (strcmp(key, "fstats_window_lo") == 0 && value >= -1 && value <= 65535) { g_opts.win_lo = (int32_t)value; return S5GPU_OK; }
    if (strcmp(key, "fstats_lds_bins") == 0 && (value == 0 || (value >= 64 && value <= (long)MAX_BINS && (value & (value - 1)) == 0))) {
        g_opts.bins = (uint32_t)value;
        return S5GPU_OK;
    }
    if (strcmp(key, "fstats_grid") == 0 && value >= 1 && value <= (long)MAX_GRID) { g_grid = (uint32_t)value; return S5GPU_OK; }
    if (strcmp(key, "fstats_flush_samples") == 0 && value >= 1 && value <= 0xFFFFFFFFl) { g_opts.flush = (uint32_t)value; return S5GPU_OK; }
    return S5GPU_ERR_ARG;
}

extern "C" int s5tool_read_floor_dev(const void *p, uint64_t bytes, uint32_t *out, void *stream) {
    if (!p || !out || ((uintptr_t)p & 15u) || ((uintptr_t)out & 3u)) { s5gpu_set_error("s5tool_read_floor_dev: NULL or misaligned argument"); return S5GPU_ERR_ARG; }
    const uint64_t n16 = bytes / 16;
    if (n16 == 0) return S5GPU_OK;
    const uint64_t blocks = (n16 + NT - 1) / NT;
    hipLaunchKernelGGL(k_read_floor, dim3((uint32_t)(blocks < 8192 ? blocks : 8192)), dim3(NT), 0, (hipStream_t)stream, (const uint4 *)p, n16, out);
    S5_LAUNCH_CHECK("k_read_floor");
    return S5GPU_OK;
}

int fsk::launch_reset(s5gpu_file_stats_t *acc, hipStream_t st) {
    hipLaunchKernelGGL(k_file_stats_reset, dim3(64), dim3(NT), 0, st, reinterpret_cast<uint64_t *>(acc));
    S5_LAUNCH_CHECK("k_file_stats_reset");
    return S5GPU_OK;
}

int fsk::launch_add_failed(s5gpu_file_stats_t *acc, uint32_t k, hipStream_t st) {
    if (k == 0) return S5GPU_OK;
    hipLaunchKernelGGL(k_file_stats_add_failed, dim3(1), dim3(64), 0, st, acc, k);
    S5_LAUNCH_CHECK("k_file_stats_add_failed");
    return S5GPU_OK;
}

int fsk::launch_accum(const sigk::SigRecs &R, s5gpu_file_stats_t *acc, hipStream_t st) {
    if (R.n == 0) return S5GPU_OK;
    const Opts O = g_opts;
    const uint32_t grid = R.n < g_grid ? R.n : g_grid;                    // by default four resident workgroups per CU: the tables are emptied once per workgroup
    hipLaunchKernelGGL(k_file_stats, dim3(grid), dim3(NT), (size_t)O.bins * COPIES * sizeof(uint32_t), st, R, O, acc);
    S5_LAUNCH_CHECK("k_file_stats");
    return S5GPU_OK;
}
