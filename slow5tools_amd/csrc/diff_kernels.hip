// diff_kernels.hip — k_sig_diff: per-pair signal error and field differences between TWO decoded batches, and the file-wide accumulator that
// stays on the device (docs/codecs.md §4.14).  Every member is an integer sum, maximum or count, so the result does not depend on the launch
// shape or on the order of the adds.  The construction rules are those of fstats_kernels.hip:
//   1. the sample count of each side is Side::n_eff (0 for a failed record, never past the record's slot), n_cmp = min of the two, nothing else;
//      a pair index is tested against its batch's record count before anything is loaded through it;
//   2. every index is a masked bit field behind a range test: LDS bins of (d + bins / 2) & (bins - 1), acc->hist of (d + 65535) & 0x1FFFF
//      behind < 131071; the id and aux bytes are loaded only after both ranges are shown to lie inside their own payload slots;
//   3. every loop's trip count is fixed by n_eff, the pair count, the bin count or the checked id / aux lengths; the flush points depend on
//      n_eff alone;
//   4. nothing waits on data: the only synchronisation is the workgroup barrier of a pair's reduction and around a flush, and every condition
//      in front of one is computed from values all threads of the workgroup load from the same addresses: reached by all threads or by none.
#include <stddef.h>
#include <string.h>

#include "dev_common.h"
#include "diff_dev.h"

extern "C" void s5gpu_set_error(const char *fmt, ...);

using namespace s5;

static_assert(sizeof(s5gpu_sig_diff_t) == 80 && offsetof(s5gpu_sig_diff_t, sum_d) == 40, "include/slow5gpu.h fixes this layout; k_sig_diff writes it as ten 8-byte words");
static_assert(sizeof(s5gpu_diff_acc_t) == 1048696 && offsetof(s5gpu_diff_acc_t, n_samples) == 64 && offsetof(s5gpu_diff_acc_t, max_abs) == 120 &&
                  offsetof(s5gpu_diff_acc_t, hist) == 128,
              "include/slow5gpu.h fixes this layout");

namespace {

dfk::Opts g_opts = {dfk::DEFAULT_BINS, 0xFFFFFFFFu};
uint32_t g_grid = dfk::MAX_GRID;   // option "diff_grid"

constexpr uint32_t NONE = S5GPU_DIFF_NONE;

__device__ __forceinline__ void add64(uint64_t *p, uint64_t v) { atomicAdd(reinterpret_cast<unsigned long long *>(p), (unsigned long long)v); }

template <class T, class Op>
__device__ __forceinline__ T wave_all(T v, Op op) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = op(v, __shfl_xor(v, d));
    return v;
}

// what one wave found in a pair
struct Part {
    uint32_t n_diff, first, fl, pad;
    unsigned long long key;            // (max_abs << 32) | ~max_at: one 64-bit max keeps the SMALLEST index among equal maxima
    long long sd;
    unsigned long long sabs, ssq;
    long long sa;
    unsigned long long ssa;
};

__device__ __forceinline__ uint64_t bits_of(double x) { return (uint64_t)__double_as_longlong(x); }

// does what f says of the payload lie inside a slot of cap bytes?  (digk::pieces_of's test)
__device__ __forceinline__ bool payload_ok(const s5gpu_rec_fields_t &f, uint32_t cap) {
    const uint64_t hl = 2ull + f.read_id_len + 36ull;
    return hl <= cap && f.aux_off <= cap && f.aux_len <= cap - f.aux_off;
}

}  // namespace

__global__ __launch_bounds__(NT) void k_diff_acc_reset(uint64_t *__restrict__ w) {
    constexpr uint32_t WORDS = sizeof(s5gpu_diff_acc_t) / 8;
    for (uint32_t k = blockIdx.x * NT + threadIdx.x; k < WORDS; k += gridDim.x * NT) w[k] = 0;
}

__global__ void k_diff_add_failed(s5gpu_diff_acc_t *acc, uint32_t k) {
    if (blockIdx.x == 0 && threadIdx.x == 0) { add64(&acc->n_pairs, k); add64(&acc->n_failed, k); }
}

// A workgroup walks the pairs blockIdx.x, blockIdx.x + gridDim.x, ...; all its threads share a pair's samples: 16-byte loads on both sides over
// the whole groups of eight (both slots start at multiples of 8 samples), the tail sample by sample.  A pair's sums go registers -> wave -> LDS
// -> thread 0, which writes the pair's row and keeps the workgroup's totals until the end.  Differences d != 0 inside [-bins / 2, bins / 2) are
// counted in LDS, COPIES counters per bin; others are global atomics; d == 0 is not counted per sample at all: bin 65535 gets n_samples - n_diff.
__global__ __launch_bounds__(NT) void k_sig_diff(uint32_t n_pairs, const uint32_t *__restrict__ pair_a, const uint32_t *__restrict__ pair_b, dfk::Side A,
                                                 dfk::Side B, dfk::Opts O, s5gpu_sig_diff_t *__restrict__ out, s5gpu_diff_acc_t *__restrict__ acc) {
    extern __shared__ __attribute__((aligned(16))) uint32_t df_win[];     // bins * COPIES counters
    __shared__ Part s_red[2][NW];
    const bool hist_on = acc != nullptr;
    const uint32_t bins = hist_on ? O.bins : 0u, bmask = bins - 1u, half = bins >> 1;
    for (uint32_t t = threadIdx.x; t < bins * dfk::COPIES; t += NT) df_win[t] = 0;
    __syncthreads();
    const uint32_t copy = threadIdx.x & (dfk::COPIES - 1u);

    auto flush = [&]() {                                                  // (called by every thread of the workgroup or by none)
        __syncthreads();
        for (uint32_t b = threadIdx.x; b < bins; b += NT) {
            uint4 *c = reinterpret_cast<uint4 *>(df_win + b * dfk::COPIES);
            uint64_t t = 0;
#pragma unroll
            for (uint32_t q = 0; q < dfk::COPIES / 4; q++) { const uint4 u = c[q]; t += (uint64_t)u.x + u.y + u.z + u.w; }
            if (t) {
                const uint32_t at = dfk::ZERO_BIN - half + b;             // 65535 - 128 .. 65535 + 127
                if (at < (uint32_t)S5GPU_DIFF_BINS) add64(&acc->hist[at & 0x1FFFFu], t);
#pragma unroll
                for (uint32_t q = 0; q < dfk::COPIES / 4; q++) c[q] = make_uint4(0, 0, 0, 0);
            }
        }
        __syncthreads();
    };

    // the same in every thread: they depend on the pair's flags and n_cmp alone
    uint64_t c_pairs = 0, c_failed = 0, c_differ = 0, c_signal = 0, c_len = 0, c_fields = 0, c_aux = 0, c_id = 0, c_samples = 0, since = 0;
    // the workgroup's sums: meaningful in thread 0
    uint64_t t_ndiff = 0, t_sabs = 0, t_ssq = 0, t_ssa = 0;
    int64_t t_sd = 0, t_sa = 0;
    uint32_t t_max = 0;
    uint32_t parity = 0;

    for (uint32_t p = blockIdx.x; p < n_pairs; p += gridDim.x) {
        const uint32_t ia = pair_a[p], ib = pair_b[p];
        c_pairs++;
        uint64_t *row = out ? reinterpret_cast<uint64_t *>(out + p) : nullptr;
        const bool bad = ia >= A.n || ib >= B.n;
        s5gpu_rec_fields_t fa, fb;
        uint32_t na = 0, nb = 0;
        bool failed = bad;
        const bool pay = A.payload && B.payload;
        if (!bad) {
            fa = A.fields[ia];
            fb = B.fields[ib];
            int32_t sta, stb;
            na = A.n_eff(ia, &sta);
            nb = B.n_eff(ib, &stb);
            failed = sta != 0 || stb != 0;
            if (!failed && pay) failed = !payload_ok(fa, A.pc(ia)) || !payload_ok(fb, B.pc(ib));
        }
        if (failed) {
            c_failed++;
            if (row && threadIdx.x == 0) {
                const uint32_t sa = bad ? 0u : (uint32_t)fa.status, sb = bad ? 0u : (uint32_t)fb.status;
                row[0] = (uint64_t)sa | ((uint64_t)sb << 32);
                row[1] = 0;
                row[2] = (uint64_t)(bad ? S5GPU_DIFF_BAD_PAIR : S5GPU_DIFF_FAILED);
                row[3] = (uint64_t)NONE;                                  // first_diff | max_abs
                row[4] = (uint64_t)NONE;                                  // max_at | reserved
                row[5] = 0; row[6] = 0; row[7] = 0; row[8] = 0; row[9] = 0;
            }
            continue;
        }
        const uint32_t n = na < nb ? na : nb;
        uint32_t fl = 0;                                                  // the flags every thread knows
        if (na != nb) fl |= S5GPU_DIFF_LEN;
        if (fa.read_group != fb.read_group) fl |= S5GPU_DIFF_READ_GROUP;
        if (bits_of(fa.digitisation) != bits_of(fb.digitisation)) fl |= S5GPU_DIFF_DIGITISATION;
        if (bits_of(fa.offset) != bits_of(fb.offset)) fl |= S5GPU_DIFF_OFFSET;
        if (bits_of(fa.range) != bits_of(fb.range)) fl |= S5GPU_DIFF_RANGE;
        if (bits_of(fa.sampling_rate) != bits_of(fb.sampling_rate)) fl |= S5GPU_DIFF_SAMPLING_RATE;
        uint32_t tfl = 0;                                                 // ... and what this thread found
        if (pay) {                                                        // (both ranges of both sides lie inside their slots: payload_ok)
            const uint8_t *pa = A.payload + A.po(ia), *pb = B.payload + B.po(ib);
            if (fa.read_id_len != fb.read_id_len) fl |= S5GPU_DIFF_ID;
            else
                for (uint32_t j = threadIdx.x; j < fa.read_id_len; j += NT)
                    if (pa[2u + j] != pb[2u + j]) tfl |= S5GPU_DIFF_ID;
            if (fa.aux_len != fb.aux_len) fl |= S5GPU_DIFF_AUX;
            else
                for (uint32_t j = threadIdx.x; j < fa.aux_len; j += NT)
                    if (pa[(uint64_t)fa.aux_off + j] != pb[(uint64_t)fb.aux_off + j]) tfl |= S5GPU_DIFF_AUX;
        }
        if (bins && since + n > (uint64_t)O.flush) { flush(); since = 0; }  // n < 2^32: the counters of one pair cannot wrap
        since += n;
        c_samples += n;

        uint32_t nd = 0, first = NONE, mabs = 0, mat = NONE;
        long long sd = 0, sa = 0, ssa = 0;
        unsigned long long sabs = 0, ssq = 0;
        int g_d = 0, g_a = 0;                                             // sums of at most eight samples: |.| <= 8 * 65535
        uint32_t g_abs = 0;
        auto one = [&](uint32_t i, int a, int b) {                        // (a thread's i only grow: its first difference is its smallest)
            const int d = b - a;
            const uint32_t ad = (uint32_t)(d < 0 ? -d : d);
            g_d += d; g_a += a; g_abs += ad;
            ssq += (unsigned long long)ad * ad;
            ssa += (long long)a * a;
            if (d != 0) {
                nd++;
                first = first < i ? first : i;
                if (ad > mabs) { mabs = ad; mat = i; }
                if (hist_on) {
                    const uint32_t w = (uint32_t)d + half, at = (uint32_t)(d + (int)dfk::ZERO_BIN);
                    if (w < bins) atomicAdd(&df_win[(w & bmask) * dfk::COPIES + copy], 1u);
                    else if (at < (uint32_t)S5GPU_DIFF_BINS) add64(&acc->hist[at & 0x1FFFFu], 1);
                }
            }
        };
        auto fold = [&]() { sd += g_d; sa += g_a; sabs += g_abs; g_d = 0; g_a = 0; g_abs = 0; };
        const uint64_t oa = A.o(ia), ob = B.o(ib);
        const int16_t *qa = A.sig + oa, *qb = B.sig + ob;
        const uint32_t nv = ((oa | ob) & 7u) == 0 ? n >> 3 : 0u;
        const uint4 *va = reinterpret_cast<const uint4 *>(qa), *vb = reinterpret_cast<const uint4 *>(qb);
        for (uint32_t k = threadIdx.x; k < nv; k += NT) {
            const uint4 u = va[k], v = vb[k];
            const uint32_t i = k << 3;
            one(i, (int)(int16_t)(u.x & 0xFFFFu), (int)(int16_t)(v.x & 0xFFFFu)); one(i + 1, (int)(int16_t)(u.x >> 16), (int)(int16_t)(v.x >> 16));
            one(i + 2, (int)(int16_t)(u.y & 0xFFFFu), (int)(int16_t)(v.y & 0xFFFFu)); one(i + 3, (int)(int16_t)(u.y >> 16), (int)(int16_t)(v.y >> 16));
            one(i + 4, (int)(int16_t)(u.z & 0xFFFFu), (int)(int16_t)(v.z & 0xFFFFu)); one(i + 5, (int)(int16_t)(u.z >> 16), (int)(int16_t)(v.z >> 16));
            one(i + 6, (int)(int16_t)(u.w & 0xFFFFu), (int)(int16_t)(v.w & 0xFFFFu)); one(i + 7, (int)(int16_t)(u.w >> 16), (int)(int16_t)(v.w >> 16));
            fold();
        }
        for (uint32_t i = (nv << 3) + threadIdx.x; i < n; i += NT) { one(i, (int)qa[i], (int)qb[i]); fold(); }

        // registers -> wave
        Part W;
        W.n_diff = wave_all(nd, [](uint32_t x, uint32_t y) { return x + y; });
        W.first = wave_all(first, [](uint32_t x, uint32_t y) { return x < y ? x : y; });
        W.fl = wave_all(tfl, [](uint32_t x, uint32_t y) { return x | y; });
        W.pad = 0;
        W.key = wave_all(((unsigned long long)mabs << 32) | (uint32_t)~mat, [](unsigned long long x, unsigned long long y) { return x > y ? x : y; });
        W.sd = wave_all(sd, [](long long x, long long y) { return x + y; });
        W.sabs = wave_all(sabs, [](unsigned long long x, unsigned long long y) { return x + y; });
        W.ssq = wave_all(ssq, [](unsigned long long x, unsigned long long y) { return x + y; });
        W.sa = wave_all(sa, [](long long x, long long y) { return x + y; });
        W.ssa = (unsigned long long)wave_all(ssa, [](long long x, long long y) { return x + y; });
        // wave -> LDS -> thread 0.  Two buffers taken in turn: a wave writes a buffer again only after the barrier of the pair in between, which
        // thread 0 reaches after it has read the buffer.  The flags of the pair come back to every thread through the same buffer.
        if (lane_id() == 0) s_red[parity][wave_id()] = W;
        __syncthreads();
        Part S = s_red[parity][0];
#pragma unroll
        for (int w = 1; w < NW; w++) {
            const Part X = s_red[parity][w];
            S.n_diff += X.n_diff;
            S.first = S.first < X.first ? S.first : X.first;
            S.fl |= X.fl;
            S.key = S.key > X.key ? S.key : X.key;
            S.sd += X.sd; S.sabs += X.sabs; S.ssq += X.ssq; S.sa += X.sa; S.ssa += X.ssa;
        }
        parity ^= 1u;
        fl |= S.fl;
        if (S.n_diff) fl |= S5GPU_DIFF_SIGNAL;
        if (fl) c_differ++;
        if (fl & S5GPU_DIFF_SIGNAL) c_signal++;
        if (fl & S5GPU_DIFF_LEN) c_len++;
        if (fl & (S5GPU_DIFF_READ_GROUP | S5GPU_DIFF_DIGITISATION | S5GPU_DIFF_OFFSET | S5GPU_DIFF_RANGE | S5GPU_DIFF_SAMPLING_RATE)) c_fields++;
        if (fl & S5GPU_DIFF_AUX) c_aux++;
        if (fl & S5GPU_DIFF_ID) c_id++;
        if (threadIdx.x == 0) {
            const uint32_t max_abs = (uint32_t)(S.key >> 32), max_at = S.n_diff ? ~(uint32_t)S.key : NONE;
            if (row) {
                row[0] = 0;                                               // both statuses are 0
                row[1] = (uint64_t)na | ((uint64_t)nb << 32);
                row[2] = (uint64_t)fl | ((uint64_t)S.n_diff << 32);
                row[3] = (uint64_t)S.first | ((uint64_t)max_abs << 32);
                row[4] = (uint64_t)max_at;
                row[5] = (uint64_t)S.sd; row[6] = S.sabs; row[7] = S.ssq; row[8] = (uint64_t)S.sa; row[9] = S.ssa;
            }
            t_ndiff += S.n_diff;
            t_max = t_max > max_abs ? t_max : max_abs;
            t_sd += S.sd; t_sabs += S.sabs; t_ssq += S.ssq; t_sa += S.sa; t_ssa += S.ssa;
        }
    }
    if (!hist_on) return;
    flush();
    if (threadIdx.x == 0) {
        if (c_pairs) add64(&acc->n_pairs, c_pairs);
        if (c_failed) add64(&acc->n_failed, c_failed);
        if (c_differ) add64(&acc->n_differ, c_differ);
        if (c_signal) add64(&acc->n_signal, c_signal);
        if (c_len) add64(&acc->n_len, c_len);
        if (c_fields) add64(&acc->n_fields, c_fields);
        if (c_aux) add64(&acc->n_aux, c_aux);
        if (c_id) add64(&acc->n_id, c_id);
        if (c_samples) {
            add64(&acc->n_samples, c_samples);
            add64(&acc->n_diff, t_ndiff);
            add64(reinterpret_cast<uint64_t *>(&acc->sum_d), (uint64_t)t_sd);
            add64(&acc->sum_abs, t_sabs);
            add64(&acc->sum_sq, t_ssq);
            add64(reinterpret_cast<uint64_t *>(&acc->sum_a), (uint64_t)t_sa);
            add64(&acc->sumsq_a, t_ssa);
            atomicMax(&acc->max_abs, t_max);
            if (c_samples > t_ndiff) add64(&acc->hist[dfk::ZERO_BIN], c_samples - t_ndiff);   // the samples with d == 0
        }
    }
}

int dfk::set_option(const char *key, long value) {
    if (!key) return S5GPU_ERR_ARG;
    if (strcmp(key, "diff_lds_bins") == 0 && (value == 0 || (value >= (long)MIN_BINS && value <= (long)MAX_BINS && (value & (value - 1)) == 0))) {
        g_opts.bins = (uint32_t)value;
        return S5GPU_OK;
    }
    if (strcmp(key, "diff_grid") == 0 && value >= 1 && value <= (long)MAX_GRID) { g_grid = (uint32_t)value; return S5GPU_OK; }
    if (strcmp(key, "diff_flush_samples") == 0 && value >= 1 && value <= 0xFFFFFFFFl) { g_opts.flush = (uint32_t)value; return S5GPU_OK; }
    return S5GPU_ERR_ARG;
}

int dfk::launch_reset(s5gpu_diff_acc_t *acc, hipStream_t st) {
    hipLaunchKernelGGL(k_diff_acc_reset, dim3(128), dim3(NT), 0, st, reinterpret_cast<uint64_t *>(acc));
    S5_LAUNCH_CHECK("k_diff_acc_reset");
    return S5GPU_OK;
}

int dfk::launch_add_failed(s5gpu_diff_acc_t *acc, uint32_t k, hipStream_t st) {
    if (k == 0) return S5GPU_OK;
    hipLaunchKernelGGL(k_diff_add_failed, dim3(1), dim3(64), 0, st, acc, k);
    S5_LAUNCH_CHECK("k_diff_add_failed");
    return S5GPU_OK;
}

int dfk::launch_diff(uint32_t n_pairs, const uint32_t *pair_a, const uint32_t *pair_b, const Side &A, const Side &B, s5gpu_sig_diff_t *out,
                     s5gpu_diff_acc_t *acc, hipStream_t st) {
    if (n_pairs == 0 || (!out && !acc)) return S5GPU_OK;
    const Opts O = g_opts;
    const uint32_t grid = n_pairs < g_grid ? n_pairs : g_grid;            // by default four resident workgroups per CU
    hipLaunchKernelGGL(k_sig_diff, dim3(grid), dim3(NT), acc ? (size_t)O.bins * COPIES * sizeof(uint32_t) : 0, st, n_pairs, pair_a, pair_b, A, B, O,
                       out, acc);
    S5_LAUNCH_CHECK("k_sig_diff");
    return S5GPU_OK;
}
