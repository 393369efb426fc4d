// signal_kernels.hip — what a signal consumer does first with decoded reads, on the device (docs/codecs.md §4.11):
//   k_sig_stats   : per read min / max / sum / sum of squares, 2 x median, 4 x MAD and up to four quantiles, all exact integers
//   k_sig_windows : a dense [n_windows, W] float32 / float16 tensor of normalised samples, cut from the reads by (read, start) windows
// Neither kernel can index outside what it owns by construction:
//   1. the sample count of a record is SigRecs::n_eff (0 for a failed record, never past the record's slot), nothing else;
//   2. every LDS histogram index is a masked bit field of a key: no data value, rank or count forms an address;
//   3. every loop's trip count is fixed by n_eff or by the key width: no loop waits for data to converge;
//   4. a window descriptor is validated on the device before anything is loaded through it: a bad one gives a row of zeros.
#include <hip/hip_fp16.h>

#include "dev_common.h"
#include "signal_dev.h"

extern "C" void s5gpu_set_error(const char *fmt, ...);

using namespace s5;

namespace {

// ---- exact radix select over the key domain ----
// Keys have at most 17 bits (samples after the bias x - min: 16; MAD keys |2x - med2|: 17).  The largest key of a read is known before the
// select starts (max - min; the larger of |2 min - med2| and |2 max - med2|), so the key's width B is: the first pass histograms the TOP
// nine bits of those B (shift s1 = B - 9, or 0), the second the s1 <= 8 bits below, of the keys that fell into the bin the rank lies in.
// Raw signals span about a thousand levels: their nine top bits are spread over hundreds of bins, where the high byte of the sample itself
// would put every lane's LDS atomic onto three or four of them.  Two passes whatever the data; the second is skipped when B <= 9.
// All wanted ranks (two for the median, up to four quantiles) go through the same two passes: the first histogram serves them all, the second
// keeps one 256-bin histogram per distinct first-pass bin.
constexpr int SEL_B1 = 9, SEL_BINS1 = 1 << SEL_B1, SEL_BINS2 = 256, SEL_MAXR = 6;

struct StatsLds {
    uint32_t h1[SEL_BINS1];
    uint32_t h2[SEL_MAXR][SEL_BINS2];
    uint32_t bin[SEL_MAXR], rem[SEL_MAXR], low[SEL_MAXR], rem2[SEL_MAXR], key[SEL_MAXR];
    long long sum[NW];
    unsigned long long sumsq[NW];
    int mn[NW], mx[NW];
};

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

// One wave: the bin of h[0, 64 * PL) that holds rank rk (counted from 0) and rk's rank inside that bin.  Lane l sums bins [l * PL, (l + 1) * PL);
// the lane whose range of ranks holds rk walks its PL bins.  If rk is not below the total nobody writes (the caller's zeros stay).
template <int PL>
__device__ __forceinline__ void wave_locate(const uint32_t *h, uint32_t rk, uint32_t *bin_out, uint32_t *rem_out) {
    const uint32_t lane = lane_id();
    uint32_t c[PL], tot = 0;
#pragma unroll
    for (int j = 0; j < PL; j++) { c[j] = h[lane * PL + j]; tot += c[j]; }
    const uint32_t inc = wave_incl_add(tot), exc = inc - tot;
    if (rk >= exc && rk < inc) {
        uint32_t a = exc, sel = 0, base = exc;
        bool found = false;
#pragma unroll
        for (int j = 0; j < PL; j++) {
            if (!found) {
                if (rk < a + c[j]) { sel = j; base = a; found = true; }
                else a += c[j];
            }
        }
        *bin_out = lane * PL + sel;
        *rem_out = rk - base;
    }
}

// L.key[r] = the key of rank rank[r] among key(x) of the n samples, r < nr <= SEL_MAXR.  kmax: an upper bound of every key (< 2^17).
// Called by the whole workgroup; ends behind a barrier.
template <class KeyF>
__device__ __forceinline__ void select_ranks(StatsLds &L, const int16_t *p, uint32_t n, bool vec, KeyF key, uint32_t kmax, const uint32_t (&rank)[SEL_MAXR],
                                             int nr) {
    const uint32_t B = 32u - (uint32_t)__builtin_clz(kmax | 1u);
    uint32_t s1 = B > (uint32_t)SEL_B1 ? B - SEL_B1 : 0u;
    if (s1 > 8u) s1 = 8u;
    const uint32_t low_mask = (1u << s1) - 1u;                       // <= 255
    for (uint32_t t = threadIdx.x; t < (uint32_t)SEL_BINS1; t += NT) L.h1[t] = 0;
    for (uint32_t t = threadIdx.x; t < (uint32_t)(SEL_MAXR * SEL_BINS2); t += NT) (&L.h2[0][0])[t] = 0;
    if (threadIdx.x < (uint32_t)SEL_MAXR) { L.bin[threadIdx.x] = 0; L.rem[threadIdx.x] = 0; L.low[threadIdx.x] = 0; L.rem2[threadIdx.x] = 0; }
    __syncthreads();
    for_each_sample(p, n, vec, [&](int x) { atomicAdd(&L.h1[(key(x) >> s1) & (uint32_t)(SEL_BINS1 - 1)], 1u); });
    __syncthreads();
    if (wave_id() == 0) {
#pragma unroll
        for (int r = 0; r < SEL_MAXR; r++)
            if (r < nr) wave_locate<SEL_BINS1 / 64>(L.h1, rank[r], &L.bin[r], &L.rem[r]);
    }
    __syncthreads();
    uint32_t bin[SEL_MAXR];
    int owner[SEL_MAXR];                                             // the first rank with the same first-pass bin: its histogram is shared
#pragma unroll
    for (int r = 0; r < SEL_MAXR; r++) {
        bin[r] = r < nr ? L.bin[r] : 0xFFFFFFFFu;
        owner[r] = r;
#pragma unroll
        for (int q = SEL_MAXR - 1; q >= 0; q--)
            if (q < r && bin[q] == bin[r]) owner[r] = q;
    }
    if (s1 == 0) {                                                    // uniform: the first field was the whole key
        if (threadIdx.x == 0) {
#pragma unroll
            for (int r = 0; r < SEL_MAXR; r++)
                if (r < nr) L.key[r] = bin[r];
        }
        __syncthreads();
        return;
    }
    for_each_sample(p, n, vec, [&](int x) {
        const uint32_t k = key(x), f1 = (k >> s1) & (uint32_t)(SEL_BINS1 - 1), low = k & low_mask;
#pragma unroll
        for (int r = 0; r < SEL_MAXR; r++)
            if (r < nr && owner[r] == r && f1 == bin[r]) atomicAdd(&L.h2[r][low], 1u);
    });
    __syncthreads();
    if (wave_id() == 0) {
#pragma unroll
        for (int r = 0; r < SEL_MAXR; r++) {
            if (r < nr) {
                const uint32_t *h = L.h2[0];
#pragma unroll
                for (int q = 0; q < SEL_MAXR; q++)
                    if (owner[r] == q) h = L.h2[q];
                wave_locate<SEL_BINS2 / 64>(h, L.rem[r], &L.low[r], &L.rem2[r]);
            }
        }
    }
    __syncthreads();
    if (threadIdx.x < (uint32_t)SEL_MAXR) L.key[threadIdx.x] = (L.bin[threadIdx.x] << s1) | (L.low[threadIdx.x] & low_mask);
    __syncthreads();
}


template <class T>
__device__ __forceinline__ T wave_reduce(T v, T (*op)(T, T)) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = op(v, __shfl_xor(v, d));
    return v;
}

}  // namespace

// One read per workgroup at a time; the grid's workgroups walk the reads with a stride.  Five passes over a read at most (first moments and
// extremes; two for the sample ranks; two for the MAD ranks): a 4000-sample read is 8 KB and stays in L2 between them.  One workgroup per
// read is also how a 100 k-sample read is served; where that stops being fine has not been measured.
__global__ __launch_bounds__(NT) void k_sig_stats(sigk::SigRecs R, sigk::Quantiles Q, s5gpu_sig_stats_t *__restrict__ stats) {
    __shared__ StatsLds L;
    const int nq = Q.n < 4u ? (int)Q.n : 4;
    for (uint32_t i = blockIdx.x; i < R.n; i += gridDim.x) {
        int32_t status;
        const uint32_t n = R.n_eff(i, &status);
        s5gpu_sig_stats_t out;
        out.n = n; out.status = status; out.sum = 0; out.sumsq = 0; out.med2 = 0; out.mad4 = 0; out.min = 0; out.max = 0;
        out.q[0] = out.q[1] = out.q[2] = out.q[3] = 0; out.reserved = 0;
        if (n == 0) {                                                 // (uniform: n is the same for every thread)
            if (threadIdx.x == 0) stats[i] = out;
            continue;
        }
        const uint64_t o = R.o(i);
        const int16_t *p = R.sig + o;
        const bool vec = (o & 7u) == 0;
        // pass 0: extremes and moments
        int mn = 32767, mx = -32768;
        long long s = 0;
        unsigned long long ss = 0;
        for_each_sample(p, n, vec, [&](int x) { mn = min(mn, x); mx = max(mx, x); s += x; ss += (uint32_t)(x * x); });
        mn = wave_reduce<int>(mn, [](int a, int b) { return a < b ? a : b; });
        mx = wave_reduce<int>(mx, [](int a, int b) { return a > b ? a : b; });
        s = wave_reduce<long long>(s, [](long long a, long long b) { return a + b; });
        ss = wave_reduce<unsigned long long>(ss, [](unsigned long long a, unsigned long long b) { return a + b; });
        if (lane_id() == 0) { L.mn[wave_id()] = mn; L.mx[wave_id()] = mx; L.sum[wave_id()] = s; L.sumsq[wave_id()] = ss; }
        __syncthreads();
        mn = L.mn[0]; mx = L.mx[0]; s = L.sum[0]; ss = L.sumsq[0];
#pragma unroll
        for (int w = 1; w < NW; w++) { mn = min(mn, L.mn[w]); mx = max(mx, L.mx[w]); s += L.sum[w]; ss += L.sumsq[w]; }
        // sample ranks: the two of the median, then the quantiles; keys x - min (0 .. 65535)
        uint32_t rank[SEL_MAXR];
        rank[0] = (n - 1) / 2; rank[1] = n / 2;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            uint32_t r = 0;
            if (k < nq) {
                const double t = floor(Q.q[k] * (double)(n - 1));
                r = t > 0.0 ? (t < (double)(n - 1) ? (uint32_t)t : n - 1) : 0u;
            }
            rank[2 + k] = r;
        }
        select_ranks(L, p, n, vec, [mn](int x) { return (uint32_t)(x - mn); }, (uint32_t)(mx - mn), rank, 2 + nq);
        const int v0 = mn + (int)L.key[0], v1 = mn + (int)L.key[1];
        out.q[0] = (int16_t)(nq > 0 ? mn + (int)L.key[2] : 0); out.q[1] = (int16_t)(nq > 1 ? mn + (int)L.key[3] : 0);
        out.q[2] = (int16_t)(nq > 2 ? mn + (int)L.key[4] : 0); out.q[3] = (int16_t)(nq > 3 ? mn + (int)L.key[5] : 0);
        const int med2 = v0 + v1;
        // MAD ranks: keys |2x - med2| (0 .. 131070)
        const int e0 = 2 * mn - med2, e1 = 2 * mx - med2;
        const uint32_t kmax = (uint32_t)max(e0 < 0 ? -e0 : e0, e1 < 0 ? -e1 : e1);
        select_ranks(L, p, n, vec, [med2](int x) { const int d = 2 * x - med2; return (uint32_t)(d < 0 ? -d : d); }, kmax, rank, 2);
        out.sum = s; out.sumsq = ss; out.min = (int16_t)mn; out.max = (int16_t)mx; out.med2 = med2;
        out.mad4 = L.key[0] + L.key[1];
        if (threadIdx.x == 0) stats[i] = out;
        __syncthreads();                                              // L.key and the reduction words are rewritten by the next read
    }
}

namespace {

// what one window needs to turn sample j of its read into an output value
struct WinP {
    const int16_t *p;     // sample 0 of the window
    uint32_t avail;       // samples of the read from the window's start on (0: a bad window, nothing is loaded)
    int mul, isub;        // float modes: float(mul * x - isub) / den
    float den;
    double A, B;          // double modes: float((double(x) + A) * B)
};

__device__ __forceinline__ WinP load_window(const sigk::SigRecs &R, const sigk::WinArgs &A, uint32_t w, bool first) {
    WinP P;
    P.p = R.sig; P.avail = 0; P.mul = 1; P.isub = 0; P.den = 1.0f; P.A = 0.0; P.B = 1.0;
    const uint32_t r = A.win_read[w], s = A.win_start[w];
    bool bad = true;
    if (r < R.n) {
        int32_t st;
        const uint32_t n = R.n_eff(r, &st);
        if (st == 0 && s <= n) {
            bad = false;
            P.p = R.sig + R.o(r) + s;
            P.avail = n - s;
            if (A.mode == S5GPU_NORM_PA) {
                P.A = R.fields[r].offset;
                P.B = R.fields[r].range / R.fields[r].digitisation;
            } else if (A.mode == S5GPU_NORM_MEDMAD) {
                const uint32_t mad4 = A.stats[r].mad4;
                P.mul = 2; P.isub = A.stats[r].med2;
                P.den = mad4 ? 0.7413f * (float)mad4 : 1.0f;
            } else if (A.mode == S5GPU_NORM_QUANT) {
                const int q0 = A.stats[r].q[0], q1 = A.stats[r].q[1];
                const double scale = A.b * (double)(q1 - q0);
                P.A = -(A.a * (double)(q0 + q1));
                P.B = 1.0 / (scale > 1.0 ? scale : 1.0);
            }
        }
    }
    if (first) A.win_status[w] = bad ? 1 : 0;
    return P;
}

template <bool DBL>
__device__ __forceinline__ float win_value(const WinP &P, int x) {
    if (DBL) return (float)(((double)x + P.A) * P.B);
    return (float)(P.mul * x - P.isub) / P.den;
}

}  // namespace

// The tensor is walked as one flat array in chunks of 8 elements, a chunk per lane: a 32-byte (float32) or 16-byte (float16) store per lane,
// consecutive lanes on consecutive chunks.  A chunk may run over the end of a row when W is no multiple of 8: the window is looked up again
// where a row starts.  The lane that writes element 0 of a row writes the row's status.  A chunk that lies inside one row, with all its eight
// samples present and 16-byte aligned (every chunk of the padded batch but a read's last, when W is a multiple of 8), takes them in one load;
// any other chunk takes them one by one.
template <bool DBL, bool HALF>
__global__ __launch_bounds__(NT) void k_sig_windows(sigk::SigRecs R, sigk::WinArgs A) {
    const uint64_t total = (uint64_t)A.n_windows * A.W, n_chunks = (total + 7) / 8;
    for (uint64_t c = (uint64_t)blockIdx.x * NT + threadIdx.x; c < n_chunks; c += (uint64_t)gridDim.x * NT) {
        const uint64_t e0 = c * 8;
        const uint32_t cnt = total - e0 < 8 ? (uint32_t)(total - e0) : 8u;
        uint32_t w = (e0 >> 32) ? (uint32_t)(e0 / A.W) : (uint32_t)e0 / A.W;
        uint32_t j = (uint32_t)(e0 - (uint64_t)w * A.W);
        WinP P = load_window(R, A, w, j == 0);
        float f[8];
        if (cnt == 8 && A.W - j >= 8 && P.avail >= 8 && j <= P.avail - 8 && ((uintptr_t)(P.p + j) & 15u) == 0) {
            // the chunk lies inside one row, all eight samples exist (below n_eff) and sit in one aligned 16 bytes: one load
            const uint4 u = *reinterpret_cast<const uint4 *>(P.p + j);
            const int x[8] = {(int)(int16_t)(u.x & 0xFFFFu), (int)(int16_t)(u.x >> 16), (int)(int16_t)(u.y & 0xFFFFu), (int)(int16_t)(u.y >> 16),
                              (int)(int16_t)(u.z & 0xFFFFu), (int)(int16_t)(u.z >> 16), (int)(int16_t)(u.w & 0xFFFFu), (int)(int16_t)(u.w >> 16)};
#pragma unroll
            for (int t = 0; t < 8; t++) f[t] = win_value<DBL>(P, x[t]);
        } else {
#pragma unroll
            for (int t = 0; t < 8; t++) {
                f[t] = 0.0f;
                if ((uint32_t)t < cnt) {                              // (so w < n_windows)
                    if (t && j == 0) P = load_window(R, A, w, true);
                    if (j < P.avail) f[t] = win_value<DBL>(P, (int)P.p[j]);
                    if (++j == A.W) { j = 0; w++; }
                }
            }
        }
        if (HALF) {
            __half *o = (__half *)A.out + e0;
            if (cnt == 8) {
                uint4 u;
                const __half2 h0 = __floats2half2_rn(f[0], f[1]), h1 = __floats2half2_rn(f[2], f[3]), h2 = __floats2half2_rn(f[4], f[5]),
                              h3 = __floats2half2_rn(f[6], f[7]);
                u.x = *reinterpret_cast<const uint32_t *>(&h0); u.y = *reinterpret_cast<const uint32_t *>(&h1);
                u.z = *reinterpret_cast<const uint32_t *>(&h2); u.w = *reinterpret_cast<const uint32_t *>(&h3);
                *reinterpret_cast<uint4 *>(o) = u;
            } else {
#pragma unroll
                for (int t = 0; t < 8; t++)
                    if ((uint32_t)t < cnt) o[t] = __float2half_rn(f[t]);
            }
        } else {
            float *o = (float *)A.out + e0;
            if (cnt == 8) {
                reinterpret_cast<float4 *>(o)[0] = make_float4(f[0], f[1], f[2], f[3]);
                reinterpret_cast<float4 *>(o)[1] = make_float4(f[4], f[5], f[6], f[7]);
            } else {
#pragma unroll
                for (int t = 0; t < 8; t++)
                    if ((uint32_t)t < cnt) o[t] = f[t];
            }
        }
    }
}

int sigk::launch_stats(const SigRecs &R, const Quantiles &Q, s5gpu_sig_stats_t *stats, hipStream_t st) {
    if (R.n == 0) return S5GPU_OK;
    const uint32_t grid = R.n < 8192u ? R.n : 8192u;                  // eight workgroups per CU and a few rounds of them: reads vary in length
    hipLaunchKernelGGL(k_sig_stats, dim3(grid), dim3(NT), 0, st, R, Q, stats);
    S5_LAUNCH_CHECK("k_sig_stats");
    return S5GPU_OK;
}

int sigk::launch_windows(const SigRecs &R, const WinArgs &A, int dtype, hipStream_t st) {
    const uint64_t total = (uint64_t)A.n_windows * A.W;
    if (total == 0) return S5GPU_OK;
    const uint64_t blocks = ((total + 7) / 8 + NT - 1) / NT;
    const dim3 grid((uint32_t)(blocks < 16384 ? blocks : 16384)), block(NT);
    const bool dbl = A.mode == S5GPU_NORM_PA || A.mode == S5GPU_NORM_QUANT, half = dtype == S5GPU_SIG_F16;
    if (dbl) { if (half) hipLaunchKernelGGL((k_sig_windows<true, true>), grid, block, 0, st, R, A); else hipLaunchKernelGGL((k_sig_windows<true, false>), grid, block, 0, st, R, A); }
    else { if (half) hipLaunchKernelGGL((k_sig_windows<false, true>), grid, block, 0, st, R, A); else hipLaunchKernelGGL((k_sig_windows<false, false>), grid, block, 0, st, R, A); }
    S5_LAUNCH_CHECK("k_sig_windows");
    return S5GPU_OK;
}
