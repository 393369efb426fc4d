// event_dev.h — what event_kernels.hip, event_api.hip and order_launch.hip share: the arguments of k_sig_events, a lane's walk over its read,
// the launchers, and the launch order by sample count (docs/codecs.md §4.15).
// With S5_EVENT_WALK_HOST defined only the walk is declared, as plain C++: tests/test_events.py compiles it for the CPU and runs the very
// code a lane runs against the restatement, without a device.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/slow5gpu.h"

#ifdef S5_EVENT_WALK_HOST
#define EV_HD static inline
#else
#include <hip/hip_runtime.h>

#include <mutex>

#include "signal_dev.h"
#define EV_HD __host__ __device__ __forceinline__
#endif

// every product and sum of the walk is rounded on its own (§4.15: no fused multiply-add); the pragma stands at the head of each function
// that computes in double, so that a translation unit that includes this header keeps its own mode
#ifdef __clang__
#define EV_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define EV_NO_CONTRACT
#endif

namespace evk {

struct EvArgs {
    uint32_t w1, w2;                 // checked by the host: 1 <= w1 < w2 <= 64
    double thr1, thr2, peak_height;
    int mode;                        // S5GPU_NORM_RAW or S5GPU_NORM_PA
    const uint64_t *ev_off;          // rows != nullptr: first row of read i, in rows
    const uint32_t *ev_cap;          //                  rows read i may write
    s5gpu_event_t *rows;             // nullptr: the count pass (ev_off / ev_cap are not read)
    uint32_t *n_events;
    int32_t *ev_status;
};

constexpr uint32_t CH = 32;          // samples a lane fetches at a time (64 bytes)
// slots of a lane's ring: the 2 w2 + 1 samples the windows at i reach, and the CH - 1 a refill puts in front of them
constexpr uint32_t ring_slots(uint32_t w2) { return (2 * w2 + CH + CH - 1) / CH * CH; }

struct alignas(16) U4 { uint32_t x, y, z, w; };    // 16 bytes moved at once: eight samples in, one row out

// where a read's rows go and how its mean and stdv are scaled
struct RowOut {
    U4 *row0;
    uint32_t cap;
    bool pa;
    double offset, scale;
};

// sqrt(num / den) of §4.15 for the windows [i - w, i) and [i, i + w): sums s1, s2 (|s| <= 64 * 32768), sums of squares q1, q2
EV_HD double t_stat(int s1, int s2, uint64_t q1, uint64_t q2, uint32_t w) {
    EV_NO_CONTRACT
    const long long d = (long long)s2 - s1;
    const uint64_t num = (uint64_t)(d * d) * w;                                             // < 2^50
    const uint64_t ss = (uint64_t)((long long)s1 * s1) + (uint64_t)((long long)s2 * s2);
    long long den = (long long)((q1 + q2) * w - ss);                                        // >= 0 (Cauchy-Schwarz), < 2^44
    if (den < 1) den = 1;
    return sqrt((double)num / (double)den);
}

EV_HD U4 make_row(uint32_t start, uint32_t L, long long S, unsigned long long Q, const RowOut &O) {
    EV_NO_CONTRACT
    const double Ld = (double)L, mean = (double)S / Ld;
    double m2 = mean * mean;
#ifdef __HIP_DEVICE_COMPILE__
    asm volatile("" : "+v"(m2));                                   // (the product is a value of its own whatever the contraction mode)
#endif
    const double var = (double)Q / Ld - m2;
    const double sd = sqrt(var > 0.0 ? var : 0.0);
    const float fm = O.pa ? (float)((mean + O.offset) * O.scale) : (float)mean;
    const float fs = O.pa ? (float)(sd * fabs(O.scale)) : (float)sd;
    U4 r;
    r.x = start; r.y = L;
    __builtin_memcpy(&r.z, &fm, 4); __builtin_memcpy(&r.w, &fs, 4);
    return r;
}

struct Det {
    uint64_t masked_to;
    uint32_t pos;
    bool has, valid;             // has: pos is set
    double val;
    long long sS;                // the running sums over [0, pos)
    unsigned long long sQ;
};

// One lane's walk over its read p[0, n): the events are counted and (FILL) the first O.cap of them stored at O.row0.  Returns the count.
//   nmax : the trip count's source, the same in every lane of the wave, >= n
//   vec  : p is 16-byte aligned
//   col  : the lane's ring column: slot s lives at col[s * pitch], slots [0, ring), ring = ring_slots(A.w2)
// One step per h = i + w2: sample h enters the ring, then the machine runs at i and the sums slide to i + 1.
template <bool FILL>
EV_HD uint32_t walk(const int16_t *p, uint32_t n, uint32_t nmax, bool vec, int16_t *col, uint32_t pitch, uint32_t ring, const EvArgs &A, const RowOut &O) {
    EV_NO_CONTRACT
    const uint32_t w1 = A.w1, w2 = A.w2;
    const double inf = __builtin_huge_val(), thr1 = A.thr1, thr2 = A.thr2, ph = A.peak_height;
    for (uint32_t s = 0; s < ring; s++) col[s * pitch] = 0;        // samples in front of the read are zeros
    Det D0 = {0, 0, false, false, inf, 0, 0}, D1 = D0;
    int a1 = 0, a2 = 0, b1 = 0, b2 = 0;                            // sums over [i - w, i) and [i, i + w)
    uint64_t qa1 = 0, qa2 = 0, qb1 = 0, qb2 = 0;
    long long PS = 0;                                              // sums over [0, i)
    unsigned long long PQ = 0;
    uint32_t cnt = 0, lastp = 0;
    long long lastS = 0;
    unsigned long long lastQ = 0;
    auto emit = [&](uint32_t at, long long Sp, unsigned long long Qp) {
        if (FILL) {
            if (cnt < O.cap) O.row0[cnt] = make_row(lastp, at - lastp, Sp - lastS, Qp - lastQ, O);
        }
        cnt++; lastp = at; lastS = Sp; lastQ = Qp;
    };
    // slots of the positions h (sb + k), i + w1, i, i - w1, i - w2: the same in every lane, each below `ring`
    uint32_t sb = 0, c_a = ring - w2 + w1, c_0 = ring - w2, c_m1 = ring - w2 - w1, c_m2 = ring - 2 * w2;
    const uint64_t steps = nmax ? (uint64_t)nmax + w2 : 0;
    for (uint64_t hb = 0; hb < steps; hb += CH) {
        if (vec && hb + CH <= (uint64_t)n) {                       // 64 bytes that lie inside the read, 16-byte aligned
            const U4 *v = reinterpret_cast<const U4 *>(p + hb);
#if defined(__clang__)
#pragma unroll
#endif
            for (uint32_t q = 0; q < CH / 8; q++) {
                const U4 u = v[q];
                int16_t *c = col + (sb + 8 * q) * pitch;
                c[0] = (int16_t)(u.x & 0xFFFFu); c[pitch] = (int16_t)(u.x >> 16); c[2 * pitch] = (int16_t)(u.y & 0xFFFFu); c[3 * pitch] = (int16_t)(u.y >> 16);
                c[4 * pitch] = (int16_t)(u.z & 0xFFFFu); c[5 * pitch] = (int16_t)(u.z >> 16); c[6 * pitch] = (int16_t)(u.w & 0xFFFFu); c[7 * pitch] = (int16_t)(u.w >> 16);
            }
        } else {
            for (uint32_t k = 0; k < CH; k++) {
                const uint64_t j = hb + k;
                col[(sb + k) * pitch] = j < (uint64_t)n ? p[j] : (int16_t)0;
            }
        }
        const uint32_t todo = steps - hb < CH ? (uint32_t)(steps - hb) : CH;
        for (uint32_t k = 0; k < todo; k++) {
            const long long i = (long long)(hb + k) - (long long)w2;
            const int xn = col[(sb + k) * pitch], xa = col[c_a * pitch], x0 = col[c_0 * pitch], xm1 = col[c_m1 * pitch], xm2 = col[c_m2 * pitch];
            if (i >= 0 && (uint64_t)i < (uint64_t)n) {
                const uint64_t iu = (uint64_t)i;
                const uint32_t i32 = (uint32_t)iu;
                const double t1 = iu >= w1 && iu + w1 <= (uint64_t)n ? t_stat(a1, b1, qa1, qb1, w1) : 0.0;
                const double t2 = iu >= w2 && iu + w2 <= (uint64_t)n ? t_stat(a2, b2, qa2, qb2, w2) : 0.0;
                if (!(D0.masked_to >= iu)) {                                   // the short detector
                    const double c = t1;
                    if (!D0.has) {
                        if (c < D0.val) D0.val = c;
                        else if (c - D0.val > ph) { D0.val = c; D0.pos = i32; D0.has = true; D0.sS = PS; D0.sQ = PQ; }
                    } else {
                        if (c > D0.val) { D0.val = c; D0.pos = i32; D0.sS = PS; D0.sQ = PQ; }
                        if (D0.val > thr1) { D1.masked_to = (uint64_t)D0.pos + w1; D1.has = false; D1.val = inf; D1.valid = false; }
                        if (D0.val - c > ph && D0.val > thr1) D0.valid = true;
                        if (D0.valid && i32 - D0.pos > w1 / 2) {
                            emit(D0.pos, D0.sS, D0.sQ);
                            D0.has = false; D0.val = c; D0.valid = false;
                        }
                    }
                }
                if (!(D1.masked_to >= iu)) {                                   // the long detector
                    const double c = t2;
                    if (!D1.has) {
                        if (c < D1.val) D1.val = c;
                        else if (c - D1.val > ph) { D1.val = c; D1.pos = i32; D1.has = true; D1.sS = PS; D1.sQ = PQ; }
                    } else {
                        if (c > D1.val) { D1.val = c; D1.pos = i32; D1.sS = PS; D1.sQ = PQ; }
                        if (D1.val - c > ph && D1.val > thr2) D1.valid = true;
                        if (D1.valid && i32 - D1.pos > w2 / 2) {
                            emit(D1.pos, D1.sS, D1.sQ);
                            D1.has = false; D1.val = c; D1.valid = false;
                        }
                    }
                }
            }
            // slide to i + 1 (samples outside [0, n) are zeros, in every lane)
            const uint32_t s0 = (uint32_t)(x0 * x0);
            a1 += x0 - xm1; qa1 += (uint64_t)s0 - (uint32_t)(xm1 * xm1);
            a2 += x0 - xm2; qa2 += (uint64_t)s0 - (uint32_t)(xm2 * xm2);
            b1 += xa - x0; qb1 += (uint64_t)(uint32_t)(xa * xa) - s0;
            b2 += xn - x0; qb2 += (uint64_t)(uint32_t)(xn * xn) - s0;
            PS += x0; PQ += s0;
            c_a = c_a + 1 == ring ? 0 : c_a + 1; c_0 = c_0 + 1 == ring ? 0 : c_0 + 1;
            c_m1 = c_m1 + 1 == ring ? 0 : c_m1 + 1; c_m2 = c_m2 + 1 == ring ? 0 : c_m2 + 1;
        }
        sb = sb + CH == ring ? 0 : sb + CH;                        // (ring is a multiple of CH)
    }
    if (n) emit(n, PS, PQ);                                        // the last event ends at n
    return cnt;
}

#ifndef S5_EVENT_WALK_HOST
// k_sig_events over the n records of R, on st (A.rows == nullptr: the count pass)
int launch_events(const sigk::SigRecs &R, const EvArgs &A, hipStream_t st);
// first[0 .. n] = the exclusive prefix of cnt[0 .. n) (first[n]: their sum), one workgroup, on st
int launch_scan(uint32_t n, const uint32_t *cnt, uint64_t *first, hipStream_t st);
#endif

}  // namespace evk

#ifndef S5_EVENT_WALK_HOST
// order_launch.hip: the counting sort of order_dev.h with the reads' n_eff as its key, so that the 64 reads of a wave end together.
// *ord = nullptr: no list (file order).  `hold` keeps the scratch the list lives in until the kernel that reads it is enqueued.
int s5kern_event_order(const sigk::SigRecs &R, hipStream_t st, const uint32_t **ord, std::unique_lock<std::mutex> &hold);
#endif
