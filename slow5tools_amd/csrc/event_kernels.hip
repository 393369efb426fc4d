// event_kernels.hip — scrappie-style event segmentation of decoded reads on the device (docs/codecs.md §4.15):
//   k_sig_events : per read, the events between the peaks of two sliding t-tests (windows w1 < w2), as 16-byte rows start | length | mean | stdv
//   k_ev_scan    : the exclusive prefix of the per-read counts between the count pass and the fill pass
// The peak detector is serial in the sample index and carries real-valued state, so a READ is a LANE's work: 64 reads of similar length (the
// counting sort of order_dev.h, keyed on n_eff) walk in lockstep, sample index i the same in every lane.  Each lane keeps the last 2 w2 + CH
// samples of its read in its own column of an LDS ring, ring[slot][lane]: the slot is the same in every lane, so the 64 lanes of a 2-byte
// access fall into 32 consecutive banks and never collide.  A lane refills its column CH = 32 samples (four 16-byte loads) at a time.  The
// four window sums and sums of squares slide in registers (integers, exact); the running sums over [0, i) are copied when a detector moves its
// candidate peak there, so that an event's sum and sum of squares are two subtractions when its closing peak is emitted.
// Nothing can index outside what it owns by construction (the rules of signal_kernels.hip):
//   1. the sample count of a record is SigRecs::n_eff, nothing else; the wave's trip count is the largest n_eff of its lanes plus w2;
//   2. every LDS index is slot * 64 + lane with a slot counter that wraps below `ring`: no sample, t value or count forms an address;
//   3. a row is stored only where its index is below the read's own ev_cap;
//   4. a workgroup is one wave and shares nothing between lanes: there is no barrier in k_sig_events; k_ev_scan's are reached by all threads.
#include "dev_common.h"
#include "event_dev.h"
#define S5_ORDER_LIST_ONLY
#include "order_dev.h"

extern "C" void s5gpu_set_error(const char *fmt, ...);

using namespace s5;

template <bool FILL>
__global__ __launch_bounds__(64) void k_sig_events(sigk::SigRecs R, evk::EvArgs A, const uint32_t *__restrict__ ord, uint32_t ring) {
    extern __shared__ int16_t ring_lds[];                          // ring * 64 samples
    const uint32_t lane = threadIdx.x, g = blockIdx.x * 64u + lane;
    uint32_t r = 0, n = 0;
    int32_t status = 0;
    bool have = false;
    if (g < R.n) {
        r = order_at(ord, g);
        if (r < R.n) { have = true; n = R.n_eff(r, &status); }     // (a list entry is a record index by construction; checked all the same)
    }
    const int16_t *p = R.sig;
    bool vec = false;
    evk::RowOut O = {nullptr, 0, false, 0.0, 1.0};
    if (n) {
        const uint64_t o = R.o(r);
        p = R.sig + o;
        vec = (o & 7u) == 0;                                       // (R.sig itself is 16-byte aligned: checked by the host)
        if (FILL) {
            O.cap = A.ev_cap[r];
            O.row0 = reinterpret_cast<evk::U4 *>(A.rows) + A.ev_off[r];
            if (A.mode == S5GPU_NORM_PA) { O.pa = true; O.offset = R.fields[r].offset; O.scale = R.fields[r].range / R.fields[r].digitisation; }
        }
    }
    uint32_t nmax = n;                                             // every lane is here: the wave walks to its longest read's end
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) nmax = max(nmax, (uint32_t)__shfl_xor((int)nmax, d));
    const uint32_t cnt = evk::walk<FILL>(p, n, nmax, vec, ring_lds + lane, 64u, ring, A, O);
    if (have) {
        A.n_events[r] = cnt;
        A.ev_status[r] = status ? status : (FILL && cnt > O.cap ? (int32_t)S5GPU_STATUS_EVENTS_OVERFLOW : 0);
    }
}

// one workgroup: first[i] = cnt[0] + ... + cnt[i - 1], first[n] = the total
__global__ __launch_bounds__(NT) void k_ev_scan(uint32_t n, const uint32_t *__restrict__ cnt, uint64_t *__restrict__ first) {
    __shared__ unsigned long long wtot[NW];
    unsigned long long carry = 0;
    for (uint32_t base = 0; base < n; base += NT) {                // (n is the same for every thread)
        const uint32_t i = base + threadIdx.x;
        const unsigned long long c = i < n ? cnt[i] : 0u;
        unsigned long long v = c;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned long long t = __shfl_up(v, d);
            if (lane_id() >= d) v += t;
        }
        if (lane_id() == 63) wtot[wave_id()] = v;
        __syncthreads();
        unsigned long long pre = carry, tot = 0;
#pragma unroll
        for (int w = 0; w < NW; w++) { if (w < wave_id()) pre += wtot[w]; tot += wtot[w]; }
        if (i < n) first[i] = pre + v - c;
        carry += tot;
        __syncthreads();
    }
    if (threadIdx.x == 0) first[n] = carry;
}

int evk::launch_events(const sigk::SigRecs &R, const EvArgs &A, hipStream_t st) {
    if (R.n == 0) return S5GPU_OK;
    std::unique_lock<std::mutex> hold;                                   // (the order scratch's: released when the kernel that reads the list is enqueued)
    const uint32_t *ord = nullptr;
    { const int rc = s5kern_event_order(R, st, &ord, hold); if (rc) return rc; }
    const uint32_t ring = ring_slots(A.w2);
    const dim3 grid((uint32_t)(((uint64_t)R.n + 63u) / 64u)), block(64);
    const size_t lds = (size_t)ring * 64 * sizeof(int16_t);              // 8 KB for w2 <= 16, 20 KB for w2 = 64
    if (A.rows) hipLaunchKernelGGL(k_sig_events<true>, grid, block, lds, st, R, A, ord, ring);
    else hipLaunchKernelGGL(k_sig_events<false>, grid, block, lds, st, R, A, ord, ring);
    S5_LAUNCH_CHECK("k_sig_events");
    return S5GPU_OK;
}

int evk::launch_scan(uint32_t n, const uint32_t *cnt, uint64_t *first, hipStream_t st) {
    hipLaunchKernelGGL(k_ev_scan, dim3(1), dim3(NT), 0, st, n, cnt, first);
    S5_LAUNCH_CHECK("k_ev_scan");
    return S5GPU_OK;
}
