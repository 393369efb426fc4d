// dtw_path_kernels.hip — the whole path of each read's sDTW alignment, event to reference, on the device (docs/codecs.md §4.17):
//   k_sdtw_dirs  : per read, the recurrence of k_sdtw over the columns [start, end] of its row only, every cell's decision (2 bits) written
//                  to the read's slot of a scratch area
//   k_sdtw_trace : per read, the walk back through these decisions from (Q - 1, end) to (0, start): lo[i], hi[i] of every query row
//   k_ev_gather  : per read, the event rows of its query as a row of an [n, qmax] matrix (for the batch call: the tool prints their samples)
// k_sdtw_dirs is the scheme of k_sdtw (dtw_kernels.hip): a wave per read, lane l owning G rows, DPP shifts, FAR left of the window, no
// predicate in a step; it carries neither S nor a (cost, end) candidate.  Its steps are dirs_walk of dtw_dev.h, which the window and band
// kernels run too: a lane packs the 2 G bits of 16 / G steps into a word and stores it at [word][lane], a wave's store is 256 contiguous
// bytes.  It steps whole words: up to 16 / G - 1 steps behind column W - 1 + last, and like the rows at or beyond Q and the columns left of
// the window their codes are whatever falls out; nobody reads them.
// k_sdtw_trace is a SEPARATE launch on the same stream: the kernel boundary is what makes the words visible to its loads (a fence of
// workgroup scope would not).  A lane per read: the walk is one chain of dependent loads, and 64 chains a wave are what hides their latency.
// It is the one place in this code base where a value read from memory chooses the next address.  The rules:
//   1. trip counts come from qlen, the row and wmax only: Q <= 1024 (clamped to the pitch), W = end - start + 1 <= wmax <= 2^20, checked
//      by path_row_check in BOTH kernels before any loop (the trace does not trust what the dirs pass wrote); the walk has at most Q + W trips;
//   2. k_sdtw_dirs forms no address from a sample or a cost: it reads ref[start + x] for x < W only (end < R is checked) and writes the
//      words [0, min(words of its steps, slot_words)) of its own slot, row `read` of lo and hi, status[read];
//   3. k_sdtw_trace: i < Q and j < W are checked before each use, a word index is clamped to the slot, a code of 3 or a step out of the
//      window ends the walk with S5GPU_STATUS_PATH_ROW and the row is filled with -1 again (path_walk, dtw_dev.h); it writes lo[i], hi[i]
//      for i < Q of its read and, on failure, status[read];
//   4. a wave shares nothing but the shifts, which every lane executes (the early returns of k_sdtw_dirs are wave-uniform): no barrier, no
//      LDS; vector stores only, no inline assembly.
#include "dev_common.h"
#include "dtw_dev.h"

extern "C" void s5gpu_set_error(const char *fmt, ...);

using namespace dtwk;

template <int G>
__global__ __launch_bounds__(256) void k_sdtw_dirs(uint32_t n, PathArgs A) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t read = wave_read(blockIdx.x, threadIdx.x);
    if (read >= n) return;                                                // (the wave's branch: `read` is the same in its 64 lanes)
    const uint32_t Q = wave_rows(A.qlen[read], A.qpitch);
    if (other_launch<G>(Q)) return;
    uint32_t W = 0, start = 0;
    int32_t st = 0;
    if (Q) {
        const U4 row = A.rows[read];
        st = path_row_check(row, Q, A.R, A.wmax, &W);
        start = row.z;
    }
    st = (int32_t)sgpr((uint32_t)st);
    W = sgpr(W);
    start = sgpr(start);
    const bool path = Q != 0 && st == 0;
    int32_t *lo = A.lo + read * A.qpitch, *hi = A.hi + read * A.qpitch;
    for (uint32_t x = (path ? Q : 0u) + lane; x < A.qpitch; x += 64u) { lo[x] = -1; hi[x] = -1; }
    if (lane == 0) A.status[read] = st;
    if (!path) return;                                                    // (wave-uniform)
    Lane<G, false> L;
    lane_init(L, lane == 0);
    const int16_t *q = A.queries + read * A.qpitch;
#pragma unroll
    for (int k = 0; k < G; k++) L.q[k] = query_value(q, lane * G + k, Q);
    const uint32_t last = (Q - 1) / G;                                     // the lane of row Q - 1
    uint32_t *slot = A.scratch + read * ((uint64_t)A.slot_words * 64u) + lane;
    dirs_walk<G, 0, false>(L, A.ref + start, W, walk_words<G>(W, last, A.slot_words), slot, lane);   // (no candidate: KB is not used)
}

__global__ __launch_bounds__(64) void k_sdtw_trace(uint32_t n, PathArgs A) {
    const uint64_t read = (uint64_t)blockIdx.x * 64u + threadIdx.x;
    if (read >= n) return;
    const uint32_t Q = rows_of(A.qlen[read], A.qpitch);
    if (Q == 0) return;
    const U4 row = A.rows[read];
    uint32_t W;
    if (path_row_check(row, Q, A.R, A.wmax, &W) != 0) return;             // (k_sdtw_dirs wrote the status and the -1s)
    int32_t *lo = A.lo + read * A.qpitch, *hi = A.hi + read * A.qpitch;
    const int32_t rc = path_walk(A.scratch + read * ((uint64_t)A.slot_words * 64u), A.slot_words, lane_height(Q), Q, W, (int32_t)row.z, lo, hi);
    if (rc != 0) {
        for (uint32_t i = 0; i < Q; i++) { lo[i] = -1; hi[i] = -1; }
        A.status[read] = rc;
    }
}

// a wave per read, 16 bytes per lane and trip
__global__ __launch_bounds__(64) void k_ev_gather(uint32_t n, const U4 *__restrict__ rows, const uint64_t *__restrict__ first, const uint32_t *__restrict__ qlen,
                                                  uint32_t skip, uint32_t qmax, U4 *__restrict__ out) {
    const uint64_t read = blockIdx.x;
    if (read >= n) return;
    const uint32_t ql = qlen[read] < qmax ? qlen[read] : qmax;             // (k_ev_query made it: rows [first + skip, first + skip + ql) exist)
    const U4 *src = rows + first[read] + skip;
    U4 *dst = out + read * qmax;
    for (uint32_t x = threadIdx.x; x < qmax; x += 64u) {
        U4 v = result_row(0, 0, 0, 0);
        if (x < ql) v = src[x];
        dst[x] = v;
    }
}

// The dirs pass: a launch per lane height that a query of at most qpitch rows can need; then the trace.
int dtwk::launch_path(uint32_t n, const PathArgs &A, hipStream_t st, int which) {
    if (n == 0) return S5GPU_OK;
    int rc = S5GPU_OK;
    if (which & 1) rc = for_each_lane_height(A.qpitch, [&](auto g) -> int {
        hipLaunchKernelGGL((k_sdtw_dirs<decltype(g)::value>), wave_grid(n), dim3(256), 0, st, n, A);
        S5_LAUNCH_CHECK("k_sdtw_dirs");
        return S5GPU_OK;
    });
    if (!rc && (which & 2)) {
        hipLaunchKernelGGL(k_sdtw_trace, dim3((uint32_t)(((uint64_t)n + 63u) / 64u)), dim3(64), 0, st, n, A);
        S5_LAUNCH_CHECK("k_sdtw_trace");
    }
    return rc;
}

int dtwk::launch_event_gather(uint32_t n, const s5gpu_event_t *rows, const uint64_t *first, const uint32_t *qlen, uint32_t skip, uint32_t qmax,
                              s5gpu_event_t *out, hipStream_t st) {
    if (n == 0) return S5GPU_OK;
    hipLaunchKernelGGL(k_ev_gather, dim3(n), dim3(64), 0, st, n, reinterpret_cast<const U4 *>(rows), first, qlen, skip, qmax, reinterpret_cast<U4 *>(out));
    S5_LAUNCH_CHECK("k_ev_gather");
    return S5GPU_OK;
}
