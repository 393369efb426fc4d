// contrast_kernels.hip — the level histograms (docs/codecs.md §4.23): their reset, the accumulate kernel, and the comparison of two of them,
// column by column.
//   k_pile_hist_reset : zeros and the head
//   k_pile_hist_accum : k_pileup_long_accum's walk (ragged_dev.h) over the same (ordered) segments and verdicts, which launch_pileup_long
//                       (pileup_kernels.hip) leaves in the work area, into R columns of 64 32-bit bins: a wave per segment at a time, lanes
//                       over rows, one add per cell.  The window is `cols` columns of 256 bytes in LDS (32-bit LDS adds), flushed word by word
//                       at the end; cells outside it are 32-bit global atomic adds.  Rules 2, 3, 5 and 6 of pileup_kernels.hip and 7 to 11 of
//                       ragged_dev.h hold as they stand; the bin is clamped below 64 (hist_bin) and masked where it indexes (hist_col_add);
//                       q0 and shift are read from the head the reset wrote, the shift clamped.
//   k_pile_contrast   : a wave per column at a time, a lane per bin: the two columns loaded (256 bytes each, coalesced), one wave scan for the
//                       prefix sums cA, cB, the 64-bit products cA nB and cB nA, and a wave reduction each for the largest difference (with
//                       its smallest bin), the overlap's sum and the two medians (a ballot).  Lane 0 writes the row as five 64-bit words.
// All integer: for nA, nB < 2^31 every product is below 2^62 and the sum of the overlap at most nA nB; above that S5GPU_CONTRAST_BIG is set
// instead.  In k_pile_contrast values read from memory form no address: a column is table[j] behind j < R, R an argument; the heads are
// compared on the device, and where they disagree (with each other or with R) no column is read at all.  No barrier there, vector stores
// only, no inline assembly.
#include <string.h>

#include "dev_common.h"
#include "pileup_dev.h"

extern "C" void s5gpu_set_error(const char *fmt, ...);

using namespace pilek;

__global__ __launch_bounds__(s5::NT) void k_pile_hist_reset(uint32_t *__restrict__ w, uint32_t R, int32_t q0, uint32_t shift) {
    const uint64_t words = HIST_HEAD_WORDS + (uint64_t)HIST_BINS * R;
    for (uint64_t k = (uint64_t)blockIdx.x * s5::NT + threadIdx.x; k < words; k += (uint64_t)gridDim.x * s5::NT) {
        uint32_t v = 0;                                                    // (s5gpu_pile_hist_head_t: the four counts are words 0 .. 7)
        if (k == 8) v = R;
        if (k == 9) v = (uint32_t)q0;
        if (k == 10) v = shift;
        if (k == 11) v = HIST_BINS;
        w[k] = v;
    }
}

__global__ void k_pile_hist_add_skipped(uint64_t *hist, uint32_t k) {
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(reinterpret_cast<unsigned long long *>(hist + 2), (unsigned long long)k);
}

namespace {
uint32_t g_hist_cols = HIST_MAX_COLS;   // option "pile_hist_cols"
uint32_t g_hist_grid = MAX_GRID;        // option "pile_hist_grid"

struct HistOps {
    static __device__ __forceinline__ void add32(uint32_t *p, uint32_t v) { atomicAdd(p, v); }
    static __device__ __forceinline__ void add32_win(uint32_t *p, uint32_t v) { atomicAdd(p, v); }   // (a pointer into LDS: a ds add)
};
}  // namespace

// per workgroup a slice of the (ordered) segments, a wave per segment at a time; cols: the window's columns, 0 or a power of two
__global__ __launch_bounds__(s5::NT) void k_pile_hist_accum(PileLongArgs A, uint32_t S, LongPtrs L, uint32_t sort, uint32_t cols, uint32_t *__restrict__ hist) {
    extern __shared__ __attribute__((aligned(16))) uint32_t hist_win[];    // cols columns of HIST_BINS words: all of the 64 KB at cols = 256
    const uint32_t lane = threadIdx.x & 63u;
    for (uint32_t t = threadIdx.x; t < cols * HIST_BINS; t += s5::NT) hist_win[t] = 0u;
    const GroupSlice G = group_slice(A, L, sort);
    Window W;
    const uint32_t l0 = cols ? group_anchor(A, S, L, G, 0u, s5::NW) : ANCHOR_NONE;
    W.lo = l0 == ANCHOR_NONE ? 0u : l0;
    W.cols = cols;
    const int32_t q0 = (int32_t)hist[9];                                   // s5gpu_pile_hist_head_t::q0, ::shift (32-bit words 9 and 10): written by the reset only
    const uint32_t shift = hist[10];
    uint32_t *table = hist + HIST_HEAD_WORDS;
    __syncthreads();
    uint64_t cells = 0;                                                    // this lane's
    walk_by_group(A, S, L, G, [&](const Seg &g) {
        const uint64_t f = A.first[g.k];                                   // (loaded beside the verdict: rule 7, k < n)
        if (L.verdict[g.k] != V_USED) return;                              // (the wave's branch)
        hist_seg_cells<HistOps>(g.r0, g.r1, lane, 64u, A.lo + f, A.hi + f, A.queries + f, q0, shift, A.R, W, hist_win, table, &cells);
    });
    __syncthreads();
    for (uint32_t t = threadIdx.x; t < cols * HIST_BINS; t += s5::NT) hist_flush_word<HistOps>(t, W, hist_win, table, A.R);
    const ReadCounts c = verdict_counts(L.verdict, A.n);
    head_add(reinterpret_cast<uint64_t *>(hist), {wave_sum(cells), c.used, c.skipped, c.bad});
}

namespace {

// the smallest lane whose flag is set (one is: lane 63's)
__device__ __forceinline__ uint32_t first_lane(bool flag) {
    const uint64_t m = __ballot(flag ? 1 : 0);
    return m ? (uint32_t)__ffsll((long long)m) - 1u : 0u;
}

}  // namespace

__global__ __launch_bounds__(s5::NT) void k_pile_contrast(const uint32_t *__restrict__ ha, const uint32_t *__restrict__ hb, const uint64_t *__restrict__ ta,
                                                         const uint64_t *__restrict__ tb, uint32_t R, uint64_t *__restrict__ out) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave = (uint64_t)blockIdx.x * s5::NW + (threadIdx.x >> 6), waves = (uint64_t)gridDim.x * s5::NW;
    // words 8 .. 11 of the heads: R, q0, shift, bins (every lane reads the same words: the branch is uniform)
    bool same = ha[8] == R && hb[8] == R && ha[9] == hb[9] && ha[10] == hb[10] && ha[11] == HIST_BINS && hb[11] == HIST_BINS;
    for (uint64_t j = wave; j < R; j += waves) {
        uint64_t *row = out + 5u * j;
        if (!same) {
            if (lane < 5u) row[lane] = lane == 4u ? (uint64_t)S5GPU_CONTRAST_HEADS << 48 : 0ull;
            continue;
        }
        const uint64_t a = ha[HIST_HEAD_WORDS + j * HIST_BINS + lane], b = hb[HIST_HEAD_WORDS + j * HIST_BINS + lane];
        const uint64_t ca = wave_incl_add64(a, lane), cb = wave_incl_add64(b, lane);
        const uint64_t na = __shfl(ca, 63), nb = __shfl(cb, 63);
        const bool big = na >= (1ull << 31) || nb >= (1ull << 31);
        uint32_t flags = (na == 0 ? S5GPU_CONTRAST_EMPTY_A : 0u) | (nb == 0 ? S5GPU_CONTRAST_EMPTY_B : 0u) | (big ? S5GPU_CONTRAST_BIG : 0u);
        uint64_t ks = 0, ov = 0;
        uint32_t ks_bin = 0;
        if (!big) {                                                        // (uniform)
            const uint64_t pa = ca * nb, pb = cb * na;                     // < 2^62
            uint64_t d = pa > pb ? pa - pb : pb - pa;
            uint32_t at = lane | (pa > pb ? 64u : 0u);                      // the bin, and above it whether A's prefix leads there
#pragma unroll
            for (int x = 32; x >= 1; x >>= 1) {                             // the maximum, at its smallest bin
                const uint64_t d2 = __shfl_xor(d, x);
                const uint32_t at2 = __shfl_xor(at, x);
                if (d2 > d || (d2 == d && (at2 & 63u) < (at & 63u))) { d = d2; at = at2; }
            }
            ks = d;
            ks_bin = at & 63u;
            if (at & 64u) flags |= S5GPU_CONTRAST_A_LOWER;
            const uint64_t ma = a * nb, mb = b * na;
            ov = wave_sum(ma < mb ? ma : mb);
        }
        const uint32_t med_a = first_lane(2u * ca >= na), med_b = first_lane(2u * cb >= nb);
        uint32_t depth_a = 0, depth_b = 0;
        if (ta && tb) {                                                    // word 0 of a column of the table: depth below, n_events above
            const uint64_t wa = ta[HEAD_WORDS + (uint64_t)COL_WORDS * j], wb = tb[HEAD_WORDS + (uint64_t)COL_WORDS * j];
            depth_a = (uint32_t)wa;
            depth_b = (uint32_t)wb;
            if ((wa >> 32) != na) flags |= S5GPU_CONTRAST_TABLE_A;
            if ((wb >> 32) != nb) flags |= S5GPU_CONTRAST_TABLE_B;
        }
        if (lane == 0) {
            const uint64_t n_a = na < 0xFFFFFFFFull ? na : 0xFFFFFFFFull, n_b = nb < 0xFFFFFFFFull ? nb : 0xFFFFFFFFull;
            row[0] = n_a | n_b << 32;
            row[1] = (uint64_t)depth_a | (uint64_t)depth_b << 32;
            row[2] = ks;
            row[3] = ov;
            row[4] = (uint64_t)ks_bin | (uint64_t)med_a << 16 | (uint64_t)med_b << 32 | (uint64_t)flags << 48;
        }
    }
}

int pilek::launch_hist_reset(void *hist, uint32_t R, int32_t q0, uint32_t shift, hipStream_t st) {
    const uint64_t words = HIST_HEAD_WORDS + (uint64_t)HIST_BINS * R, blocks = (words + s5::NT - 1) / s5::NT;
    hipLaunchKernelGGL(k_pile_hist_reset, dim3((uint32_t)(blocks < 4096 ? blocks : 4096)), dim3(s5::NT), 0, st, reinterpret_cast<uint32_t *>(hist), R, q0, shift);
    S5_LAUNCH_CHECK("k_pile_hist_reset");
    return S5GPU_OK;
}

int pilek::hist_set_option(const char *key, long value) {
    if (!key) return S5GPU_ERR_ARG;
    const bool pow2 = value > 0 && (value & (value - 1)) == 0;
    if (strcmp(key, "pile_hist_cols") == 0 && (value == 0 || (pow2 && value >= (long)HIST_MIN_COLS && value <= (long)HIST_MAX_COLS))) {
        g_hist_cols = (uint32_t)value;
        return S5GPU_OK;
    }
    if (strcmp(key, "pile_hist_grid") == 0 && value >= 1 && value <= (long)MAX_GRID) { g_hist_grid = (uint32_t)value; return S5GPU_OK; }
    return S5GPU_ERR_ARG;
}

int pilek::launch_hist_accum(const PileLongArgs &A, uint32_t S, const LongPtrs &L, uint32_t sort, void *hist, hipStream_t st) {
    const uint32_t cols = g_hist_cols;
    hipLaunchKernelGGL(k_pile_hist_accum, dim3(long_grid(A, S, g_hist_grid)), dim3(s5::NT), (size_t)cols * HIST_BINS * sizeof(uint32_t), st, A, S, L, sort, cols,
                       reinterpret_cast<uint32_t *>(hist));
    S5_LAUNCH_CHECK("k_pile_hist_accum");
    return S5GPU_OK;
}

int pilek::launch_hist_add_skipped(void *hist, uint32_t k, hipStream_t st) {
    if (k == 0) return S5GPU_OK;
    hipLaunchKernelGGL(k_pile_hist_add_skipped, dim3(1), dim3(64), 0, st, reinterpret_cast<uint64_t *>(hist), k);
    S5_LAUNCH_CHECK("k_pile_hist_add_skipped");
    return S5GPU_OK;
}

int pilek::launch_contrast(const void *hist_a, const void *hist_b, const void *acc_a, const void *acc_b, uint32_t R, s5gpu_pile_contrast_t *out, hipStream_t st) {
    const uint32_t quads = (R + 3u) / 4u;
    hipLaunchKernelGGL(k_pile_contrast, dim3(quads < MAX_GRID ? quads : MAX_GRID), dim3(s5::NT), 0, st, reinterpret_cast<const uint32_t *>(hist_a),
                       reinterpret_cast<const uint32_t *>(hist_b), reinterpret_cast<const uint64_t *>(acc_a), reinterpret_cast<const uint64_t *>(acc_b), R,
                       reinterpret_cast<uint64_t *>(out));
    S5_LAUNCH_CHECK("k_pile_contrast");
    return S5GPU_OK;
}
