// band_kernels.hip — whole-read banded alignment in tiles from a known anchor, on the device (docs/codecs.md §4.21):
//   k_ev_query_long   : a lane per read, as k_ev_query: the quantised means of event rows [skip, skip + Q) at queries[first[i] ..), ragged.
//   k_sdtw_band<G>    : the hot path.  A wave per read, four reads a workgroup; the wave loops over its read's tiles of T = 64 G rows.  Within
//                       a tile it is k_sdtw_win's systolic scheme over the tile's window of W <= band columns (dirs_walk of dtw_dev.h: lane l
//                       owns G rows, DPP shifts, no predicate in a step, decision words in §4.17's [word][lane] layout, one slot a tile) with
//                       a Carry.  What differs: lane 0's "cell
//                       above" comes from the carried row, fetched 64 columns at a time and handed out by v_readlane as the reference values
//                       are; the lane that holds a full tile's last row stores that row, a word a step, for the next tile; at the tile's end
//                       the minimum, its smallest column and the next window are made scalar.  The carried row lives in LDS, band + 1 words a
//                       wave, updated in place: the storing lane (63) stores window column j at step j + 63, and the words a block fetch at
//                       step tb reads belong to columns >= tb of the OLD row, which no step before tb has stored (j <= tb - 64).  The last
//                       tile stores nothing.  LDS operations of one wave are ordered: no barrier.
//   k_sdtw_band_trace : a SEPARATE launch (the kernel boundary makes the words visible), a lane per read: bandk::band_walk.
// The rules, those of §4.17 / §4.20:
//   1. trip counts come from qlen, R, T and band only, checked before any loop: Q is qlen clamped to the read's rows and to 2^20, a tile has
//      W + last <= band + 63 steps, clamped to the slot;
//   2. no sample or cost forms an address: the windows' first columns come from columns (< R) clamped into [0, amax]; ref is read at
//      a + x for x < W only; the carried row at an index <= the width of the window before (<= band); a slot's index is checked against the
//      slots there are before the tile loop;
//   3. k_sdtw_band_trace does not trust what the pass before wrote (band_walk's bounds);
//   4. early returns are wave-uniform; a wave shares nothing but shifts, readlanes and its own LDS region;
//   5. vector stores and HIP builtins only.
#include <string.h>

#include "dev_common.h"
#include "band_dev.h"

extern "C" void s5gpu_set_error(const char *fmt, ...);

using namespace dtwk;
using namespace bandk;

// a read per lane: the quantiser is serial by definition (§4.16), and a negligible share of the work
__global__ __launch_bounds__(256) void k_ev_query_long(uint32_t n, LongQueryArgs A) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint64_t f0 = A.first[i], f1 = A.first[i + 1];
    const bool lies = f0 <= f1 && f1 <= A.total_rows;
    const uint64_t E = lies ? f1 - f0 : 0;
    uint32_t ql = long_qlen(E, A.skip, A.emin, A.emax);
    int32_t st = A.ev_status ? A.ev_status[i] : 0;
    if (st != 0) ql = 0;
    else if (ql == 0) st = S5GPU_STATUS_QUERY_SHORT;
    int16_t *q = A.queries + f0;
    if (ql) quant_row(&A.rows[f0 + A.skip].mean, sizeof(s5gpu_event_t) / sizeof(float), ql, A.scale, A.clip, q);
    for (uint64_t j = ql; j < E; j++) q[j] = 0;
    A.qlen[i] = ql;
    A.status[i] = st;
}

namespace {

// what a tile takes from the one before: S and how to read it (band_dev.h, carry_index / carry_value), as dirs_walk asks for it
struct Carry {
    uint32_t *S;                     // the wave's band + 1 words
    uint32_t delta, wprev, pmin;
    bool first;
    // the cell above this tile's window column x - 1 (x = 0: the diagonal of column 0)
    __device__ __forceinline__ uint32_t at(uint32_t x) const {
        bool in;
        const uint32_t i = carry_index(delta, x, wprev, &in);
        return carry_value(first ? 0u : S[i], in, pmin, first);
    }
    // the bottom cell of this tile's window column j, for the next tile
    __device__ __forceinline__ void store(uint32_t j, uint32_t cell) const { S[j + 1u] = cell; }
};

// kb -> the walk compiled for it.  The kernel's own dispatch, not with_kb of dtw_dev.h: with the Carry in a closure the compiler allocates
// 6 to 10 more VGPRs at G = 2, 4 and 8, and k_sdtw_band<4> measured 1.4 to 2.2 % slower on the device
template <int G, int KB = 0>
struct TileWalk {
    static __device__ __forceinline__ void run(int kb, Lane<G, false> &L, const int16_t *__restrict__ ref, uint32_t W, uint32_t nw, uint32_t *slot,
                                               uint32_t lane, const Carry &C, uint32_t wl) {
        if (kb == KB) dirs_walk<G, KB, true>(L, ref, W, nw, slot, lane, C, wl);
        else if constexpr (KB + 1 < G) TileWalk<G, KB + 1>::run(kb, L, ref, W, nw, slot, lane, C, wl);
    }
};

}  // namespace

template <int G>
__global__ __launch_bounds__(256) void k_sdtw_band(uint32_t n, BandArgs A) {
    extern __shared__ uint32_t lds[];
    constexpr uint32_t T = 64u * G;
    const uint32_t lane = threadIdx.x & 63u, wave = sgpr(threadIdx.x >> 6);
    const uint64_t read = wave_read(blockIdx.x, threadIdx.x);
    if (read >= n) return;                                                // (the wave's branch)
    const uint64_t f0 = A.first[read], f1 = A.first[read + 1];
    const bool lies = f0 <= f1 && f1 <= A.total_rows;
    const uint64_t E = lies ? f1 - f0 : 0;
    uint32_t Q = A.qlen[read];
    Q = Q < EMAX ? Q : EMAX;
    Q = sgpr((uint64_t)Q < E ? Q : (uint32_t)E);
    int32_t st = (int32_t)sgpr((uint32_t)A.status_in[read]);
    const int32_t anchor = (int32_t)sgpr((uint32_t)A.anchor[read * A.anchor_stride]);
    const uint32_t K = tiles_of(Q, T);
    const uint64_t slot0 = slot_first(f0 >= A.row0 ? f0 - A.row0 : 0, T, read);
    if (st == 0 && Q != 0 && (f0 < A.row0 || anchor < 0 || (uint32_t)anchor >= A.R || slot0 + K > A.slots)) st = S5GPU_STATUS_PATH_ROW;
    const bool path = st == 0 && Q != 0;
    int32_t *lo = A.lo + f0, *hi = A.hi + f0;
    for (uint64_t x = (path ? Q : 0u) + lane; x < E; x += 64u) { lo[x] = -1; hi[x] = -1; }
    if (!path) {                                                          // (wave-uniform)
        if (lane == 0) A.rows_out[read] = row_none(st);
        return;
    }
    Carry C;
    C.S = lds + wave * (A.band + 1u);
    C.delta = 0; C.wprev = 0; C.pmin = 0; C.first = true;
    if (lane == 0) C.S[0] = FAR;                                           // the column left of a window: no cell
    const int16_t *q = A.queries + f0;
    const uint32_t amax = win_amax(A.R, A.band);
    uint32_t a = win_place((uint32_t)anchor, A.band, 0u, amax);
    uint64_t base = 0;
    uint32_t end = 0;
    for (uint32_t k = 0; k < K; k++) {
        const uint32_t Qk = tile_rows_of(Q, T, k), W = win_cols(a, A.R, A.band);
        const uint32_t last = (Qk - 1u) / G;                               // the lane of the tile's last row: it does column W - 1 at step W - 1 + last
        const int kb = (int)(Qk - 1u - last * G);
        Lane<G, false> L;
        lane_init(L, false);
        if (lane == 0) L.dg = C.at(0u);                                    // the diagonal of column 0
#pragma unroll
        for (int kk = 0; kk < G; kk++) L.q[kk] = query_value(q, k * T + lane * G + kk, Q);
        const uint32_t nw = walk_words<G>(W, last, A.slot_words), wl = k + 1u < K ? 63u : 64u;   // a full tile's last row is lane 63's
        uint32_t *slot = A.scratch + (slot0 + k) * ((uint64_t)A.slot_words * 64u) + lane;
        if (lane == 0) A.tile_a[slot0 + k] = (int32_t)a;
        TileWalk<G>::run(kb, L, A.ref + a, W, nw, slot, lane, C, wl);
        const uint32_t mn = (uint32_t)__builtin_amdgcn_readlane((int)L.best, (int)last);
        const uint32_t m = (uint32_t)__builtin_amdgcn_readlane(L.best_end, (int)last);
        if (m >= W || mn >= FAR) {                                         // (cannot be: column m_k of the tile before carries 0 into this one)
            for (uint32_t x = lane; x < Q; x += 64u) { lo[x] = -1; hi[x] = -1; }
            if (lane == 0) A.rows_out[read] = row_none(S5GPU_STATUS_PATH_ROW);
            return;
        }
        base += mn;
        end = a + m;
        const uint32_t an = win_place(end, A.band, a, amax);
        C.delta = an - a; C.wprev = W; C.pmin = mn; C.first = false;
        if (k + 1u < K) a = an;
    }
    if (lane == 0) {
        s5gpu_ext_row_t r;
        r.cost = base; r.qlen = Q; r.tiles = K; r.start = -1; r.end = (int32_t)end; r.a_last = (int32_t)a; r.status = 0;
        A.rows_out[read] = r;
    }
}

__global__ __launch_bounds__(64) void k_sdtw_band_trace(uint32_t n, BandArgs A) {
    const uint64_t read = (uint64_t)blockIdx.x * 64u + threadIdx.x;
    if (read >= n) return;
    s5gpu_ext_row_t row = A.rows_out[read];
    if (row.status != 0 || row.qlen == 0) return;                          // (k_sdtw_band wrote the row and the -1s)
    const uint64_t f0 = A.first[read], f1 = A.first[read + 1];
    const bool lies = f0 <= f1 && f1 <= A.total_rows;
    const uint64_t E = lies ? f1 - f0 : 0;
    uint32_t Q = A.qlen[read];
    Q = Q < EMAX ? Q : EMAX;
    Q = (uint64_t)Q < E ? Q : (uint32_t)E;
    const uint64_t slot0 = slot_first(f0 >= A.row0 ? f0 - A.row0 : 0, A.T, read);
    int32_t *lo = A.lo + f0, *hi = A.hi + f0;
    int32_t rc = S5GPU_STATUS_PATH_ROW, start = -1;
    if (Q != 0 && row.qlen == Q && f0 >= A.row0 && slot0 + tiles_of(Q, A.T) <= A.slots)
        rc = band_walk(A.scratch + slot0 * ((uint64_t)A.slot_words * 64u), A.slot_words, A.tile_a + slot0, A.T / 64u, A.T, A.band, Q, A.R, row.end, lo, hi, &start);
    if (rc != 0) {
        for (uint32_t i = 0; i < Q; i++) { lo[i] = -1; hi[i] = -1; }
        A.rows_out[read] = row_none(rc);
        return;
    }
    row.start = start;
    A.rows_out[read] = row;
}

int bandk::launch_queries_long(uint32_t n, const LongQueryArgs &A, hipStream_t st) {
    if (n == 0) return S5GPU_OK;
    hipLaunchKernelGGL(k_ev_query_long, dim3((uint32_t)(((uint64_t)n + 255u) / 256u)), dim3(256), 0, st, n, A);
    S5_LAUNCH_CHECK("k_ev_query_long");
    return S5GPU_OK;
}

// the LDS of a workgroup: four waves of band + 1 words.  Above 64 KiB (band 4096) the kernel has to be told
template <int G>
static int launch_band_class(uint32_t n, const BandArgs &A, hipStream_t st) {
    const size_t lds = 4u * (size_t)(A.band + 1u) * sizeof(uint32_t);
    if (lds > 65536u) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_sdtw_band<G>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) {
            s5gpu_set_error("k_sdtw_band: %zu bytes of LDS refused: %s", lds, hipGetErrorString(e));
            return S5GPU_ERR_HIP;
        }
    }
    hipLaunchKernelGGL((k_sdtw_band<G>), dim3((uint32_t)(((uint64_t)n + 3u) / 4u)), dim3(256), lds, st, n, A);
    S5_LAUNCH_CHECK("k_sdtw_band");
    return S5GPU_OK;
}

static uint32_t g_band_passes = 3;                                         // option "sdtw_band_passes"

int bandk::set_option(const char *key, long value) {
    // which passes the band call launches: 1 k_sdtw_band only, 2 k_sdtw_band_trace only (over what an earlier call left in the scratch and
    // the rows), 3 both (the default).  For tools/extend_time.py: the passes are timed apart.
    if (key && strcmp(key, "sdtw_band_passes") == 0 && value >= 1 && value <= 3) { g_band_passes = (uint32_t)value; return S5GPU_OK; }
    return S5GPU_ERR_ARG;
}

int bandk::launch_band(uint32_t n, const BandArgs &A, hipStream_t st) {
    if (n == 0) return S5GPU_OK;
    int rc = S5GPU_OK;
    if (g_band_passes & 1u) switch (A.T) {
    case 64: rc = launch_band_class<1>(n, A, st); break;
    case 128: rc = launch_band_class<2>(n, A, st); break;
    case 256: rc = launch_band_class<4>(n, A, st); break;
    case 512: rc = launch_band_class<8>(n, A, st); break;
    case 1024: rc = launch_band_class<16>(n, A, st); break;
    }
    if (rc || !(g_band_passes & 2u)) return rc;
    hipLaunchKernelGGL(k_sdtw_band_trace, dim3((uint32_t)(((uint64_t)n + 63u) / 64u)), dim3(64), 0, st, n, A);
    S5_LAUNCH_CHECK("k_sdtw_band_trace");
    return S5GPU_OK;
}
