// sites_kernels.hip — per-read levels at chosen reference columns, and their scores against a control histogram (docs/codecs.md §4.25).
//   k_site_fill  : the M n empty entries {0, 0, 0xFFFFFFFF}, a 16-byte store each
//   k_site_cells : behind the plan and the check of pileup_kernels.hip (no sort: there is no window to keep warm; walk_by_wave of
//                  ragged_dev.h, a wave per segment, lanes over rows).  A segment's first lo and last hi, the same two words for every lane,
//                  give by two binary searches the sites [sa, sb) it can touch; a segment that touches none ends there.  Otherwise each lane
//                  searches its row's lo inside [sa, sb) and walks the sites up to its hi: per hit one 64-bit add, one 32-bit add and one
//                  32-bit min, global atomics (site_seg_cells of sites_dev.h).  The site list is read from global memory where it lies: at a
//                  typical M it is a cache line, and no barrier is needed.  The grid's threads also write verdict_out, a read each.
//   k_site_score : a wave per site at a time, a lane per bin: the control's column loaded (256 bytes, coalesced), one inclusive 64-bit wave
//                  scan; then the lanes stride over the reads k = lane, lane + 64, ... with a trip count that comes from n alone, and each
//                  takes the prefix sums at its bin and below it from the lanes that hold them (two shuffles with a per-lane source, executed
//                  by all 64 lanes).  Entries and rows are site-major: a wave reads and writes 1 KB runs.  No doubles.
// Rules 2, 3 and 6 of pileup_kernels.hip and 7 to 9 and 11 of ragged_dev.h hold as they stand: nothing of a read is touched unless its verdict
// is V_USED behind the check pass, so first[k] + i lies inside the ragged arrays for i < Q and every row's 0 <= lo <= hi < R.  A site index
// indexes the list and the matrix behind t < M (site_lower returns inside the range it is given); sites[t] indexes the histogram behind
// `< R`, R an argument; the head is compared on the device and where it disagrees no column is read.  Trip counts come from M, n, qlen and
// S.  No barrier, no LDS; vector stores and HIP atomics only, no inline assembly.
#include <string.h>

#include "dev_common.h"
#include "sites_dev.h"

extern "C" void s5gpu_set_error(const char *fmt, ...);

using namespace pilek;

namespace {
uint32_t g_site_passes = 7;             // option "site_passes"

struct SiteOps {
    static __device__ __forceinline__ void add64(uint64_t *p, uint64_t v) { atomicAdd(reinterpret_cast<unsigned long long *>(p), (unsigned long long)v); }
    static __device__ __forceinline__ void add32(uint32_t *p, uint32_t v) { atomicAdd(p, v); }
    static __device__ __forceinline__ void min32(uint32_t *p, uint32_t v) { atomicMin(p, v); }
};
}  // namespace

__global__ __launch_bounds__(s5::NT) void k_site_fill(uint4 *__restrict__ out, uint64_t entries) {
    const uint4 empty = make_uint4(0u, 0u, 0u, SITE_ROW_NONE);            // sum_q (two words), cells, row0
    for (uint64_t e = (uint64_t)blockIdx.x * s5::NT + threadIdx.x; e < entries; e += (uint64_t)gridDim.x * s5::NT) out[e] = empty;
}

__global__ __launch_bounds__(s5::NT) void k_site_cells(PileLongArgs A, uint32_t S, LongPtrs L, const uint32_t *__restrict__ sites, uint32_t M,
                                                       s5gpu_site_cell_t *out, uint32_t *__restrict__ verdict_out) {
    const uint32_t lane = threadIdx.x & 63u;
    walk_by_wave(A, S, L, [&](const Seg &g) {
        const uint64_t f = A.first[g.k];                                   // (loaded beside the verdict: rule 7, k < n)
        if (L.verdict[g.k] != V_USED) return;                              // (the wave's branch)
        site_seg_cells<SiteOps>(g.r0, g.r1, lane, 64u, A.lo + f, A.hi + f, A.queries + f, sites, M, g.k, A.n, out);
    });
    if (!verdict_out) return;
    for (uint64_t k = (uint64_t)blockIdx.x * s5::NT + threadIdx.x; k < A.n; k += (uint64_t)gridDim.x * s5::NT) {   // the reads, once each
        const uint32_t v = L.verdict[k];
        verdict_out[k] = (v & V_SKIPPED) ? 1u : (v & V_BAD) ? 2u : 0u;
    }
}

__global__ __launch_bounds__(s5::NT) void k_site_score(const s5gpu_site_cell_t *__restrict__ cells, uint32_t n, const uint32_t *__restrict__ sites, uint32_t M,
                                                       const uint32_t *__restrict__ hist, uint32_t R, s5gpu_site_score_t *__restrict__ out) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave = (uint64_t)blockIdx.x * s5::NW + (threadIdx.x >> 6), waves = (uint64_t)gridDim.x * s5::NW;
    const bool head = site_head_ok(hist, R);                               // (every lane reads the same words: the branches are uniform)
    const int32_t q0 = (int32_t)hist[9];                                   // s5gpu_pile_hist_head_t::q0, ::shift; hist_bin clamps the shift
    const uint32_t shift = hist[10];
    const uint32_t trips = (n + 63u) / 64u;
    for (uint64_t t = wave; t < M; t += waves) {
        const uint32_t s = sites[t];
        const bool col = s < R;
        const uint64_t c = head && col ? hist[HIST_HEAD_WORDS + (uint64_t)s * HIST_BINS + lane] : 0u;
        const uint64_t cum = wave_incl_add64(c, lane), total = __shfl(cum, 63);
        for (uint32_t trip = 0; trip < trips; trip++) {
            const uint64_t k = (uint64_t)trip * 64u + lane;
            s5gpu_site_cell_t e = {0, 0u, SITE_ROW_NONE};
            if (k < n) e = cells[t * n + k];
            int16_t level;
            const uint32_t b = site_level_bin(e, q0, shift, &level);      // < 64
            const uint64_t cum_b = __shfl(cum, (int)b), below_b = __shfl(cum, b ? (int)b - 1 : 0);
            if (k < n) out[t * n + k] = head ? site_score_row(e, level, cum_b, b ? below_b : 0u, total, col ? 0u : S5GPU_SITE_COLUMN) : site_score_head();
        }
    }
}

// which kernels s5gpu_site_cells_long_dev launches: 1 the fill, 2 the plan and the check, 4 k_site_cells, over what an earlier call left; 7
// all (the default).  For tools/sites_time.py: the passes are timed apart.
int pilek::site_set_option(const char *key, long value) {
    if (key && strcmp(key, "site_passes") == 0 && value >= 1 && value <= 7) { g_site_passes = (uint32_t)value; return S5GPU_OK; }
    return S5GPU_ERR_ARG;
}

int pilek::launch_site_cells(const PileLongArgs &A, const uint32_t *sites, uint32_t M, s5gpu_site_cell_t *out, uint32_t *verdict_out, hipStream_t st) {
    if (A.n == 0) return S5GPU_OK;
    const uint64_t entries = (uint64_t)M * A.n, blocks = (entries + s5::NT - 1) / s5::NT;
    int rc;
    if (g_site_passes & 1u) {
        hipLaunchKernelGGL(k_site_fill, dim3((uint32_t)(blocks < 4096 ? blocks : 4096)), dim3(s5::NT), 0, st, reinterpret_cast<uint4 *>(out), entries);
        S5_LAUNCH_CHECK("k_site_fill");
    }
    if ((g_site_passes & 2u) && (rc = launch_long_plan_check(A, st))) return rc;
    if (g_site_passes & 4u) {
        const uint32_t S = long_seg();
        hipLaunchKernelGGL(k_site_cells, dim3(long_grid(A, S)), dim3(s5::NT), 0, st, A, S, long_ptrs(A), sites, M, out, verdict_out);
        S5_LAUNCH_CHECK("k_site_cells");
    }
    return S5GPU_OK;
}

int pilek::launch_site_score(const s5gpu_site_cell_t *cells, uint32_t n, const uint32_t *sites, uint32_t M, const void *hist, uint32_t R, s5gpu_site_score_t *out,
                             hipStream_t st) {
    if (n == 0) return S5GPU_OK;
    const uint32_t quads = (M + 3u) / 4u;
    hipLaunchKernelGGL(k_site_score, dim3(quads < MAX_GRID ? quads : MAX_GRID), dim3(s5::NT), 0, st, cells, n, sites, M, reinterpret_cast<const uint32_t *>(hist), R, out);
    S5_LAUNCH_CHECK("k_site_score");
    return S5GPU_OK;
}
