// fold_kernels.hip — the fold of a table of pileup and of a level histogram onto classes (docs/codecs.md §4.26; fold_dev.h): the input's
// columns that share a class added into an output of K columns.  Every member is an integer sum, min or max, so the bytes do not depend on
// the launch shape, on "pile_fold_lds" or on the order of the adds.
//   k_pile_fold      : a thread takes a column at a time, grid-stride: cls[j] and the column's 48 bytes (three 16-byte loads), dropped and
//                      empty columns passed over, the rest merged into its class with col_merge (pileup_dev.h).  With lds != 0 (K <= 1024)
//                      the workgroup keeps the whole class table in LDS, the Window code with lo = 0, and adds its non-empty classes to the
//                      output at its end; else every merge is a global atomic.  cells and cost are reduced per wave, one atomic each a wave.
//   k_pile_hist_fold : a wave per column at a time, a lane per bin: one coalesced 256-byte load, one 32-bit global atomic add per
//                      non-zero bin of a kept column; the cells reduced per wave.
// Both read the two heads first (uniform loads): where fold_heads_ok (fold_hist_heads_ok) fails no column is read, nothing is added and
// S5GPU_FOLD_REFUSED is set in reserved[0] of the output's head.
// Values read from memory form addresses here (cls).  The rules, as in pileup_kernels.hip:
//   1. a class indexes the output (and the LDS table) only behind cls < K (fold_col, fold_bin); an input column is cols[j] behind j < R;
//   2. trip counts come from R and K, arguments both;
//   3. the only barriers are those around the LDS reset and the flush, reached by every thread: a refused call skips its loop, not them;
//   4. vector stores and HIP atomics only, no inline assembly.
#include <string.h>

#include "dev_common.h"
#include "fold_dev.h"

extern "C" void s5gpu_set_error(const char *fmt, ...);

using namespace pilek;

namespace {

uint32_t g_fold_lds = 1;            // option "pile_fold_lds"
uint32_t g_fold_grid = 512;         // option "pile_fold_grid"

struct FoldHistOps {
    static __device__ __forceinline__ void add32(uint32_t *p, uint32_t v) { atomicAdd(p, v); }
};

union ColLoad {
    uint4 v[3];
    s5gpu_pile_col_t c;
};

}  // namespace

// lds: 0, or K (<= FOLD_LDS_K) columns of 48 bytes of dynamic LDS
__global__ __launch_bounds__(s5::NT) void k_pile_fold(const uint64_t *__restrict__ in, uint32_t R, const uint32_t *__restrict__ cls, uint32_t K, uint64_t *out,
                                                     uint32_t lds) {
    extern __shared__ __attribute__((aligned(16))) uint64_t fold_win[];   // lds columns of COL_WORDS words
    for (uint32_t t = threadIdx.x; t < lds * COL_WORDS; t += s5::NT) fold_win[t] = t % COL_WORDS == 5 ? EMPTY_MINMAX : 0ull;
    // the heads: word 3 the cells, word 5 R below reserved[0] (every thread reads the same words: the branch is uniform)
    const bool go = fold_heads_ok(in[3], (uint32_t)in[5], R, (uint32_t)__hip_atomic_load(out + 5, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), K);
    __syncthreads();
    Window W;
    W.lo = 0u;
    W.cols = lds ? FOLD_LDS_K : 0u;
    s5gpu_pile_col_t *win = reinterpret_cast<s5gpu_pile_col_t *>(fold_win);
    s5gpu_pile_col_t *table = reinterpret_cast<s5gpu_pile_col_t *>(out + HEAD_WORDS);
    const uint4 *cols = reinterpret_cast<const uint4 *>(in + HEAD_WORDS);
    uint64_t cells = 0, cost = 0;                                          // this lane's
    if (go) {
        for (uint64_t j = (uint64_t)blockIdx.x * s5::NT + threadIdx.x; j < R; j += (uint64_t)gridDim.x * s5::NT) {
            const uint32_t c = cls[j];
            if (c >= K) continue;                                          // (dropped: its 48 bytes are not read)
            ColLoad L;
            L.v[0] = cols[3u * j];
            L.v[1] = cols[3u * j + 1u];
            L.v[2] = cols[3u * j + 2u];
            fold_col<DevOps>(L.c, c, K, W, win, table, &cells, &cost);       // (lds != 0: it is K, the slots fold_col allows)
        }
    }
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < lds && b < K; b += s5::NT) col_merge<DevOps>(table + b, win + b);
    const bool first = blockIdx.x == 0 && threadIdx.x < 64u;               // the input's reads, once
    head_add(out, {go && first ? in[0] : 0ull, go && first ? in[1] : 0ull, go && first ? in[2] : 0ull, wave_sum(cells), wave_sum(cost)});
    if (!go && blockIdx.x == 0 && threadIdx.x == 0) atomicOr(reinterpret_cast<uint32_t *>(out) + 11, S5GPU_FOLD_REFUSED);   // total.reserved[0]
}

__global__ __launch_bounds__(s5::NT) void k_pile_hist_fold(const uint32_t *__restrict__ in, uint32_t R, const uint32_t *__restrict__ cls, uint32_t K, uint32_t *out) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave = (uint64_t)blockIdx.x * s5::NW + (threadIdx.x >> 6), waves = (uint64_t)gridDim.x * s5::NW;
    const uint64_t *in64 = reinterpret_cast<const uint64_t *>(in);
    // the heads: 64-bit word 0 the cells, 32-bit word 8 R, 9 .. 11 q0, shift and bins (uniform)
    const bool go = fold_heads_ok(in64[0], in[8], R, out[8], K) && fold_hist_heads_ok(in, out);
    uint64_t cells = 0;                                                    // this lane's
    if (go) {
        for (uint64_t j = wave; j < R; j += waves) {
            const uint32_t c = cls[j];                                     // (the wave's)
            if (c >= K) continue;
            cells += fold_bin<FoldHistOps>(in[HIST_HEAD_WORDS + j * HIST_BINS + lane], c, K, lane, out + HIST_HEAD_WORDS);
        }
    }
    const bool first = blockIdx.x == 0 && threadIdx.x < 64u;
    head_add(reinterpret_cast<uint64_t *>(out), {wave_sum(cells), go && first ? in64[1] : 0ull, go && first ? in64[2] : 0ull, go && first ? in64[3] : 0ull});
    if (!go && blockIdx.x == 0 && threadIdx.x == 0) atomicOr(out + 12, S5GPU_FOLD_REFUSED);   // head.reserved[0], its low half
}

int pilek::fold_set_option(const char *key, long value) {
    if (!key) return S5GPU_ERR_ARG;
    if (strcmp(key, "pile_fold_lds") == 0 && (value == 0 || value == 1)) { g_fold_lds = (uint32_t)value; return S5GPU_OK; }
    if (strcmp(key, "pile_fold_grid") == 0 && value >= 1 && value <= (long)MAX_GRID) { g_fold_grid = (uint32_t)value; return S5GPU_OK; }
    return S5GPU_ERR_ARG;
}

int pilek::launch_fold(const void *acc_in, uint32_t R, const uint32_t *cls, uint32_t K, void *acc_out, hipStream_t st) {
    const uint32_t lds = g_fold_lds && K <= FOLD_LDS_K ? K : 0u;
    const uint32_t blocks = (R + s5::NT - 1u) / s5::NT;
    hipLaunchKernelGGL(k_pile_fold, dim3(blocks < g_fold_grid ? blocks : g_fold_grid), dim3(s5::NT), (size_t)lds * sizeof(s5gpu_pile_col_t), st,
                       reinterpret_cast<const uint64_t *>(acc_in), R, cls, K, reinterpret_cast<uint64_t *>(acc_out), lds);
    S5_LAUNCH_CHECK("k_pile_fold");
    return S5GPU_OK;
}

int pilek::launch_hist_fold(const void *hist_in, uint32_t R, const uint32_t *cls, uint32_t K, void *hist_out, hipStream_t st) {
    const uint32_t quads = (R + 3u) / 4u;
    hipLaunchKernelGGL(k_pile_hist_fold, dim3(quads < MAX_GRID ? quads : MAX_GRID), dim3(s5::NT), 0, st, reinterpret_cast<const uint32_t *>(hist_in), R, cls, K,
                       reinterpret_cast<uint32_t *>(hist_out));
    S5_LAUNCH_CHECK("k_pile_hist_fold");
    return S5GPU_OK;
}
