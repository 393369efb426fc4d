// digest_kernels.hip — k_rec_digest: XXH64 (seed 0) of every decoded record's canonical form, where the decoder left it (docs/codecs.md §4.12).
//
// XXH64 is four serial multiply-rotate chains per stream, so the parallelism is across records: a quad of lanes owns a record, lane q of the
// quad the accumulator of the q-th 8-byte word of every 32-byte stripe; a wave owns sixteen records.  The merge of the four accumulators and
// the tail of fewer than 32 bytes run on the quad's first lane.  Records are taken longest canonical form first (order_dev.h), so the sixteen
// records of a wave end together and the longest read of a batch starts first.
//
// The canonical form is a virtual stream of four pieces (digest_dev.h).  A word that lies inside one piece is built from the two aligned
// 8-byte words around it and a funnel shift: the signal begins at virtual offset id_len + 46, so with most id lengths every lane word of the
// signal straddles dwords, and with an odd one samples.  Only the few words that cross a piece boundary are put together byte by byte.
// What bounds the loads:
//   1. digk::pieces_of refuses a record whose fields point outside its own payload or signal slot: nothing of it is read;
//   2. a word taken the aligned way lies inside one piece, so each of the two aligned words overlaps that piece, i.e. lies in the slot
//      rounded out to 16 bytes (the second one is not loaded when the word is aligned itself);
//   3. the byte path loads single bytes of a piece.
#include "dev_common.h"
#include "digest_dev.h"
#define S5_ORDER_LIST_ONLY
#include "order_dev.h"

extern "C" void s5gpu_set_error(const char *fmt, ...);

using namespace s5;

namespace {

constexpr uint64_t XP1 = 0x9E3779B185EBCA87ull, XP2 = 0xC2B2AE3D27D4EB4Full, XP3 = 0x165667B19E3779F9ull, XP4 = 0x85EBCA77C2B2AE63ull,
                   XP5 = 0x27D4EB2F165667C5ull;

__device__ __forceinline__ uint64_t rotl64(uint64_t x, int r) { return (x << r) | (x >> (64 - r)); }
__device__ __forceinline__ uint64_t xround(uint64_t acc, uint64_t in) { return rotl64(acc + in * XP2, 31) * XP1; }

// The 8 bytes at p (any alignment), little endian, from the aligned words around them: w = the aligned word that holds p[0], o = p's offset
// in it.  The second word is w[1] only when the bytes reach into it (o != 0), else w[0] again, and (hi << 1) << (63 - sh) shifts it out
// whole when sh = 0: no branch, and no load of a word that holds nothing of the bytes.
struct Aligned {
    const uint64_t *w;
    uint32_t sh, hi_at;
    __device__ __forceinline__ explicit Aligned(const uint8_t *p) {
        const uint32_t o = (uint32_t)((uintptr_t)p & 7u);
        w = reinterpret_cast<const uint64_t *>(p - o);
        sh = 8u * o;
        hi_at = o ? 1u : 0u;
    }
    // the bytes k aligned words further on
    __device__ __forceinline__ uint64_t at(uint64_t k) const {
        const uint64_t lo = w[k], hi = w[k + hi_at];
        return (lo >> sh) | ((hi << 1) << (63u - sh));
    }
};
__device__ __forceinline__ uint64_t word_at(const uint8_t *p) { return Aligned(p).at(0); }

// one record's stream: where its pieces lie in memory
struct Src {
    digk::Pieces P;
    const uint8_t *pay, *sig;       // the payload slot; the signal slot as bytes

    // byte v of the stream, v < P.total
    __device__ __forceinline__ uint32_t byte_at(uint64_t v) const {
        if (v < P.hl) return pay[v];
        if (v < P.sig_at) return (uint32_t)(P.n_samples >> (8u * (uint32_t)(v - P.hl))) & 0xFFu;
        if (v < P.aux_at) return sig[v - P.sig_at];
        return pay[P.aux_off + (v - P.aux_at)];
    }
    // the k <= 8 bytes from v on, little endian; v + k <= P.total
    __device__ __forceinline__ uint64_t bytes_at(uint64_t v, uint32_t k) const {
        uint64_t w = 0;
        for (uint32_t j = 0; j < k; j++) w |= (uint64_t)byte_at(v + j) << (8u * j);
        return w;
    }
    // the 8 bytes from v on; v + 8 <= P.total
    __device__ __forceinline__ uint64_t word(uint64_t v) const {
        if (v + 8 <= P.hl) return word_at(pay + v);
        if (v >= P.sig_at && v + 8 <= P.aux_at) return word_at(sig + (v - P.sig_at));
        if (v >= P.aux_at) return word_at(pay + P.aux_off + (v - P.aux_at));
        return bytes_at(v, 8);
    }
};

}  // namespace

__global__ __launch_bounds__(NT) void k_rec_digest(digk::DigRecs R, const uint32_t *__restrict__ ord, uint64_t *__restrict__ digest) {
    const uint32_t slot = blockIdx.x * (uint32_t)(NT / 4) + (threadIdx.x >> 2), q = threadIdx.x & 3u;
    const bool have = slot < R.n;
    uint32_t r = 0;
    Src S;
    S.P.ok = false; S.P.total = 0; S.P.hl = 0; S.P.aux_off = 0; S.P.n_samples = 0; S.P.sig_at = 0; S.P.aux_at = 0;
    S.pay = R.payload; S.sig = reinterpret_cast<const uint8_t *>(R.sig);
    if (have) {
        r = order_at(ord, slot);
        if (r < R.n) {                                                   // (a list entry is a record index by construction; checked all the same)
            const s5gpu_rec_desc_t d = R.desc[r];
            S.P = digk::pieces_of(d, R.fields[r]);
            S.pay = R.payload + d.pay_off;
            S.sig = reinterpret_cast<const uint8_t *>(R.sig + d.sig_off);
        }
    }
    const uint64_t total = S.P.ok ? S.P.total : 0ull, n_stripes = total >> 5;
    // stripes [s_lo, s_hi) lie in the signal with all their four words
    uint64_t s_lo = (S.P.sig_at + 31) >> 5, s_hi = S.P.aux_at >> 5;
    if (s_lo > n_stripes) s_lo = n_stripes;
    if (s_hi < s_lo) s_hi = s_lo;
    if (s_hi > n_stripes) s_hi = n_stripes;
    uint64_t v = q == 0 ? XP1 + XP2 : q == 1 ? XP2 : q == 2 ? 0ull : 0ull - XP1;
    for (uint64_t s = 0; s < s_lo; s++) v = xround(v, S.word(32 * s + 8 * q));
    {
        // the offset of a lane's words in their aligned words is the same in every stripe: it is taken apart once
        const Aligned A(S.sig + (32 * s_lo + 8 * q - S.P.sig_at));       // (not dereferenced when the range is empty)
        const uint64_t cnt = s_hi - s_lo;
#pragma unroll 4
        for (uint64_t k = 0; k < cnt; k++) v = xround(v, A.at(4 * k));
    }
    for (uint64_t s = s_hi; s < n_stripes; s++) v = xround(v, S.word(32 * s + 8 * q));
    // every lane of the wave is back here: the quad's accumulators go to its first lane
    const uint64_t v1 = __shfl(v, 0, 4), v2 = __shfl(v, 1, 4), v3 = __shfl(v, 2, 4), v4 = __shfl(v, 3, 4);
    if (q != 0 || !have || r >= R.n) return;
    if (!S.P.ok) { digest[r] = 0; return; }
    uint64_t h;
    if (total >= 32) {
        h = rotl64(v1, 1) + rotl64(v2, 7) + rotl64(v3, 12) + rotl64(v4, 18);
        h = (h ^ xround(0, v1)) * XP1 + XP4;
        h = (h ^ xround(0, v2)) * XP1 + XP4;
        h = (h ^ xround(0, v3)) * XP1 + XP4;
        h = (h ^ xround(0, v4)) * XP1 + XP4;
    } else h = XP5;
    h += total;
    uint64_t i = n_stripes << 5;
    for (; i + 8 <= total; i += 8) h = rotl64(h ^ xround(0, S.word(i)), 27) * XP1 + XP4;
    if (i + 4 <= total) { h = rotl64(h ^ (S.bytes_at(i, 4) * XP1), 23) * XP2 + XP3; i += 4; }
    for (; i < total; i++) h = rotl64(h ^ ((uint64_t)S.byte_at(i) * XP5), 11) * XP1;
    h ^= h >> 33; h *= XP2; h ^= h >> 29; h *= XP3; h ^= h >> 32;
    digest[r] = h;
}

int digk::launch_digest(const DigRecs &R, uint64_t *digest, hipStream_t st) {
    if (R.n == 0) return S5GPU_OK;
    std::unique_lock<std::mutex> hold;                                   // (the order scratch's: released when the kernel that reads the list is enqueued)
    const uint32_t *ord = nullptr;
    { const int rc = s5kern_digest_order(R, st, &ord, hold); if (rc) return rc; }
    const uint32_t per_wg = NT / 4;
    hipLaunchKernelGGL(k_rec_digest, dim3((R.n + per_wg - 1) / per_wg), dim3(NT), 0, st, R, ord, digest);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { s5gpu_set_error("k_rec_digest launch failed: %s", hipGetErrorString(e)); return S5GPU_ERR_HIP; }
    return S5GPU_OK;
}
