// order_launch.hip — the length-ordered launch lists of order_dev.h on the host side: the per-(device, stream) scratch they are built in, the
// one builder, and a named entry point per list.  The only unit that holds the sort's kernels (k_order_*).
#include <limits.h>

#include <vector>

#include "launch_common.h"
#include "dec_plan.h"
#include "order_dev.h"
#include "event_dev.h"

using namespace s5;

static uint32_t g_order_min = 8192;            // batches of at least this many records are launched longest first (option "order_min"; 0 = never)
// Scratch of the launch-order list: one buffer per (device, stream) — work on one stream is ordered, so the buffer of a stream is free again
// when the next call on that stream is enqueued — grown on demand, released by s5gpu_shutdown.  One pool and one lock PER DEVICE: the
// multi-device batch calls run one host thread per device, and those must not serialise on each other's list builds.  A buffer that is
// outgrown is retired, not freed (hipFree waits for the device — and an earlier launch on the stream may still read the old list): the
// retired ones are freed once an event recorded on their stream at that moment has completed (round 5; before: at shutdown), and a device keeps
// entries for at most ORD_MAX_STREAMS streams, the least recently used one making room.
struct OrderBuf {
    uint32_t *p = nullptr;
    size_t words = 0;
    hipStream_t st = nullptr;
    uint64_t used = 0;             // the pool's use counter when this stream last asked: the least recently used entry goes first
};
struct RetiredBuf {
    uint32_t *p;
    hipEvent_t ev;                 // recorded on the buffer's stream when it was outgrown: once it has completed nobody reads the buffer any more
};
constexpr int ORD_MAX_DEV = 64;
constexpr size_t ORD_MAX_STREAMS = 32;   // entries kept per device; a process that makes streams by the thousand does not keep a buffer for each
struct OrderPool {
    std::mutex mu;
    std::vector<OrderBuf> live;
    std::vector<RetiredBuf> retired;
    uint64_t tick = 0;
};
static OrderPool g_ord[ORD_MAX_DEV];
void s5kern_release_order() {                 // s5gpu_shutdown
    int cur = 0;
    const bool have_cur = hipGetDevice(&cur) == hipSuccess;
    for (int dev = 0; dev < ORD_MAX_DEV; dev++) {
        OrderPool &P = g_ord[dev];
        std::lock_guard<std::mutex> lk(P.mu);
        if (P.live.empty() && P.retired.empty()) continue;
        (void)hipSetDevice(dev);
        for (OrderBuf &b : P.live) if (b.p) (void)hipFree(b.p);
        for (RetiredBuf &q : P.retired) { (void)hipFree(q.p); if (q.ev) (void)hipEventDestroy(q.ev); }
        P.live.clear();
        P.retired.clear();
    }
    if (have_cur) (void)hipSetDevice(cur);
}
// the (device, stream)'s scratch with room for `need` words, and the pool's lock in `hold`
static int order_scratch(hipStream_t st, size_t need, uint32_t **out, std::unique_lock<std::mutex> &hold) {
    *out = nullptr;
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    if (dev < 0 || dev >= ORD_MAX_DEV) return S5GPU_OK;          // (file order is always correct)
    OrderPool &P = g_ord[dev];
    hold = std::unique_lock<std::mutex>(P.mu);
    // retired buffers whose last reader has finished go back to the device (round 5: they used to wait for s5gpu_shutdown)
    for (size_t i = 0; i < P.retired.size();) {
        if (!P.retired[i].ev || hipEventQuery(P.retired[i].ev) == hipSuccess) {
            if (P.retired[i].ev) { (void)hipFree(P.retired[i].p); (void)hipEventDestroy(P.retired[i].ev); P.retired[i] = P.retired.back(); P.retired.pop_back(); continue; }
        }
        i++;
    }
    OrderBuf *hit = nullptr;
    for (OrderBuf &b : P.live) if (b.st == st) { hit = &b; break; }
    if (!hit) {
        if (P.live.size() >= ORD_MAX_STREAMS) {
            // the stream not seen for the longest time gives up its entry.  Its handle may be gone (the caller destroyed it), so no event can be
            // recorded on it: hipFree waits for the device, which is correct whatever became of the stream — and rare (the 33rd stream)
            size_t lru = 0;
            for (size_t i = 1; i < P.live.size(); i++) if (P.live[i].used < P.live[lru].used) lru = i;
            if (P.live[lru].p) (void)hipFree(P.live[lru].p);
            P.live[lru] = P.live.back();
            P.live.pop_back();
        }
        P.live.emplace_back();
        hit = &P.live.back();
        hit->st = st;
    }
    hit->used = ++P.tick;
    if (hit->words < need) {
        const size_t w = need + need / 2;
        uint32_t *q = nullptr;
        if (hipMalloc((void **)&q, w * sizeof(uint32_t)) != hipSuccess) { hold.unlock(); s5gpu_set_error("no device memory for the launch-order list"); return S5GPU_ERR_NOMEM; }
        if (hit->p) {
            RetiredBuf r{hit->p, nullptr};
            if (hipEventCreateWithFlags(&r.ev, hipEventDisableTiming) != hipSuccess || hipEventRecord(r.ev, st) != hipSuccess) {
                if (r.ev) { (void)hipEventDestroy(r.ev); r.ev = nullptr; }      // no event: the buffer waits for s5gpu_shutdown, as before
            }
            P.retired.push_back(r);
        }
        hit->p = q;
        hit->words = w;
    }
    *out = hit->p;
    return S5GPU_OK;
}
// The one builder behind every length-ordered list (order_dev.h): the (device, stream)'s scratch, then the four kernels with `key` on `st`.
// *out = nullptr when no list is wanted (`list` = false) or none can be had (no scratch: file order is always correct).  `hold` keeps the
// device's pool locked until the caller has enqueued the kernels that read the list: two threads that share a stream (the default stream,
// say) must not interleave "build my list" / "build yours" / "read mine".
// `extra_words` more words of the same scratch (16-byte aligned, behind the list) come back in *extra — the zstd decoders' weights pass; they are
// handed out whether or not a list is built
template <class Key>
static int build_order(const Key &key, uint32_t n, bool list, uint32_t long_bucket, hipStream_t st, const uint32_t **out,
                       std::unique_lock<std::mutex> &hold, size_t extra_words = 0, uint32_t **extra = nullptr) {
    *out = nullptr;
    if (extra) *extra = nullptr;
    if (!list && !(extra && extra_words)) return S5GPU_OK;
    const size_t list_words = list ? (((size_t)ORD_LIST + n + 3) & ~(size_t)3) : 0;
    uint32_t *p = nullptr;
    { const int rc = order_scratch(st, list_words + (extra ? extra_words : 0), &p, hold); if (rc) return rc; }
    if (!p) return S5GPU_OK;
    if (list) {
        const uint32_t nb = (n + NT - 1) / NT;
        hipLaunchKernelGGL(k_order_zero, dim3(1), dim3(NT), 0, st, p);
        hipLaunchKernelGGL(k_order_count<Key>, dim3(nb), dim3(NT), 0, st, key, p);
        hipLaunchKernelGGL(k_order_scan, dim3(1), dim3(128), 0, st, p, long_bucket);
        hipLaunchKernelGGL(k_order_scatter<Key>, dim3(nb), dim3(NT), 0, st, key, p);
        *out = p;
    }
    if (extra && extra_words) *extra = p + list_words;
    return S5GPU_OK;
}
static const S5Option OPTIONS[] = {
    {"order_min", &g_order_min, 0, LONG_MAX, ~0u},         // big zlib batches: longest records first from this many records on (0: never)
};
int ordk::set_option(const char *key, long value) { return s5_set_option(OPTIONS, key, value); }
int ordk::warm() {                             // s5gpu_warmup: asking for a function of this file loads its code object
    hipFuncAttributes fa;
    HIP_TRY(hipFuncGetAttributes(&fa, reinterpret_cast<const void *>(k_order_zero)));
    return S5GPU_OK;
}

// the named lists (launch_common.h)
int s5kern_decode_order(const s5gpu_decode_args_t *a, hipStream_t st, const uint32_t **out, std::unique_lock<std::mutex> &hold,
                        size_t extra_words, uint32_t **extra, bool want_order) {
    const bool order = want_order && s5plan::from_count(a->n_recs, g_order_min);
    return build_order(OrderByInLen{a->desc, a->n_recs}, a->n_recs, order, 0, st, out, hold, extra_words, extra);
}
int s5kern_routed_order(const s5gpu_decode_args_t *a, hipStream_t st, const uint32_t **out, std::unique_lock<std::mutex> &hold) {
    return build_order(OrderByInLen{a->desc, a->n_recs}, a->n_recs, true, ROUTE_LONG_BUCKET, st, out, hold);
}
int s5kern_encode_order(const s5gpu_encode_args_t *a, hipStream_t st, const uint32_t **out, std::unique_lock<std::mutex> &hold) {
    const bool order = s5plan::from_count(a->n_reads, g_order_min);
    return build_order(OrderOvfBySamples{a->desc, a->ovf}, a->n_reads, order, 0, st, out, hold);
}
// ... the digest's: decoded records by canonical length (digest_kernels.hip); a batch of one wave's worth of records needs no order
int s5kern_digest_order(const digk::DigRecs &R, hipStream_t st, const uint32_t **out, std::unique_lock<std::mutex> &hold) {
    return build_order(OrderByCanonLen{R.desc, R.fields, R.n}, R.n, R.n > 16, 0, st, out, hold);
}
// ... the event detector's: decoded reads by n_eff (event_kernels.hip); a batch of one wave's worth of reads needs no order
int s5kern_event_order(const sigk::SigRecs &R, hipStream_t st, const uint32_t **out, std::unique_lock<std::mutex> &hold) {
    return build_order(OrderBySigLen{R}, R.n, R.n > 64, 0, st, out, hold);
}
