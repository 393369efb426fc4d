// skim_kernels.hip — k_skim_format: the lines of slow5tools skim (src/skim.c:271-335) from uncompressed records in HBM.
//
// One lane per record: every record of a file has the same fields in the same order (the header's), so the lanes of a wave walk the
// same role list and stay together; what differs — id length, digits, string lengths — is a few bytes.  Pass 1 measures each line,
// an exclusive scan of the lengths (the record-stream scan of batch_kernels.hip) places them back to back, pass 2 writes them there, gathered
// into aligned 8-byte stores.  The signal is never decoded: its sample count sits in the blob's first bytes (skim_dev.h).
#include "dev_common.h"
#include "skim_dev.h"

extern "C" void s5gpu_set_error(const char *fmt, ...);

namespace {

constexpr int SKIM_NT = 256;

__device__ __forceinline__ bool payload_of(const skim::SkimArgs &a, uint32_t i, const uint8_t **p, uint64_t *len, int32_t *st) {
    const s5gpu_rec_desc_t d = a.desc[i];
    if (!a.fields) { *p = a.pay + d.in_off; *len = d.in_len; return true; }
    const s5gpu_rec_fields_t &f = a.fields[i];
    if (f.status) { *st = f.status; return false; }
    if (f.payload_len > d.pay_cap) { *st = 5; return false; }
    *p = a.pay + d.pay_off;
    *len = f.payload_len;
    return true;
}

__global__ __launch_bounds__(SKIM_NT) void k_skim_format_measure(skim::SkimArgs a) {
    const uint32_t i = blockIdx.x * SKIM_NT + threadIdx.x;
    if (i >= a.n) return;
    const uint8_t *p;
    uint64_t len;
    int32_t st = 0;
    if (!payload_of(a, i, &p, &len, &st)) { a.status[i] = st; a.len[i] = 0; return; }
    skim::Sink o(nullptr);
    st = skim::skim_line(p, len, a.sig_method, a.plan, o);
    a.status[i] = st;
    a.len[i] = st == 0 && o.n <= 0xFFFFFFFFull ? (uint32_t)o.n : 0;
    if (st == 0 && o.n > 0xFFFFFFFFull) a.status[i] = 7;
}

__global__ __launch_bounds__(SKIM_NT) void k_skim_format_write(skim::SkimArgs a) {
    const uint32_t i = blockIdx.x * SKIM_NT + threadIdx.x;
    if (i >= a.n) return;
    const int32_t st = a.status[i];
    uint8_t *dst = a.out + a.off[i];
    if (st == skim::SKIM_HOST) {                 // the host printed this line: copy it into place
        uint32_t lo = 0, hi = a.n_host;
        while (lo < hi) { const uint32_t mid = (lo + hi) / 2; if (a.host_idx[mid] < i) lo = mid + 1; else hi = mid; }
        if (lo >= a.n_host || a.host_idx[lo] != i) return;
        const uint8_t *src = a.host_text + a.host_off[lo];
        skim::Sink o(dst);
        for (uint32_t j = 0, l = a.len[i]; j < l; j++) o.put(src[j]);
        o.flush();
        return;
    }
    if (st != 0) return;
    const uint8_t *p;
    uint64_t len;
    int32_t s2 = 0;
    if (!payload_of(a, i, &p, &len, &s2)) return;
    skim::Sink o(dst);
    skim::skim_line(p, len, a.sig_method, a.plan, o);
    o.flush();
}

__global__ void k_skim_patch_len(uint32_t *len, uint32_t n_host, const uint32_t *host_idx, const uint32_t *host_len) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n_host) len[host_idx[j]] = host_len[j];
}

}  // namespace

int s5_skim_measure(const skim::SkimArgs &a, hipStream_t st) {
    if (a.n == 0) return S5GPU_OK;
    hipLaunchKernelGGL(k_skim_format_measure, dim3((a.n + SKIM_NT - 1) / SKIM_NT), dim3(SKIM_NT), 0, st, a);
    S5_LAUNCH_CHECK("k_skim_format (measure)");
    return S5GPU_OK;
}
int s5_skim_write(const skim::SkimArgs &a, hipStream_t st) {
    if (a.n == 0) return S5GPU_OK;
    hipLaunchKernelGGL(k_skim_format_write, dim3((a.n + SKIM_NT - 1) / SKIM_NT), dim3(SKIM_NT), 0, st, a);
    S5_LAUNCH_CHECK("k_skim_format (write)");
    return S5GPU_OK;
}
int s5_skim_patch_len(uint32_t *len, uint32_t n_host, const uint32_t *host_idx, const uint32_t *host_len, hipStream_t st) {
    if (n_host == 0) return S5GPU_OK;
    hipLaunchKernelGGL(k_skim_patch_len, dim3((n_host + 255) / 256), dim3(256), 0, st, len, n_host, host_idx, host_len);
    S5_LAUNCH_CHECK("k_skim_patch_len");
    return S5GPU_OK;
}
