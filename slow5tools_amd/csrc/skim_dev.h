// skim_dev.h — one skim line (slow5tools skim, src/skim.c:271-311 process_read2) from one uncompressed BLOW5 record.
//
// The same code runs on the device (k_skim_format, skim_kernels.hip: one lane per record) and on the host (the few lines the device
// hands back, skim_api.hip).  The rules are docs/codecs.md §4.9:
//   read_id \t read_group \t digitisation \t offset \t range \t sampling_rate \t len_raw_signal \t . [\t aux]... \n
// doubles as "%f" with trailing zeros and a bare '.' trimmed (NaN: "."), len_raw_signal = the SAMPLE count, aux fields printed by
// the role the header's field name gives them (s5gpu_skim_layout_t).
//
// Doubles are printed exactly: round_half_even(|v| * 10^6) from the mantissa and exponent in 128-bit integer arithmetic — what glibc's
// "%f" prints.  A value of 2^107 (about 1.6e32) or more does not fit: the device gives its line up (status SKIM_HOST) and the host
// prints that line with snprintf.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/slow5gpu.h"

#define SKIM_HD __host__ __device__ __forceinline__

namespace skim {

constexpr int SKIM_HOST = -1;   // internal status: the line holds a double of 2^107 or more (the host prints it)

// where a line goes: counts only (p == nullptr), or writes at p.  Bytes are gathered into 8-byte words and stored aligned; the bytes in
// front of the first aligned word and behind the last one are stored one by one (a neighbour's line may share those words)
struct Sink {
    uint8_t *p;
    uint64_t n = 0;
    uint64_t acc = 0;
    uint32_t k = 0;
    SKIM_HD explicit Sink(uint8_t *dst) : p(dst) {}
    SKIM_HD void put(uint8_t c) {
        if (p) {
            uint8_t *d = p + n;
            if (k == 0 && ((uintptr_t)d & 7)) {
                *d = c;
            } else {
                acc |= (uint64_t)c << (8 * k);
                if (++k == 8) {
                    *reinterpret_cast<uint64_t *>(d - 7) = acc;
                    acc = 0;
                    k = 0;
                }
            }
        }
        n++;
    }
    SKIM_HD void flush() {
        if (!p) return;
        for (uint32_t j = 0; j < k; j++) p[n - k + j] = (uint8_t)(acc >> (8 * j));
        acc = 0;
        k = 0;
    }
};

template <class T>
SKIM_HD T ld(const uint8_t *p) {
    uint64_t v = 0;
#pragma unroll
    for (int i = 0; i < (int)sizeof(T); i++) v |= (uint64_t)p[i] << (8 * i);
    T t;
    if (sizeof(T) == 8) { memcpy(&t, &v, 8); }
    else { const uint32_t w = (uint32_t)v; memcpy(&t, &w, sizeof(T)); }
    return t;
}

SKIM_HD void put_u64(Sink &o, uint64_t v) {
    char d[20];
    int k = 0;
    do { d[k++] = (char)('0' + v % 10); v /= 10; } while (v);
    while (k) o.put((uint8_t)d[--k]);
}

// 128-bit unsigned as two 64-bit halves
struct U128 { uint64_t lo, hi; };
SKIM_HD U128 shl(U128 x, int s) {   // 0 <= s < 128
    if (s == 0) return x;
    if (s >= 64) return U128{0, x.lo << (s - 64)};
    return U128{x.lo << s, (x.hi << s) | (x.lo >> (64 - s))};
}
SKIM_HD U128 shr(U128 x, int s) {   // 0 <= s < 128
    if (s == 0) return x;
    if (s >= 64) return U128{x.hi >> (s - 64), 0};
    return U128{(x.lo >> s) | (x.hi << (64 - s)), x.hi >> s};
}
SKIM_HD bool lt(U128 a, U128 b) { return a.hi < b.hi || (a.hi == b.hi && a.lo < b.lo); }
SKIM_HD U128 sub(U128 a, U128 b) { return U128{a.lo - b.lo, a.hi - b.hi - (a.lo < b.lo ? 1u : 0u)}; }
SKIM_HD U128 add1(U128 a) { return U128{a.lo + 1, a.hi + (a.lo == UINT64_MAX ? 1u : 0u)}; }
// x /= d, returns x % d (d < 2^32): long division over four 32-bit limbs
SKIM_HD uint32_t divmod(U128 &x, uint32_t d) {
    uint32_t l[4] = {(uint32_t)(x.hi >> 32), (uint32_t)x.hi, (uint32_t)(x.lo >> 32), (uint32_t)x.lo};
    uint64_t r = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const uint64_t cur = (r << 32) | l[i];
        l[i] = (uint32_t)(cur / d);
        r = cur % d;
    }
    x.hi = ((uint64_t)l[0] << 32) | l[1];
    x.lo = ((uint64_t)l[2] << 32) | l[3];
    return (uint32_t)r;
}

// "%f" of v with trailing zeros and a bare '.' trimmed; NaN -> ".".  false: |v| >= 2^107, nothing written (the host prints it)
SKIM_HD bool put_f64_exact(Sink &o, double v) {
    uint64_t bits;
    memcpy(&bits, &v, 8);
    const bool neg = bits >> 63;
    const int be = (int)((bits >> 52) & 0x7FF);
    const uint64_t frac = bits & ((1ull << 52) - 1);
    if (be == 0x7FF) {
        if (frac) { o.put('.'); return true; }
        if (neg) o.put('-');
        o.put('i'); o.put('n'); o.put('f');
        return true;
    }
    const uint64_t m = be ? frac | (1ull << 52) : frac;
    const int e = be ? be - 1075 : -1074;          // |v| = m * 2^e
    if (e > 54) return false;                      // m * 10^6 * 2^e would not fit 128 bits
    // N = m * 10^6 (< 2^73)
    const uint64_t mh = m >> 32, ml = m & 0xFFFFFFFFull;
    const uint64_t a = ml * 1000000ull, b = mh * 1000000ull;   // a < 2^52, b < 2^41
    U128 N;
    N.lo = a + (b << 32);
    N.hi = (b >> 32) + (N.lo < a ? 1u : 0u);
    U128 R;
    if (e >= 0) {
        R = shl(N, e);
    } else {
        const int s = -e;
        if (s >= 75) {                              // N < 2^73 <= half: rounds to 0
            R = U128{0, 0};
        } else {
            R = shr(N, s);
            const U128 r = sub(N, shl(R, s));
            const U128 half = shl(U128{1, 0}, s - 1);
            if (lt(half, r) || (!lt(r, half) && (R.lo & 1))) R = add1(R);
        }
    }
    if (neg) o.put('-');
    uint32_t f;
    if (R.hi == 0) {
        put_u64(o, R.lo / 1000000ull);
        f = (uint32_t)(R.lo % 1000000ull);
    } else {
        f = divmod(R, 1000000u);
        uint32_t chunk[5];
        int k = 0;
        while (R.hi) chunk[k++] = divmod(R, 1000000000u);
        put_u64(o, R.lo);
        while (k) {                                  // 9 digits per chunk, zero-padded
            const uint32_t c = chunk[--k];
            uint32_t p = 100000000u;
            for (int j = 0; j < 9; j++) { o.put((uint8_t)('0' + (c / p) % 10)); p /= 10; }
        }
    }
    if (f) {
        o.put('.');
        uint32_t p = 100000u;
        while (f) { o.put((uint8_t)('0' + f / p)); f %= p; p /= 10; }
    }
    return true;
}

// a double the device cannot print: snprintf, as the ASCII path's fmt_f64 (host only)
SKIM_HD bool put_f64(Sink &o, double v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return put_f64_exact(o, v);
#else
    if (put_f64_exact(o, v)) return true;
    char tmp[352];
    int n = snprintf(tmp, sizeof tmp, "%f", v);
    if (n < 0) n = 0;
    if (memchr(tmp, '.', (size_t)n)) {
        while (n && tmp[n - 1] == '0') n--;
        if (n && tmp[n - 1] == '.') n--;
    }
    for (int i = 0; i < n; i++) o.put((uint8_t)tmp[i]);
    return true;
#endif
}

SKIM_HD uint32_t kind_bytes(int kind) {   // S5GPU_AUX_* element size (0: not a kind)
    return kind <= S5GPU_AUX_INT64 ? 1u << kind : kind <= S5GPU_AUX_UINT64 ? 1u << (kind - 4) : kind == S5GPU_AUX_FLOAT ? 4u
         : kind == S5GPU_AUX_DOUBLE ? 8u : kind <= S5GPU_AUX_ENUM ? 1u : 0u;
}

// One record's line.  0, 7 (malformed record), S5GPU_STATUS_BAD_ENUM, or SKIM_HOST (device only: a double too large to print here)
SKIM_HD int skim_line(const uint8_t *pay, uint64_t len, int sig_method, const s5gpu_skim_layout_t *L, Sink &o) {
    if (len < 2) return 7;
    const uint32_t idl = ld<uint16_t>(pay);
    if (len < 2ull + idl + 4 + 32 + 8) return 7;
    uint64_t q = 2;
    for (uint32_t j = 0; j < idl; j++) o.put(pay[q + j]);
    q += idl;
    o.put('\t'); put_u64(o, ld<uint32_t>(pay + q)); q += 4;
    for (int j = 0; j < 4; j++) {
        o.put('\t');
        if (!put_f64(o, ld<double>(pay + q))) return SKIM_HOST;
        q += 8;
    }
    const uint64_t sl = ld<uint64_t>(pay + q);
    q += 8;
    const uint64_t rem = len - q;
    uint64_t ns, blob;
    if (sig_method == S5GPU_SIG_SVB_ZD) {
        if (sl > rem || sl < 4) return 7;
        ns = ld<uint32_t>(pay + q); blob = sl;
    } else if (sig_method == S5GPU_SIG_EX_ZD) {
        if (sl > rem || sl < 9) return 7;
        ns = ld<uint64_t>(pay + q + 1); blob = sl;
    } else {
        if (sl > rem / 2) return 7;
        ns = sl; blob = 2 * sl;
    }
    q += blob;
    o.put('\t'); put_u64(o, ns);
    o.put('\t'); o.put('.');
    for (uint32_t a = 0; a < L->n_aux; a++) {
        const uint8_t t = L->type[a];
        const uint32_t es = kind_bytes(t & 0x0F);
        if (!es) return 7;
        o.put('\t');
        if (t & S5GPU_AUX_ARRAY) {
            if (len - q < 8) return 7;
            const uint64_t cnt = ld<uint64_t>(pay + q);
            q += 8;
            if (cnt > (len - q) / es) return 7;
            if (L->role[a] == S5GPU_SKIM_STRING && cnt) { for (uint64_t j = 0; j < cnt; j++) o.put(pay[q + j]); }
            else o.put('.');
            q += cnt * es;
            continue;
        }
        if (len - q < es) return 7;
        const uint8_t *p = pay + q;
        q += es;
        switch (L->role[a]) {
        case S5GPU_SKIM_DOUBLE: { const double v = ld<double>(p); if (!put_f64(o, v)) return SKIM_HOST; break; }
        case S5GPU_SKIM_FLOAT: { const float v = ld<float>(p); if (!put_f64(o, (double)v)) return SKIM_HOST; break; }
        case S5GPU_SKIM_INT32: {
            const int32_t v = ld<int32_t>(p);
            if (v == INT32_MAX) { o.put('.'); break; }
            if (v < 0) o.put('-');
            put_u64(o, v < 0 ? (uint64_t)(-(int64_t)v) : (uint64_t)v);
            break;
        }
        case S5GPU_SKIM_UINT8: { const uint8_t v = p[0]; if (v == UINT8_MAX) o.put('.'); else put_u64(o, v); break; }
        case S5GPU_SKIM_UINT32: { const uint32_t v = ld<uint32_t>(p); if (v == UINT32_MAX) o.put('.'); else put_u64(o, v); break; }
        case S5GPU_SKIM_UINT64: { const uint64_t v = ld<uint64_t>(p); if (v == UINT64_MAX) o.put('.'); else put_u64(o, v); break; }
        case S5GPU_SKIM_ENUM: {
            const uint8_t v = p[0];
            if (v == UINT8_MAX) { o.put('.'); break; }
            if (v >= L->n_labels[a]) return S5GPU_STATUS_BAD_ENUM;
            const uint32_t l = (uint32_t)L->label_first[a] + v;
            const uint32_t at = L->label_off[l], ll = L->label_len[l];
            for (uint32_t j = 0; j < ll; j++) o.put((uint8_t)L->text[at + j]);
            break;
        }
        default: o.put('.'); break;
        }
    }
    if (q != len) return 7;
    o.put('\n');
    return 0;
}

}  // namespace skim

// ---- k_skim_format (skim_kernels.hip): pass 1 measures every line, an exclusive scan of the lengths places them, pass 2 writes them ----
namespace skim {
struct SkimArgs {
    uint32_t n;
    int32_t sig_method;
    const s5gpu_rec_desc_t *desc;         // record i's payload: pay + desc[i].pay_off (inflated), or pay + desc[i].in_off (record press none)
    const s5gpu_rec_fields_t *fields;     // inflate results (status, payload_len); nullptr: record press none, the payload is desc[i].in_len bytes
    const uint8_t *pay;
    const s5gpu_skim_layout_t *plan;      // device copy of the layout
    uint32_t *len;                        // pass 1 out: line bytes (0 for a record that failed or went to the host)
    int32_t *status;                      // pass 1 out: 0, record status, or SKIM_HOST
    const uint64_t *off;                  // pass 2 in: line i at out + off[i]
    uint8_t *out;
    uint32_t n_host;                      // pass 2 in: lines the host printed, by ascending record index
    const uint32_t *host_idx;
    const uint64_t *host_off;             // line host_idx[j] at host_text + host_off[j], len[host_idx[j]] bytes
    const uint8_t *host_text;
};
}  // namespace skim
int s5_skim_measure(const skim::SkimArgs &a, hipStream_t st);
int s5_skim_write(const skim::SkimArgs &a, hipStream_t st);
// len[host_idx[j]] = host_len[j] for the n_host host-printed lines (before the scan)
int s5_skim_patch_len(uint32_t *len, uint32_t n_host, const uint32_t *host_idx, const uint32_t *host_len, hipStream_t st);
// off[i] = len[0] + ... + len[i-1], off[n] = the total (batch_kernels.hip: the scan of s5gpu_compact_dev); tmp: 8 * (n / 1024 + 2) bytes
int s5_scan_lengths(const uint32_t *len, uint32_t n, uint64_t *off, uint64_t *tmp, hipStream_t st);
