// resident_rules.h — the host-side rules every decode-and-analyse call shares: which methods decode, where a batch lies in its chunk, how a
// record's guessed slots grow, and what happens to a batch with corrupt records.  Plain C++ over host arrays, no HIP:
// tests/test_resident_rules.py compiles it on its own and compares every rule with its arithmetic restated.
#pragma once
#include <stdint.h>

#include <vector>

#include "../../include/slow5gpu.h"
#include "dec_plan.h"

extern "C" void s5gpu_set_error(const char *fmt, ...);

namespace s5rules {

inline bool sig_method_ok(int sig_method) { return sig_method == S5GPU_SIG_NONE || sig_method == S5GPU_SIG_SVB_ZD || sig_method == S5GPU_SIG_EX_ZD; }
inline bool methods_ok(int rec_method, int sig_method) {
    return (rec_method == S5GPU_REC_NONE || rec_method == S5GPU_REC_ZLIB || rec_method == S5GPU_REC_ZSTD) && sig_method_ok(sig_method);
}

// the decoders that keep no payload (S5GPU_DEC_NO_PAYLOAD; the pairs are dec_plan.h's); every other pair is decoded in full
inline bool decodes_without_payload(int rec_method, int sig_method) { return s5plan::np_served(rec_method, sig_method); }

// Every item [pos[i], pos[i] + len[i]) lies inside the chunk, or S5GPU_ERR_ARG and a message that names who, the noun and i.  [*b0, *e1) is the
// part of the chunk the items span, b0 rounded down to 16 bytes (the alignment the decoders' loads want); n = 0: an empty span at 0.
// b0 = NULL: the check alone (the multi-device calls: the span is then taken share by share).
inline int chunk_span(const char *who, const char *noun, uint32_t n, size_t chunk_bytes, const uint64_t *pos, const uint32_t *len, uint64_t *b0,
                      uint64_t *e1) {
    uint64_t lo = n ? UINT64_MAX : 0, hi = 0;
    for (uint32_t i = 0; i < n; i++) {
        if (pos[i] > chunk_bytes || len[i] > chunk_bytes - pos[i]) { s5gpu_set_error("%s: %s %u lies outside the chunk", who, noun, i); return S5GPU_ERR_ARG; }
        lo = lo < pos[i] ? lo : pos[i];
        hi = hi > pos[i] + len[i] ? hi : pos[i] + len[i];
    }
    if (b0) { *b0 = lo & ~15ull; *e1 = hi; }
    return S5GPU_OK;
}

inline int host_records_ok(const char *who, uint32_t n, const void *const *rec, const size_t *len) {
    for (uint32_t i = 0; i < n; i++)
        if (!rec[i] && len[i]) { s5gpu_set_error("%s: record %u is NULL", who, i); return S5GPU_ERR_ARG; }
    return S5GPU_OK;
}

// ---- the slots a record is decoded into: guessed first, grown from what the decoder reports ----
constexpr uint32_t CAP_MAX = 0xFFFFFF00u;
constexpr int ATTEMPTS = 3;

inline uint32_t first_cap(uint64_t guess) { return (uint32_t)(guess > CAP_MAX ? CAP_MAX : guess); }

// A record whose payload outgrew pcap (status 5) reports in payload_len the size it needs — zlib, uncompressed records and zstd frames that
// state their content size — or 0, a zstd frame without one; never a size within pcap.  Without a size the slot grows eightfold.
inline uint32_t grown_cap(uint32_t pcap, uint32_t reported) { return reported > pcap ? reported : pcap < 0x10000000u ? 8 * pcap + 65536 : CAP_MAX; }

enum Grow { SETTLED, RETRY, BAD };
// one record after attempt `attempt` (0 ..): status 5 grows the payload slot (and the signal slot with it: a sample takes at least one payload
// byte in either signal format), status 6 takes the signal slot the record asked for, while attempts are left; any other failure is final
inline Grow grow_slots(const s5gpu_rec_fields_t &f, int attempt, uint32_t *pcap, uint32_t *scap) {
    if (f.status == 0) return SETTLED;
    if (attempt + 1 >= ATTEMPTS || (f.status != 5 && f.status != 6)) return BAD;
    if (f.status == 5) {
        *pcap = grown_cap(*pcap, f.payload_len);
        if (*scap < *pcap) *scap = *pcap;
    } else {
        *scap = f.n_samples;
    }
    return RETRY;
}
// ... and a batch: true when the batch is to be decoded again with the grown slots; *bad when a record failed for good (status[i], where
// given, then holds its status)
inline bool grow_batch(uint32_t n, const s5gpu_rec_fields_t *ff, int attempt, uint32_t *pcap, uint32_t *scap, int32_t *status, bool *bad) {
    bool retry = false;
    for (uint32_t i = 0; i < n; i++) {
        const Grow g = grow_slots(ff[i], attempt, &pcap[i], &scap[i]);
        retry |= g == RETRY;
        if (g == BAD) { *bad = true; if (status) status[i] = ff[i].status; }
    }
    return retry;
}

// ---- a batch with corrupt records ----
// The decoder redoes the records that outgrew their guessed slots (status 5 / 6) itself, but its retry stops at the first attempt that meets a
// corrupt record.  The other records' results must be valid all the same: while such records are left, the batch is decoded again without the
// corrupt ones, at most three more times.
// decode(m, idx) decodes the records idx[0, m) of the caller's batch and leaves their fields in ff[0, m); S5GPU_ERR_DATA from it is not an error
// here but sets *corrupt.  On return cur lists the records of the LAST decode, in order (what is resident in the context), ff holds their
// fields, and status[i] (n entries) the last status seen of every record of the batch, the dropped ones included.
template <class Decode>
int decode_dropping_corrupt(uint32_t n, Decode decode, std::vector<s5gpu_rec_fields_t> &ff, std::vector<uint32_t> &cur, int32_t *status, bool *corrupt) {
    enum { ROUNDS = 4 };
    cur.resize(n);
    for (uint32_t i = 0; i < n; i++) cur[i] = i;
    for (int round = 0;; round++) {
        const uint32_t m = (uint32_t)cur.size();
        if (m == 0) ff.clear();
        const int drc = m ? decode(m, cur.data()) : S5GPU_OK;
        if (drc && drc != S5GPU_ERR_DATA) return drc;
        *corrupt |= drc != 0;
        bool unfinished = false, droppable = false;
        for (uint32_t k = 0; k < m; k++) {
            status[cur[k]] = ff[k].status;
            unfinished |= ff[k].status == 5 || ff[k].status == 6;
            droppable |= ff[k].status != 0 && ff[k].status != 5 && ff[k].status != 6;
        }
        if (!drc || !unfinished || !droppable || round + 1 == ROUNDS) return S5GPU_OK;
        uint32_t w = 0;
        for (uint32_t k = 0; k < m; k++)
            if (ff[k].status == 0 || ff[k].status == 5 || ff[k].status == 6) cur[w++] = cur[k];
        cur.resize(w);
    }
}

}  // namespace s5rules
