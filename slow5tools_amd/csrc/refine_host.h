// refine_host.h — what the host sides of refine and of the whole-read chain (refine_api.hip, refine_long_api.hip, band_api.hip) share: the
// check of the refine parameters, and the rounds of s5gpu_extend_refine_dev over a group of consecutive reads (docs/codecs.md §4.24).
#pragma once
#include "band_host.h"
#include "refine_dev.h"

namespace refk {

int check_refine_params(const char *who, const s5gpu_refine_params_t *p);  // every parameter inside its range (§4.20), and not NULL

// The rounds over n consecutive reads of a ragged batch: first, qlen, rows_in and every [n] output point at the group's first read, the
// ragged arrays at row 0 of the batch.  row0: first[0] of the group, on the host (the band call counts the group's slots from it).
// scratch: bandk::scratch_bytes(slots, slot_words) bytes; work: refine_long_work(n, total_rows).bytes.
struct LongRounds {
    uint32_t n;
    const int16_t *queries;          // [total_rows]
    const uint64_t *first;           // [n + 1]
    const uint32_t *qlen;
    uint64_t total_rows;
    const int16_t *ref;
    uint32_t R;
    const s5gpu_ext_row_t *rows_in;
    const int32_t *lo_in, *hi_in;    // [total_rows]
    uint64_t row0;
    uint32_t T, band;
    s5gpu_refine_params_t P;
    void *scratch;
    uint64_t slots;
    uint32_t slot_words;
    void *work;
    int16_t *queries_out;            // [total_rows]
    s5gpu_ext_row_t *rows_out;
    int32_t *lo_out, *hi_out;        // [total_rows]
    s5gpu_fit_t *fit_out;
    uint32_t *rounds_out;
};
// queries_out = 0 and lo_out = hi_out = -1 over all total_rows rows: what the rows of no read, behind a query, or of a read without a
// result hold.  Once, before the rounds of a batch's groups.
int long_rounds_fill(int16_t *queries_out, int32_t *lo_out, int32_t *hi_out, uint64_t total_rows, hipStream_t st);
// Round 0 and P.iters rounds, queued on st; nothing is downloaded
int long_rounds(const LongRounds &X, hipStream_t st);

}  // namespace refk
