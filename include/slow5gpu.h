/*
 * slow5gpu.h — C ABI of the MI355X-native BLOW5 record press path (libslow5gpu.so).
 *
 * Plain C, plain pointers and sizes.  This is the drop-in boundary for the one data-parallel hot
 * path of slow5tools: the per-record worker that `work_db` fans out over pthreads
 *     /root/reference/src/view.c:35-57   depress_parse_rec_to_mem
 *     /root/reference/src/merge.c:43-70  parallel_reads_model
 *     /root/reference/src/get.c:37-66    work_per_single_read_get
 * i.e. slow5_rec_to_mem() = svb-zd(raw_signal) -> pack -> zlib, and its inverse
 * slow5_rec_depress_parse().  A whole batch (db_t, /root/reference/src/thread.h:50-66) is handed
 * over in one call; results come back in the same per-record slots so the ordered fwrite loops
 * (/root/reference/src/view.c:296-299) stay untouched.  See INTEGRATION.md for the patch.
 *
 * Two levels:
 *   s5gpu_*_dev   : device-resident buffers + a HIP stream (what bench.py times; kernels only)
 *   s5gpu_*_batch : host buffers in, malloc'd host buffers out (what slow5tools would call)
 * The slow5lib-compatible per-record API (slow5_press_*, slow5_rec_to_mem, ...) is declared in
 * slow5_compat.h and implemented on top of the batch calls.
 */
#ifndef SLOW5GPU_H
#define SLOW5GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* on-disk method codes, identical to slow5lib's enum slow5_press_method values used by
 * /root/reference/src/misc.c:253-263 (SLOW5_COMPRESS_NONE/ZLIB, SLOW5_COMPRESS_NONE/SVB_ZD) */
enum { S5GPU_REC_NONE = 0, S5GPU_REC_ZLIB = 1, S5GPU_REC_ZSTD = 2 };   /* zstd: any frame libzstd writes is decoded (an optional content
                                                                         * checksum is verified: status 4 on a mismatch); encoded frames are literals-only
                                                                         *  */
enum { S5GPU_SIG_NONE = 0, S5GPU_SIG_SVB_ZD = 1, S5GPU_SIG_EX_ZD = 2 };

enum {
    S5GPU_OK = 0,
    S5GPU_ERR_ARG = -1,       /* bad argument / unsupported method        */
    S5GPU_ERR_HIP = -2,       /* HIP runtime error (s5gpu_last_error())   */
    S5GPU_ERR_NOMEM = -3,
    S5GPU_ERR_NODEV = -4,     /* no gfx950 device: the library never falls back to a CPU path */
    S5GPU_ERR_DATA = -5       /* corrupt record (per-record status says which) */
};

/* One read of an encode batch.  All offsets index the batch-wide device buffers. */
typedef struct s5gpu_read_desc {
    uint64_t sig_off;    /* first sample of the read in `sig` (sample index, multiple of 8)          */
    uint64_t hdr_off;    /* byte offset in `hdr` of the record bytes that precede the u64 length:    */
                         /*   u16 read_id_len | read_id | u32 read_group | 4 x f64                   */
    uint64_t aux_off;    /* byte offset in `aux` of the already-serialised aux fields                */
    uint64_t out_off;    /* byte offset of this read's slot in `slots` (multiple of 16)              */
    uint32_t n_samples;  /* len_raw_signal                                                          */
    uint32_t hdr_len;    /* 2 + read_id_len + 4 + 32                                                 */
    uint32_t aux_len;
    uint32_t slot_cap;   /* bytes available at out_off, >= s5gpu_slot_bound()                        */
} s5gpu_read_desc_t;

/* Worst-case bytes one encoded record can occupy in its slot (incl. the u64 size prefix). */
uint64_t s5gpu_slot_bound(uint32_t n_samples, uint32_t hdr_len, uint32_t aux_len, int rec_method, int sig_method);
/* Uncompressed payload upper bound (what `max_payload` below must cover). */
uint64_t s5gpu_payload_bound(uint32_t n_samples, uint32_t hdr_len, uint32_t aux_len, int sig_method);

typedef struct s5gpu_encode_args {
    uint32_t n_reads;
    int32_t rec_method, sig_method;
    const s5gpu_read_desc_t *desc;   /* device, n_reads entries                                      */
    const int16_t *sig;              /* device, raw_signal of all reads                              */
    const uint8_t *hdr;              /* device                                                       */
    const uint8_t *aux;              /* device (may be NULL when every aux_len == 0)                 */
    uint8_t *slots;                  /* device, out: [u64 size][record bytes] per read at out_off    */
    uint32_t *out_len;               /* device, out: bytes written per read, incl. the 8-byte prefix */
    uint32_t max_payload;            /* max over reads of s5gpu_payload_bound()                      */
    uint32_t lds_payload_cap;        /* 0 = auto.  LDS bytes the one-workgroup-per-read kernel keeps */
                                     /*   for a payload; reads that need more (long or incompressible*/
                                     /*   signals) are re-run through the HBM-staged kernels.  With 0 and */
                                     /*   a longest read far over the budget the whole batch is staged;   */
                                     /*   name a budget (8192 is a good one) for batches that mix short   */
                                     /*   and long reads: the host batch calls do so from the lengths     */
    uint32_t *ovf;                   /* device, n_reads + 1 words of scratch (list of such reads)    */
} s5gpu_encode_args_t;

/* One record of a decode batch. */
typedef struct s5gpu_rec_desc {
    uint64_t in_off;     /* byte offset in `in` of the record bytes (without the u64 size prefix)    */
    uint64_t pay_off;    /* byte offset of this record's payload slot in `payload` (multiple of 16)  */
    uint64_t sig_off;    /* sample offset of this record's output in `sig_out` (multiple of 8)       */
    uint32_t in_len;
    uint32_t pay_cap;    /* bytes available at pay_off                                               */
    uint32_t sig_cap;    /* samples available at sig_off                                             */
    uint32_t reserved;
} s5gpu_rec_desc_t;

/* Parsed primary fields of one decoded record (slow5_rec_t minus the pointers). */
typedef struct s5gpu_rec_fields {
    int32_t status;        /* 0 ok; 1 bad zlib header; 2 corrupt data; 3 truncated; 4 adler mismatch;  */
                           /* 5 payload slot too small (payload_len = needed); 6 signal slot too small */
                           /* (n_samples = needed); 7 malformed record                                 */
    uint32_t payload_len;  /* uncompressed record length                                               */
    uint32_t n_samples;
    uint32_t read_id_len;  /* read_id sits at payload + 2                                              */
    uint32_t read_group;
    uint32_t aux_off;      /* offset of the aux bytes within the payload                               */
    uint32_t aux_len;
    uint32_t reserved;
    double digitisation, offset, range, sampling_rate;
} s5gpu_rec_fields_t;

/* s5gpu_decode_args.flags */
enum {
    /* s5gpu_decode_dev, zlib or zstd records with svb-zd signals and zlib records with ex-zd signals: the caller wants fields + signals only (what `get` and the
     * decode half of a signal consumer need; read_id / aux bytes live in the uncompressed record and are NOT kept).  `payload` is then
     * SCRATCH of payload_bytes bytes (s5gpu_decode_scratch_bytes() says how much is useful): the kernel runs as persistent
     * workgroups, each with one scratch slot of max_pay_cap bytes that it reuses record after record, so an uncompressed record
     * needs no slot of its own (n x pay_cap bytes saved; the HBM traffic is that of the full form: DESIGN.md 4.8).  desc[i].pay_off / pay_cap are ignored; a record whose payload
     * exceeds max_pay_cap reports status 5 with the size needed.  fields[i].aux_off / aux_len are still reported. */
    S5GPU_DEC_NO_PAYLOAD = 1
};

typedef struct s5gpu_decode_args {
    uint32_t n_recs;
    int32_t rec_method, sig_method;
    uint32_t flags;                  /* 0, or S5GPU_DEC_* (this word was padding before: zeroed structs keep their meaning)  */
    const s5gpu_rec_desc_t *desc;    /* device                                                       */
    const uint8_t *in;               /* device, compressed records; 16 readable bytes must follow the */
                                     /*   last record (the inflate kernels fetch aligned dwords ahead) */
    uint8_t *payload;                /* device, out: uncompressed record per slot (scratch with S5GPU_DEC_NO_PAYLOAD) */
    int16_t *sig_out;                /* device, out: raw_signal per record                           */
    s5gpu_rec_fields_t *fields;      /* device, out                                                  */
    uint64_t payload_bytes;          /* S5GPU_DEC_NO_PAYLOAD: bytes of scratch at `payload`          */
    uint32_t max_pay_cap;            /* largest uncompressed record to expect (0 = not known).  S5GPU_DEC_NO_PAYLOAD: the scratch slot
                                      * size.  Any form: a batch of short records (<= 32 KiB of slot, i.e. reads of up to ~10 k samples) with
                                      * svb-zd / ex-zd signals runs the inflate kernel in its 24-waves-per-CU shape (a 256-entry list
                                      * of waiting matches); longer or unknown ones in the 21-wave shape with 768 entries, which long
                                      * reads written by stock zlib need in their key bytes */
    uint32_t max_in_len;             /* largest COMPRESSED record of the batch, bytes (0 = not known; this word was `reserved`: zeroed structs keep
                                      * their meaning).  S5GPU_DEC_NO_PAYLOAD on zlib + svb-zd records: when every record fits one 4 KiB window
                                      * of the inflate (max_in_len <= 4000: reads of up to ~4500 samples) the uncompressed record is kept in
                                      * LDS and never reaches HBM (round 6: k_inflate_par_np_lp; a record whose payload outgrows the 5.3 KiB
                                      * of LDS after all is redone by the slot decoder).  A hint: any value is safe */
} s5gpu_decode_args_t;
/* scratch worth bringing for S5GPU_DEC_NO_PAYLOAD (one slot per workgroup the device can hold + the fallback decoder's);
 * anything from 64 + 2 * (max_pay_cap + 32) bytes up works, less only means fewer workgroups */
uint64_t s5gpu_decode_scratch_bytes(uint32_t max_pay_cap);

/* ---- lifetime ---- */
int s5gpu_init(int device);              /* select device; S5GPU_ERR_NODEV if it is not a gfx950 GPU */
/* Several GPUs of one node behind the host-buffer batch calls: bit d of dev_mask = HIP device d.  A host batch is
 * then cut into one contiguous index range per device — device g of G takes records [g*n/G, (g+1)*n/G), exactly how work_db
 * cuts a batch per thread (/root/reference/src/thread.c:76-90) — each range goes through its own pinned H2D -> kernels -> D2H on
 * its device's stream, concurrently, and every result lands in the caller's out[i]: the ordered write loop
 * (/root/reference/src/view.c:296-299) does not change.  No collective, no peer traffic.  The *_dev entry points are not
 * affected: their caller picks the device (hipSetDevice) and passes buffers of that device. */
int s5gpu_init_mask(uint64_t dev_mask);
int s5gpu_devices_in_use(void);          /* devices the batch calls run on (0 before initialisation) */
/* Brings up, on the first device in use, what the first batch call would otherwise pay for: the HIP runtime and context, the kernels'
 * code objects (loaded on first launch) and one set of streams.  A tool calls it from a helper thread at start-up, under its own file
 * opening / index loading (examples/s5view.c, s5get.c: the first GPU call of a 100 k-id `get` was 175 ms of a 230 ms job).  Optional.
 * If the library is not initialised yet it initialises it as s5gpu_init(0) does — a caller that wants other devices calls
 * s5gpu_init_mask FIRST (afterwards it reports "already initialised"). */
int s5gpu_warmup(void);
void s5gpu_shutdown(void);
const char *s5gpu_last_error(void);
int s5gpu_device_count(void);
/* tuning knobs.  "inflate_par" (0/1, default 1): zlib records are inflated by the decoder that is parallel inside a record (one record
 * per wave, 64 self-synchronising segment decoders; whatever it declines is redone by the wave-per-record decoder).  With 0 the two
 * older kernels are used, chosen by batch size:  "inflate_simt_min": batches with at least this many zlib records use the lane-per-record
 * inflate kernel (throughput), smaller ones the wave-per-record kernel (latency); default 24576.
 * "inflate_route" (0/1, default 1): such batches are first counting-sorted by compressed length on the device, and records
 * of >= 32 KiB go to the wave-per-record kernel beside the lane kernel (real runs have read lengths spread over two decades).
 * "multi_min_per_device" (default 1024): a host batch of fewer than this many records per device stays on the first device.
 * "unpack_fused" (0/1, default 1): s5gpu_decode_dev on zlib / zstd + svb-zd records lets the wave that decompressed a record parse it and decode
 * its signal as well (fields.reserved is scratch on the way and 0 at the end); 0 = always the separate unpack kernel.
 * "zstd_sequences" (0/1, default 1): the zstd encoder sends runs of >= 5 equal bytes as one literal + one match at the repeat
 * offset (predefined FSE tables); 0 = literals-only frames cut at the record's seams (round 1; ~2 % larger records).
 * "fused_tier2" (bytes, 0 .. 16384, default 0 = off): batches of mixed lengths (s5gpu_encode_args.lds_payload_cap named) get a SECOND
 * one-workgroup-per-read launch with this LDS budget for the reads between the named budget and one 16 KiB DEFLATE block, before
 * the HBM-staged kernels take the rest; measured on real-run read lengths it gains nothing (profiles/r04_mixed_tier2.txt).
 * "order_min" (default 8192; 0 = never): batches of at least this many zlib / zstd records are DECODED longest record first (a counting sort
 * by compressed length on the device builds the launch order), and the overflow list of a mixed ENCODE batch (the reads the staged kernels
 * redo) is taken longest read first.  Costs 4 bytes per record of scratch per (device, stream), kept until s5gpu_shutdown; the sorted list of
 * "inflate_route" (batches of >= 1024 records, whatever order_min says) lives in the same scratch at the same cost.
 * "zstd_pre_min" (default 256; 0 = never): zstd batches of at least this many frames run a first pass that reads every frame's first tree
 * description, a frame per lane, in front of the decoder.  Costs 144 bytes per record in the same per-(device, stream) scratch
 * (144 MB for a million frames); a process that decodes on many short-lived streams should reuse streams or set this to 0. */
int s5gpu_set_option(const char *key, long value);

/* ---- device-resident entry points (asynchronous on `hip_stream`, a hipStream_t; NULL = default) ---- */
int s5gpu_encode_dev(const s5gpu_encode_args_t *args, void *hip_stream);
int s5gpu_decode_dev(const s5gpu_decode_args_t *args, void *hip_stream);
/* svb-zd only (BASELINE config 2): blob per read written at slots+out_off, out_len = blob bytes */
int s5gpu_svbzd_encode_dev(const s5gpu_encode_args_t *args, void *hip_stream);
/* Encode with ORDERED SINGLE-PASS OUTPUT (zlib record press): records go straight into the contiguous BLOW5 record
 * stream, rec_off[i] / rec_off[n] as s5gpu_compact_dev would produce them; no slots, no second pass.  args->slots and
 * args->ovf are not used.  state: n_reads u64 of scratch; ctl: 4 u32 of scratch, read them back after completion:
 * ctl[0] != 0 (some read did not fit the LDS budget) or ctl[2] != 0 (look-back timed out) => the stream is invalid,
 * fall back to s5gpu_encode_dev + s5gpu_compact_dev.  stream_out must hold the sum of the slot bounds. */
int s5gpu_encode_stream_dev(const s5gpu_encode_args_t *args, uint8_t *stream_out, uint64_t *rec_off, uint64_t *state,
                            uint32_t *ctl, void *hip_stream);
/* The same for the svb-zd stage alone (s5gpu_svbzd_encode_dev + s5gpu_compact_dev in one pass): blobs straight into the contiguous
 * blob stream; ctl as above (ctl[0]: a blob did not fit the LDS budget).  args->hdr / aux / slots / ovf are not used. */
int s5gpu_svbzd_encode_stream_dev(const s5gpu_encode_args_t *args, uint8_t *stream_out, uint64_t *rec_off, uint64_t *state,
                                  uint32_t *ctl, void *hip_stream);
/* single stages, for the solo press calls (slow5_ptr_compress_solo / slow5_ptr_depress_solo):
 *  deflate_parked: zlib-compress byte ranges already parked in their slots — read i's bytes sit at
 *    slots + out_off + ((slot_cap - s5gpu_payload_bound(desc i)) & ~15), out_len[i] = their length on entry
 *    and the framed length on return; works in place (see DESIGN.md "staged path").
 *  inflate: zlib streams -> payload slots, fields[i].status / payload_len (Adler-32 verified)
 *  svbzd_decode: svb-zd blobs (desc.in_off/in_len) -> sig_out, fields[i].status / n_samples */
int s5gpu_deflate_parked_dev(const s5gpu_encode_args_t *args, void *hip_stream);   /* rec_method zstd: the zstd twin */
/* pack_parked: the step in front of it for whole reads — signal press + record layout, every payload parked where deflate_parked
 *    expects it, out_len[i] = its length.  pack_parked + deflate_parked = s5gpu_encode_dev on a batch of long reads, as two calls a
 *    caller may put on different streams (bench.py's configs[3] leg: the next chunk's pack and the previous chunk's compaction run
 *    beside a chunk's deflate). */
int s5gpu_pack_parked_dev(const s5gpu_encode_args_t *args, void *hip_stream);
int s5gpu_inflate_dev(const s5gpu_decode_args_t *args, void *hip_stream);
int s5gpu_svbzd_decode_dev(const s5gpu_decode_args_t *args, void *hip_stream);
/* inflate_head: only the first desc[i].pay_cap bytes of every zlib record (a record's head: u16 read_id_len | read_id | ...; what
 * slow5_idx_create needs of a record), decoding stops there: fields[i].payload_len = bytes written, no Adler-32; desc[i].in_len may
 * cover just the front of the record (status 3 if it ends before pay_cap bytes are out). */
int s5gpu_inflate_head_dev(const s5gpu_decode_args_t *args, void *hip_stream);
/* Gather the slots into one contiguous BLOW5 record stream (what the ordered fwrite loop emits):
 * rec_off[i] = byte offset of record i in `stream`, rec_off[n] = total bytes.  tmp: >= 8*(n/1024+2) bytes. */
int s5gpu_compact_dev(uint32_t n_reads, const s5gpu_read_desc_t *desc, const uint8_t *slots, const uint32_t *out_len,
                      uint64_t *rec_off, uint8_t *stream, uint64_t *tmp, void *hip_stream);
/* write val[i] (little-endian u32) at base + off[i]: the read_group rewrite of merge (src/merge.c:51) on device */
int s5gpu_patch_u32_dev(uint8_t *base, const uint64_t *off, const uint32_t *val, uint32_t n, void *hip_stream);
/* qts rounding in place (slow5tools degrade, slow5_rec_qts_round): every sample x of record i, sig[sig_off[i] .. + n_samples[i]), becomes
 *     y = ((x + 2^(bits-1)) >> bits) << bits   in int32 (nearest multiple of 2^bits, ties toward +inf);  y > 32767: y -= 2^bits
 * bits 1..16 (else S5GPU_ERR_ARG).  sig_off / n_samples: device arrays of n entries, the records in order and apart
 * (sig_off[i] + n_samples[i] <= sig_off[i + 1]), every sig_off a multiple of 8.  Nothing outside the records' samples is touched. */
int s5gpu_qts_round_dev(int16_t *sig, uint32_t n, const uint64_t *sig_off, const uint32_t *n_samples, uint32_t bits, void *hip_stream);
/* synthetic reads on device (bench/test workload; bit-identical to oracle/synth.c) */
int s5gpu_synth_dev(int16_t *sig, uint64_t n_reads, uint64_t n_samples, uint64_t stride_samples, uint64_t seed,
                    uint64_t first_read_idx, void *hip_stream);
/* hdr bytes for synthetic reads: 74 bytes per read (36-char id, read_group 0, 8192/23/1467.61/4000) */
int s5gpu_synth_hdr_dev(uint8_t *hdr, uint64_t n_reads, uint64_t first_read_idx, void *hip_stream);

/* timing hook: runs fn-equivalent `iters` times between two hipEvents on the stream, returns ms (bench.py) */
int s5gpu_event_create(void **ev);
int s5gpu_event_record(void *ev, void *hip_stream);
int s5gpu_event_elapsed_ms(void *ev_start, void *ev_stop, float *ms);   /* synchronises on ev_stop */
int s5gpu_event_destroy(void *ev);

/* ---- host-buffer batch entry points: the work_db replacement ---- */
/* Encode n reads.  hdr[i]/aux[i] as in s5gpu_read_desc_t.  out[i] receives a malloc'd buffer the caller
 * frees (ownership as slow5_rec_to_mem, /root/reference/src/view.c:49,298); out_len[i] its length. */
int s5gpu_encode_batch(uint32_t n, const int16_t *const *sig, const uint64_t *n_samples, const void *const *hdr,
                       const uint32_t *hdr_len, const void *const *aux, const uint32_t *aux_len, int rec_method,
                       int sig_method, void **out, size_t *out_len);
/* Decode n records (bytes without the u64 prefix).  payload[i] and sig[i] receive malloc'd buffers. */
int s5gpu_decode_batch(uint32_t n, const void *const *rec, const size_t *rec_len, int rec_method, int sig_method,
                       void **payload, int16_t **sig, s5gpu_rec_fields_t *fields);

/* The whole view / merge worker for a batch of BLOW5 records (src/view.c:35-57, src/merge.c:43-70): decode with
 * (from_rec, from_sig), optionally rewrite read_group and drop the aux fields, re-encode with (to_rec, to_sig).
 * Only compressed bytes cross PCIe: decoded signals and payloads stay in HBM between the two halves.
 * out[i] malloc'd [u64 size][record]; a corrupt input record fails the call (status[i], may be NULL, says which). */
int s5gpu_recompress_batch(uint32_t n, const void *const *rec, const size_t *rec_len, int from_rec, int from_sig, int to_rec,
                           int to_sig, const uint32_t *new_read_group, int drop_aux, void **out, size_t *out_len,
                           int32_t *status);

/* The ARENA form of the two calls above (round 5).  One malloc per record is what slow5_rec_to_mem promises (src/view.c:49,298), and at
 * a million records per call it is what bounds the call: a million fresh buffers the process has never touched, page-faulted in one by
 * one.  Here out[i] point INTO a few pinned buffers the device-to-host copies landed in — no copy, no allocation per record — and the
 * caller gives the whole batch back with ONE s5gpu_arena_release(*arena) once its ordered write loop is through (the free() of
 * src/view.c:298 goes).  The buffers return to a process-wide pool (up to 6 GB kept; drained by s5gpu_shutdown), so a loop of
 * similar batches neither allocates nor faults after its first ones.  *arena is NULL when the call fails.  Never free() an out[i]. */
int s5gpu_encode_batch_arena(uint32_t n, const int16_t *const *sig, const uint64_t *n_samples, const void *const *hdr,
                             const uint32_t *hdr_len, const void *const *aux, const uint32_t *aux_len, int rec_method,
                             int sig_method, void **out, size_t *out_len, void **arena);
int s5gpu_recompress_batch_arena(uint32_t n, const void *const *rec, const size_t *rec_len, int from_rec, int from_sig, int to_rec,
                                 int to_sig, const uint32_t *new_read_group, int drop_aux, void **out, size_t *out_len,
                                 int32_t *status, void **arena);
void s5gpu_arena_release(void *arena);   /* NULL is fine */

/* The two calls as SUBMIT / WAIT pairs (round 6): the reference's loop reads K records, works on them, writes them, and overlaps nothing
 * (/root/reference/src/view.c:254-300; /root/reference/README.md:197 names the overlap as future work).  A submitted batch runs on a
 * thread of the library's and takes one of its contexts (S5GPU_CONTEXTS, default 2): with two tickets in flight one batch's PCIe copies
 * run under the other's kernels while the caller reads the next batch.  want_arena != 0: out[i] point into an arena that
 * s5gpu_batch_wait hands over (release it with s5gpu_arena_release); 0: one malloc per record.  Every array named here belongs to the
 * library until the ticket is waited for; every ticket is waited for exactly once.  NULL ticket: s5gpu_last_error() says why.
 * s5gpu_batch_wait returns the batch call's own code, its message in the waiting thread's s5gpu_last_error(). */
void *s5gpu_recompress_batch_submit(uint32_t n, const void *const *rec, const size_t *rec_len, int from_rec, int from_sig, int to_rec,
                                    int to_sig, const uint32_t *new_read_group, int drop_aux, void **out, size_t *out_len,
                                    int32_t *status, int want_arena);
void *s5gpu_encode_batch_submit(uint32_t n, const int16_t *const *sig, const uint64_t *n_samples, const void *const *hdr,
                                const uint32_t *hdr_len, const void *const *aux, const uint32_t *aux_len, int rec_method,
                                int sig_method, void **out, size_t *out_len, int want_arena);
int s5gpu_batch_wait(void *ticket, void **arena);

/* The same worker on a CHUNK of a BLOW5 file (what bounds `view` end to end is the read and write phases around
 * work_db, /root/reference/src/view.c:265-278,296-299, not the compute).  The n records sit framed — [u64 size][bytes] — in one
 * host buffer `chunk` exactly as read from disk: rec_pos[i] = offset of record i's bytes (behind its size prefix), rec_len[i]
 * their length.  The re-encoded records come back as ONE contiguous stream in out_buf, exactly the bytes the ordered write loop
 * emits: out_off[i] = offset of record i (its u64 prefix), out_off[n] = total.  No per-record malloc or memcpy on either side.
 * chunk / out_buf from s5gpu_host_alloc (pinned) move at PCIe speed; any host memory works.  If out_cap is too small the call
 * fails with S5GPU_ERR_NOMEM and out_off[0] = the capacity needed.
 * s5gpu_host_alloc never pins less than 2 MiB at a time (meant for chunk-sized buffers, not for small objects): round 5 met small pinned
 * buffers, allocated by one host thread while another was inside its first batch, that device copies did not reach. */
void *s5gpu_host_alloc(size_t bytes);
void s5gpu_host_free(void *p);
int s5gpu_recompress_stream(uint32_t n, const void *chunk, size_t chunk_bytes, const uint64_t *rec_pos, const uint32_t *rec_len, int from_rec,
                            int from_sig, int to_rec, int to_sig, const uint32_t *new_read_group, int drop_aux, void *out_buf, size_t out_cap,
                            uint64_t *out_off, int32_t *status);

/* The decode half alone on a chunk of framed records (`get --benchmark`, /root/reference/src/get.c:52, and any consumer of signals): the
 * decoded signals come back as ONE contiguous int16 block — sig_off[i] = first sample of record i, sig_off[n] = total — and the parsed
 * fields in fields[i]; no malloc per record.  sig_cap in samples; too little: S5GPU_ERR_NOMEM and sig_off[0] = samples needed.  A corrupt
 * record fails the call with S5GPU_ERR_DATA (fields[i].status says which; with several devices, records of a share that gave up because
 * another share failed read S5GPU_STATUS_NOT_DECODED, never 0). */
#define S5GPU_STATUS_NOT_DECODED 15
int s5gpu_decode_stream(uint32_t n, const void *chunk, size_t chunk_bytes, const uint64_t *rec_pos, const uint32_t *rec_len, int rec_method,
                        int sig_method, int16_t *sig_out, size_t sig_cap, uint64_t *sig_off, s5gpu_rec_fields_t *fields);

/* The read ids of the n records of a file chunk (framed as for s5gpu_recompress_stream), for the index builder (slow5_idx_create): only the
 * front of every zlib record crosses PCIe and only its first 2 + id_pitch bytes are inflated; uncompressed records are read on the host.
 * ids: n * id_pitch bytes (id i at ids + i * id_pitch, id_len[i] bytes, not terminated).  status[i] != 0: this record needs the general
 * decode (id longer than id_pitch: 5; corrupt: 1-4, 7).  rec_method zstd is refused (S5GPU_ERR_ARG). */
int s5gpu_record_ids_stream(uint32_t n, const void *chunk, size_t chunk_bytes, const uint64_t *rec_pos, const uint32_t *rec_len, int rec_method,
                            uint32_t id_pitch, char *ids, uint16_t *id_len, int32_t *status);

/* ---- one-stage host-buffer calls behind slow5_ptr_compress_solo / slow5_ptr_depress_solo ----
 * stage: 0 zlib compress, 1 zlib inflate, 2 svb-zd encode (in = int16 samples, in_len in bytes),
 * 3 svb-zd decode, 4 zstd decompress (whole frames), 5 zstd compress, 6 ex-zd encode (in = int16 samples), 7 ex-zd decode.
 * out[i] malloc'd, caller frees.  status[i] per record (0 ok), may be NULL. */
int s5gpu_solo_batch(int stage, uint32_t n, const void *const *in, const size_t *in_len, void **out, size_t *out_len,
                     int32_t *status);

/* ---- SLOW5 ASCII <-> BLOW5 (the parse/format half of slow5_rec_depress_parse / slow5_rec_to_mem
 * when one side of `view` is a .slow5 file, /root/reference/src/view.c:35-57) ----
 * The raw_signal column (comma-separated decimal int16) is ~95 % of an ASCII record: it is parsed / formatted on the
 * device, one read per workgroup.  The handful of scalar columns and the aux columns are converted on the host. */
typedef struct {             /* 32 B: one read's raw_signal text on the device */
    uint64_t txt_off;        /* byte offset of the text in `text` (any alignment) */
    uint64_t sig_off;        /* int16 index of the first sample in `sig` */
    uint32_t txt_len;        /* parse: length of the text; format: capacity of the text slot (7 bytes/sample is enough) */
    uint32_t n_samples;      /* parse: the count the len_raw_signal column promised; format: samples to print */
    uint32_t reserved[2];
} s5gpu_txt_desc_t;
/* status[i]: 0 ok, 1 bad character, 2 value out of int16 range / too many digits, 3 empty number, 4 count mismatch,
 * 5 text slot too small.  `text` needs 32 readable bytes after the last read. */
int s5gpu_ascii_parse_dev(uint32_t n, const s5gpu_txt_desc_t *desc, const uint8_t *text, int16_t *sig, int32_t *status, void *stream);
int s5gpu_ascii_format_dev(uint32_t n, const s5gpu_txt_desc_t *desc, const int16_t *sig, uint8_t *text, uint32_t *txt_len,
                           int32_t *status, void *stream);
/* copy n byte ranges src[src_off[i] .. +len[i]) -> dst[dst_off[i] ..) on the device */
/* dst[0, bytes) = src[0, bytes) by a kernel on `stream`: both 16-byte aligned, with room for `bytes` rounded up to 16.  dst may be pinned host
 * memory (s5gpu_host_alloc): results then travel as the kernel's own stores, not through the copy engines every stream of the process shares. */
int s5gpu_copy_dev(void *dst, const void *src, uint64_t bytes, void *stream);
int s5gpu_gather_dev(uint32_t n, const uint64_t *src_off, const uint32_t *len, const uint64_t *dst_off, const uint8_t *src, uint8_t *dst,
                     void *stream);

/* aux column types of a SLOW5 header, in column order: low 4 bits = element kind, bit 7 = array ("type*"; char* = string) */
enum { S5GPU_AUX_INT8 = 0, S5GPU_AUX_INT16, S5GPU_AUX_INT32, S5GPU_AUX_INT64, S5GPU_AUX_UINT8, S5GPU_AUX_UINT16, S5GPU_AUX_UINT32,
       S5GPU_AUX_UINT64, S5GPU_AUX_FLOAT, S5GPU_AUX_DOUBLE, S5GPU_AUX_CHAR, S5GPU_AUX_ENUM, S5GPU_AUX_ARRAY = 0x80 };
/* Types line of a SLOW5 header ("#char*\tuint32_t\t...") -> aux type codes of the columns after raw_signal.
 * Returns the number of aux columns (<= cap), or a negative S5GPU_ERR_*. */
int s5gpu_aux_types_parse(const char *types_line, size_t len, uint8_t *aux_type, uint32_t cap);

/* ASCII records (one line each, with or without the trailing newline) -> BLOW5 records [u64 size][press(payload)].
 * new_read_group / drop_aux as in s5gpu_recompress_batch.  status[i] (may be NULL): 0 ok, 1-5 as above, 16 malformed line. */
int s5gpu_ascii_to_blow5_batch(uint32_t n, const char *const *line, const size_t *line_len, uint32_t n_aux, const uint8_t *aux_type,
                               int to_rec, int to_sig, const uint32_t *new_read_group, int drop_aux, void **out, size_t *out_len,
                               int32_t *status);
/* The same on a CHUNK of a .slow5 file, for a loop that reads the file in large pieces (examples/s5view.c; what s5gpu_recompress_stream
 * is for BLOW5 input): the n record lines sit in one host buffer `chunk` exactly as read from disk, line_pos[i] / line_len[i] = offset and
 * length of line i (with or without its newline).  The chunk is uploaded as it is and the raw_signal columns are parsed where they lie;
 * the BLOW5 records come back as ONE contiguous stream in out_buf (out_off[i] = offset of record i's u64 prefix, out_off[n] = total):
 * no per-line malloc or memcpy on either side.  Too little room: S5GPU_ERR_NOMEM and out_off[0] = the capacity needed.  `chunk` needs
 * 32 readable bytes behind the last line. */
int s5gpu_ascii_to_blow5_stream(uint32_t n, const void *chunk, size_t chunk_bytes, const uint64_t *line_pos, const uint32_t *line_len,
                                uint32_t n_aux, const uint8_t *aux_type, int to_rec, int to_sig, const uint32_t *new_read_group, int drop_aux,
                                void *out_buf, size_t out_cap, uint64_t *out_off, int32_t *status);
/* slot r (desc[r].out_off in `slots`, len[r] bytes) -> dst + off[r], on the device (the copy of s5gpu_compact_dev with the destinations given) */
int s5gpu_scatter_slots_dev(uint32_t n, const s5gpu_read_desc_t *desc, const uint8_t *slots, const uint32_t *len, const uint64_t *off, uint8_t *dst,
                            void *hip_stream);
/* ... and the other way round on a CHUNK of a BLOW5 file (records framed as for s5gpu_recompress_stream): the SLOW5 text lines of the n records
 * come back as ONE contiguous block in out_buf (out_off[i] = start of line i, out_off[n] = total; every line ends in a newline) — the signal
 * columns printed on the device, prefix | signal | suffix of every line put in place there, one D2H.  Too little room: S5GPU_ERR_NOMEM and
 * out_off[0] = the capacity needed. */
int s5gpu_blow5_to_ascii_stream(uint32_t n, const void *chunk, size_t chunk_bytes, const uint64_t *rec_pos, const uint32_t *rec_len, int from_rec,
                                int from_sig, uint32_t n_aux, const uint8_t *aux_type, const uint32_t *new_read_group, int drop_aux,
                                void *out_buf, size_t out_cap, uint64_t *out_off, int32_t *status);
/* BLOW5 records (bytes without the u64 prefix) -> ASCII lines ending in a newline; out[i] malloc'd. */
int s5gpu_blow5_to_ascii_batch(uint32_t n, const void *const *rec, const size_t *rec_len, int from_rec, int from_sig, uint32_t n_aux,
                               const uint8_t *aux_type, const uint32_t *new_read_group, int drop_aux, void **out, size_t *out_len,
                               int32_t *status);
/* SLOW5 -> SLOW5 (get --to slow5 on a .slow5): every line printed again, byte for byte what slow5_gpu_convert_batch(ASCII -> ASCII) gives.
 * Arguments, status[i] and the NOMEM protocol of s5gpu_ascii_to_blow5_stream without the press methods; the lines come back as ONE block
 * laid out as by s5gpu_blow5_to_ascii_stream. */
int s5gpu_ascii_to_ascii_stream(uint32_t n, const void *chunk, size_t chunk_bytes, const uint64_t *line_pos, const uint32_t *line_len,
                                uint32_t n_aux, const uint8_t *aux_type, const uint32_t *new_read_group, int drop_aux,
                                void *out_buf, size_t out_cap, uint64_t *out_off, int32_t *status);
/* its batch twin: lines (with or without the newline) -> lines ending in a newline, out[i] malloc'd */
int s5gpu_ascii_to_ascii_batch(uint32_t n, const char *const *line, const size_t *line_len, uint32_t n_aux, const uint8_t *aux_type,
                               const uint32_t *new_read_group, int drop_aux, void **out, size_t *out_len, int32_t *status);

/* _qts twins of the convert calls (slow5tools degrade, src/degrade.c:235-271): the same arguments and results, with every sample
 * qts-rounded to qts_bits (1..16, else S5GPU_ERR_ARG; the rule at s5gpu_qts_round_dev) on the device between the stage that makes the
 * signals (decode / text parse) and the one that takes them (encode / text format).  The plain calls round nothing. */
int s5gpu_recompress_batch_qts(uint32_t n, const void *const *rec, const size_t *rec_len, int from_rec, int from_sig, int to_rec,
                               int to_sig, const uint32_t *new_read_group, int drop_aux, void **out, size_t *out_len,
                               int32_t *status, uint32_t qts_bits);
int s5gpu_recompress_stream_qts(uint32_t n, const void *chunk, size_t chunk_bytes, const uint64_t *rec_pos, const uint32_t *rec_len, int from_rec,
                                int from_sig, int to_rec, int to_sig, const uint32_t *new_read_group, int drop_aux, void *out_buf,
                                size_t out_cap, uint64_t *out_off, int32_t *status, uint32_t qts_bits);
int s5gpu_ascii_to_blow5_batch_qts(uint32_t n, const char *const *line, const size_t *line_len, uint32_t n_aux, const uint8_t *aux_type,
                                   int to_rec, int to_sig, const uint32_t *new_read_group, int drop_aux, void **out, size_t *out_len,
                                   int32_t *status, uint32_t qts_bits);
int s5gpu_ascii_to_blow5_stream_qts(uint32_t n, const void *chunk, size_t chunk_bytes, const uint64_t *line_pos, const uint32_t *line_len,
                                    uint32_t n_aux, const uint8_t *aux_type, int to_rec, int to_sig, const uint32_t *new_read_group, int drop_aux,
                                    void *out_buf, size_t out_cap, uint64_t *out_off, int32_t *status, uint32_t qts_bits);
int s5gpu_blow5_to_ascii_batch_qts(uint32_t n, const void *const *rec, const size_t *rec_len, int from_rec, int from_sig, uint32_t n_aux,
                                   const uint8_t *aux_type, const uint32_t *new_read_group, int drop_aux, void **out, size_t *out_len,
                                   int32_t *status, uint32_t qts_bits);
int s5gpu_blow5_to_ascii_stream_qts(uint32_t n, const void *chunk, size_t chunk_bytes, const uint64_t *rec_pos, const uint32_t *rec_len, int from_rec,
                                    int from_sig, uint32_t n_aux, const uint8_t *aux_type, const uint32_t *new_read_group, int drop_aux,
                                    void *out_buf, size_t out_cap, uint64_t *out_off, int32_t *status, uint32_t qts_bits);

/* ---- skim (slow5tools skim, src/skim.c): every field of every read but the raw signal, one text line per record ----
 * The line: read_id \t read_group \t digitisation \t offset \t range \t sampling_rate \t len_raw_signal \t . [\t aux]... \n, doubles as
 * "%f" with trailing zeros and a bare '.' trimmed, len_raw_signal the SAMPLE count (read from the signal blob's head: the signal is never
 * decoded), each aux field printed by the role its NAME gives it (src/skim.c:227-260; docs/codecs.md §4.9). */
enum { S5GPU_SKIM_DOT = 0,      /* a field skim does not handle (arrays included): "."                            */
       S5GPU_SKIM_STRING,       /* channel_number (char*): the string, "." when empty                             */
       S5GPU_SKIM_DOUBLE,       /* median_before: "%f"-trimmed, NaN "."                                           */
       S5GPU_SKIM_FLOAT,        /* tracked_scaling_shift / _scale, predicted_scaling_shift / _scale, time_since_mux_change */
       S5GPU_SKIM_INT32,        /* read_number; "." for INT32_MAX                                                 */
       S5GPU_SKIM_UINT8,        /* start_mux; "." for 255                                                         */
       S5GPU_SKIM_UINT32,       /* num_reads_since_mux_change; "." for UINT32_MAX                                 */
       S5GPU_SKIM_UINT64,       /* start_time, num_minknow_events; "." for UINT64_MAX                             */
       S5GPU_SKIM_ENUM };       /* end_reason: its label from the header's enum{...}; "." for 255                 */
#define S5GPU_SKIM_MAX_AUX 64
#define S5GPU_SKIM_MAX_LABELS 1024
#define S5GPU_SKIM_TEXT 16384
/* record status of the skim calls beside 1-5 and 7 (s5gpu_rec_fields_t): an enum value at or past the label count */
#define S5GPU_STATUS_BAD_ENUM 8
/* What skim needs of a header, parsed once per file.  Field a's name and enum labels sit in text[]. */
typedef struct s5gpu_skim_layout {
    uint32_t n_aux;                              /* aux fields, header order                                  */
    uint32_t n_labels_total;
    uint32_t text_len;
    uint32_t n_unhandled;                        /* fields with role S5GPU_SKIM_DOT (s5skim warns once each)  */
    uint8_t type[S5GPU_SKIM_MAX_AUX];            /* S5GPU_AUX_* code: how the field's bytes are laid out      */
    uint8_t role[S5GPU_SKIM_MAX_AUX];            /* S5GPU_SKIM_*: how it prints                               */
    uint16_t n_labels[S5GPU_SKIM_MAX_AUX];       /* enum fields: label count                                  */
    uint16_t label_first[S5GPU_SKIM_MAX_AUX];    /* enum fields: index of the first label in label_off / len  */
    uint32_t name_off[S5GPU_SKIM_MAX_AUX];       /* field name at text + name_off, name_len bytes             */
    uint32_t name_len[S5GPU_SKIM_MAX_AUX];
    uint32_t label_off[S5GPU_SKIM_MAX_LABELS];   /* label l at text + label_off[l], label_len[l] bytes        */
    uint16_t label_len[S5GPU_SKIM_MAX_LABELS];
    char text[S5GPU_SKIM_TEXT];
} s5gpu_skim_layout_t;
/* header text (as stored in a BLOW5 header: the '@' lines, the types line "#char*\t...", the names line "#read_id\t...") -> layout.
 * S5GPU_ERR_DATA when a field skim prints by name is declared with another type (slow5lib's slow5_aux_get_<type> fails on it) or the
 * two '#' lines are missing or disagree; S5GPU_ERR_ARG when the header has more fields, labels or name bytes than the layout holds. */
int s5gpu_skim_layout_parse(const char *header, size_t len, s5gpu_skim_layout_t *layout);
/* The skim worker on a CHUNK of a BLOW5 file (records framed as for s5gpu_recompress_stream): the lines of the n records come back as ONE
 * contiguous block of text in out_buf, out_off[i] = start of line i, out_off[n] = total.  Records are inflated on the device (zlib, zstd)
 * or taken as they are (record press none), the lines formatted there (k_skim_format), one D2H of finished text.  Too little room:
 * S5GPU_ERR_NOMEM and out_off[0] = the bytes needed.  A bad record fails the call with S5GPU_ERR_DATA; status[i] (may be NULL) says which:
 * 1-5 as in s5gpu_rec_fields_t, 7 malformed record, S5GPU_STATUS_BAD_ENUM.  Several devices split the records as the other chunk calls do. */
int s5gpu_skim_stream(uint32_t n, const void *chunk, size_t chunk_bytes, const uint64_t *rec_pos, const uint32_t *rec_len, int rec_method,
                      int sig_method, const s5gpu_skim_layout_t *layout, void *out_buf, size_t out_cap, uint64_t *out_off, int32_t *status);
/* ... on n records anywhere in host memory (bytes without the u64 prefix): out[i] = line i, malloc'd and NUL-terminated (a C string, as the
 * reference's print loop takes it: src/skim.c:416-420), out_len[i] its length without the NUL */
int s5gpu_skim_batch(uint32_t n, const void *const *rec, const size_t *rec_len, int rec_method, int sig_method, const s5gpu_skim_layout_t *layout,
                     void **out, size_t *out_len, int32_t *status);

/* ---- signals: per-read order statistics and normalised tensors of DECODED reads, on the device (docs/codecs.md §4.11) ----
 * The input is what s5gpu_decode_dev left behind: `sig`, and per record its sig_off (a multiple of 8 samples), the sig_cap the decoder was
 * given for it, and its parsed fields.  The samples a kernel may touch of record i are
 *     n_eff = fields[i].status == 0 ? min(fields[i].n_samples, sig_cap[i]) : 0
 * never n_samples as it stands (a record that failed with status 6 holds the count it NEEDED there).  Every statistic is an integer. */
typedef struct s5gpu_sig_stats {
    uint32_t n;            /* n_eff; 0: every other member but status is 0                                         */
    int32_t status;        /* 0 ok, else the record's decode status (s5gpu_rec_fields_t)                           */
    int64_t sum;
    uint64_t sumsq;        /* exact: x^2 <= 2^30, n < 2^32                                                         */
    int32_t med2;          /* 2 x median: s[(n-1)/2] + s[n/2] of the sorted samples s                              */
    uint32_t mad4;         /* 4 x MAD: ks[(n-1)/2] + ks[n/2] of the sorted keys |2x - med2| (0 .. 131070)          */
    int16_t min, max;
    int16_t q[4];          /* q[k] = s[floor(q_k * (n-1))] (the "lower" order statistic; product in double); unused: 0 */
    uint32_t reserved;     /* 0 */
} s5gpu_sig_stats_t;
/* n records -> stats[i].  q: n_q (<= 4) quantiles in [0, 1], a HOST array (may be NULL when n_q == 0).  sig_off / sig_cap / fields / stats:
 * device arrays of n entries.  Asynchronous on hip_stream. */
int s5gpu_signal_stats_dev(uint32_t n, const int16_t *sig, const uint64_t *sig_off, const uint32_t *sig_cap, const s5gpu_rec_fields_t *fields,
                           uint32_t n_q, const double *q, s5gpu_sig_stats_t *stats, void *hip_stream);
enum { S5GPU_NORM_RAW = 0,      /* float(x)                                                                                  */
       S5GPU_NORM_PA,           /* float32((double(x) + offset) * (range / digitisation)), in double from the read's fields  */
       S5GPU_NORM_MEDMAD,       /* (2x - med2) / (0.7413f * mad4) = (x - med) / (1.4826 MAD); scale 1 when mad4 == 0         */
       S5GPU_NORM_QUANT };      /* (x - a (q[0] + q[1])) / max(b (q[1] - q[0]), 1), in double, rounded to float32 once       */
enum { S5GPU_SIG_F32 = 0, S5GPU_SIG_F16 = 1 };   /* float16 = the float32 result rounded to nearest even */
/* A dense [n_windows, W] tensor of normalised samples at `out` (16-byte aligned).  Window w = (read win_read[w], start win_start[w]), device
 * arrays: element j of its row is sample win_start[w] + j of that read where that lies below n_eff, and 0 otherwise.  A window whose read is
 * >= n or failed, or whose start is > n_eff, is a row of zeros and win_status[w] = 1 (else 0): it is never loaded from.  stats: what
 * s5gpu_signal_stats_dev wrote for the same records (MEDMAD, QUANT; may be NULL for RAW and PA).  a, b: QUANT only. */
int s5gpu_signal_windows_dev(uint32_t n, const int16_t *sig, const uint64_t *sig_off, const uint32_t *sig_cap, const s5gpu_rec_fields_t *fields,
                             const s5gpu_sig_stats_t *stats, uint32_t n_windows, const uint32_t *win_read, const uint32_t *win_start, uint32_t W,
                             int mode, double a, double b, int dtype, void *out, int32_t *win_status, void *hip_stream);
/* Statistics of the n records of a file chunk (framed as for s5gpu_decode_stream): one upload, the decode (fields + signals only where the
 * methods allow S5GPU_DEC_NO_PAYLOAD, the full form otherwise), the statistics kernel, and one small download of stats_out[i] and fields_out[i]
 * (may be NULL): the signals never leave the device.  Runs on the FIRST device in use, whatever s5gpu_init_mask named.  A corrupt record
 * fails the call with S5GPU_ERR_DATA; stats_out[i].status / fields_out[i].status say which, the other records' results are valid. */
int s5gpu_signal_stats_stream(uint32_t n, const void *chunk, size_t chunk_bytes, const uint64_t *rec_pos, const uint32_t *rec_len, int rec_method,
                              int sig_method, uint32_t n_q, const double *q, s5gpu_sig_stats_t *stats_out, s5gpu_rec_fields_t *fields_out);

/* ---- sum: a content digest per read, independent of the presses the record was stored with, hashed on the device (docs/codecs.md §4.12) ----
 * The CANONICAL record C(r) of a read is its record as a BLOW5 file with record press none and signal press none stores it, without the u64
 * size prefix:  u16 read_id_len | read_id | u32 read_group | 4 x f64 | u64 N | N x int16 LE | the aux bytes unchanged.  Its digest is
 * XXH64(C(r), seed 0).  C(r) is never built: the kernel hashes payload[0, 2 + id_len + 36), the 8 bytes of N, 2N bytes of the record's
 * signal slot and payload[aux_off, aux_off + aux_len) as one stream.  The digest resists accidents, not adversaries.
 *
 * s5gpu_digest_dev: the input is what the full form of s5gpu_decode_dev (flags = 0) left behind: the descriptors it was given, its payload
 * slots, its sig_out and its fields (all device; payload and sig 16-byte aligned, desc / fields / digest 8).  digest[i] = the digest of
 * record i, or 0 for a record with fields[i].status != 0 or whose fields point outside its own slots: nothing of such a record is read.
 * The kernel loads aligned 8-byte words: it touches [pay_off, pay_off + pay_cap) and the record's signal slot rounded out to 16 bytes and
 * nothing else, so 16 readable bytes must follow the last slot of `payload` and of `sig`.  sig_method: the signal press the records were
 * decoded from (S5GPU_SIG_*; checked, the decoded form does not depend on it).  Asynchronous on hip_stream. */
int s5gpu_digest_dev(uint32_t n, const s5gpu_rec_desc_t *desc, const uint8_t *payload, const int16_t *sig, const s5gpu_rec_fields_t *fields,
                     int sig_method, uint64_t *digest, void *hip_stream);
/* The digests of the n records of a file chunk (framed as for s5gpu_decode_stream) and of n records anywhere in host memory (bytes without the
 * u64 prefix): one upload, the full decode, the digest kernel, and a download of 8 bytes per record; every record press x signal press.  Both
 * run on the FIRST device in use.  A corrupt record fails the call with S5GPU_ERR_DATA: its status_out[i] (may be NULL) is the decoder's
 * (s5gpu_rec_fields_t.status) and its digest 0; the other records' digests are valid. */
int s5gpu_digest_stream(uint32_t n, const void *chunk, size_t chunk_bytes, const uint64_t *rec_pos, const uint32_t *rec_len, int rec_method,
                        int sig_method, uint64_t *digest_out, int32_t *status_out);
int s5gpu_digest_batch(uint32_t n, const void *const *rec, const size_t *rec_len, int rec_method, int sig_method, uint64_t *digest_out,
                       int32_t *status_out);

/* ---- stats: what is in a whole file's signal, accumulated on the device while the batches stream through (docs/codecs.md §4.13) ----
 * One accumulator per file stays in device memory; its 528 720 bytes come back once.  Every member is an integer sum, minimum, maximum, OR or
 * AND over the records with status 0 and their n_eff samples (the rule of "signals" above): the result does not depend on the batches the file
 * was cut into, on their order or on the launch shape.  A record with status != 0 adds 1 to n_failed and nothing else; none of its samples is
 * loaded.  The layout is fixed (little-endian, no padding). */
typedef struct s5gpu_file_stats {
    uint64_t n_reads;          /* records with status 0                                                                     */
    uint64_t n_failed;         /* records with any other status                                                             */
    uint64_t n_samples;
    int64_t sum;
    uint64_t sumsq;            /* the sum of x^2 modulo 2^64: it WRAPS (x^2 <= 2^30, so not before 2^34 samples)             */
    int32_t min, max;          /* 32767 / -32768 while there is no sample                                                   */
    uint32_t or_bits;          /* OR of (uint16_t)x; 0 while there is no sample                                             */
    uint32_t and_bits;         /* AND of (uint16_t)x; 0xFFFF while there is no sample                                       */
    uint32_t len_min, len_max; /* samples of the shortest / longest read; 0xFFFFFFFF / 0 while there is no read             */
    uint64_t len_hist[33];     /* reads by length class: [0] reads of 0 samples, else [1 + floor(log2 n)]                   */
    uint64_t rg_reads[256];    /* reads of read group g < 256                                                               */
    uint64_t rg_samples[256];  /* their samples                                                                             */
    uint64_t rg_other;         /* reads of read groups >= 256 (their samples are in n_samples only)                         */
    uint64_t hist[65536];      /* samples of value x at [x + 32768]                                                         */
} s5gpu_file_stats_t;
/* acc: device memory, 8-byte aligned, sizeof(s5gpu_file_stats_t).  reset: the empty accumulator.  accum: adds n records; the input is what
 * s5gpu_decode_dev left behind, exactly as for s5gpu_signal_stats_dev (sig 16-byte aligned; sig_off / sig_cap / fields device arrays).  Both are
 * asynchronous on hip_stream; accum calls on one acc may run on several streams at once (it only adds with atomics).
 * A workgroup counts the samples inside a window of values in LDS and sends the others straight to acc->hist with 64-bit atomics; it empties
 * its LDS counters into acc->hist before one of them could wrap, and at its end.  Where the window lies changes the time, never the result.
 * s5gpu_set_option (tests, tools):
 *   "fstats_window_lo"     -1 (default): each workgroup centres the window on the mean of the first samples it meets; 0 .. 65535: the bin
 *                          (value + 32768) of the window's low edge, moved down where the window would pass bin 65535.
 *   "fstats_lds_bins"      bins of the window: 0 (no LDS histogram: every sample is a global atomic) or a power of two from 64 to 2048 (default).
 *   "fstats_flush_samples" 1 .. 4294967295 (default): a workgroup empties its LDS counters before a read would take the samples it has counted
 *                          since the last time past this number.
 *   "fstats_grid"          1 .. 1024 (default): the most workgroups of one launch; below the record count a workgroup walks several records. */
size_t s5gpu_file_stats_bytes(void);   /* sizeof(s5gpu_file_stats_t) as the library was built */
int s5gpu_file_stats_reset_dev(s5gpu_file_stats_t *acc, void *hip_stream);
int s5gpu_file_stats_accum_dev(uint32_t n, const int16_t *sig, const uint64_t *sig_off, const uint32_t *sig_cap, const s5gpu_rec_fields_t *fields,
                               s5gpu_file_stats_t *acc, void *hip_stream);
/* The chunk calls: an opaque per-file handle that owns one accumulator on the FIRST device in use (NULL + s5gpu_last_error() on failure).
 * add_stream: n records framed as for s5gpu_decode_stream: one upload, one decode (fields + signals only where the methods allow
 * S5GPU_DEC_NO_PAYLOAD, the full form otherwise; every record press x signal press), the accumulate kernel; nothing comes back but
 * status_out[i] (may be NULL).  A corrupt record fails the call with S5GPU_ERR_DATA: it is counted in n_failed, the other records of the batch
 * are accumulated, and the handle stays usable.  Only then may the batch be decoded more than once: the decoder's own retry of records that
 * outgrew their guessed slots stops at a corrupt record, so the batch is decoded again without the corrupt ones (at most three more times; in
 * the full form each of these uploads the chunk again); a record that still has status 5 or 6 after the last is counted in n_failed.
 * close: the single download into *out (may be NULL: the accumulator is abandoned) and the end of the handle, whatever it returns.
 * Not built: several devices per file (a file's batches all go to the first device), a choice of qts bits from or_bits (`degrade -b auto`),
 * and N50, which needs the sorted read lengths and not their classes. */
void *s5gpu_file_stats_open(void);
int s5gpu_file_stats_add_stream(void *h, uint32_t n, const void *chunk, size_t chunk_bytes, const uint64_t *rec_pos, const uint32_t *rec_len,
                                int rec_method, int sig_method, int32_t *status_out);
int s5gpu_file_stats_close(void *h, s5gpu_file_stats_t *out);

/* ---- diff: where and by how much the reads of two files differ, compared on the device (docs/codecs.md §4.14) ----
 * A PAIR is read ia of decoded batch A and read ib of decoded batch B; each batch is what s5gpu_decode_dev left behind, and the two may come
 * from different record and signal presses.  The sample count of each side is n_eff (the rule of "signals" above) and nothing else;
 * n_cmp = min(n_a, n_b); d[i] = b[i] - a[i] as int32 for i < n_cmp.  Samples past n_cmp are never loaded.  Every member is an integer. */
enum { S5GPU_DIFF_SIGNAL = 1,          /* n_diff > 0                                                                             */
       S5GPU_DIFF_LEN = 2,             /* n_a != n_b                                                                             */
       S5GPU_DIFF_READ_GROUP = 4,
       S5GPU_DIFF_DIGITISATION = 8,    /* the four doubles are compared bit for bit: 0.0 and -0.0 differ, equal-bit NaNs are equal */
       S5GPU_DIFF_OFFSET = 16,
       S5GPU_DIFF_RANGE = 32,
       S5GPU_DIFF_SAMPLING_RATE = 64,
       S5GPU_DIFF_ID = 128,            /* id length or bytes differ; only compared when both sides bring their payloads            */
       S5GPU_DIFF_AUX = 256,           /* aux_len or an aux byte differs; only compared when both sides bring their payloads       */
       S5GPU_DIFF_FAILED = 0x4000,     /* either status is not 0, or (payloads given) a side's fields point outside its own payload slot: nothing
                                        * of the pair is loaded, every other member is 0, first_diff and max_at are 0xFFFFFFFF     */
       S5GPU_DIFF_BAD_PAIR = 0x8000 }; /* ia >= A.n or ib >= B.n: checked before anything is loaded through the index; every other member as
                                        * for FAILED                                                                               */
#define S5GPU_DIFF_NONE 0xFFFFFFFFu    /* first_diff / max_at: no such sample */
typedef struct s5gpu_sig_diff {        /* 80 bytes, little-endian, no padding */
    int32_t status_a, status_b;        /* the decoder's statuses                                      */
    uint32_t n_a, n_b;                 /* n_eff of each side                                          */
    uint32_t flags;                    /* S5GPU_DIFF_*                                                */
    uint32_t n_diff;                   /* count of d[i] != 0                                          */
    uint32_t first_diff;               /* smallest such i; S5GPU_DIFF_NONE when none                  */
    uint32_t max_abs;                  /* max of abs(d[i]): 0 .. 65535                                */
    uint32_t max_at;                   /* SMALLEST i reaching max_abs; S5GPU_DIFF_NONE when n_diff == 0 */
    uint32_t reserved;                 /* 0                                                           */
    int64_t sum_d;
    uint64_t sum_abs;
    uint64_t sum_sq;                   /* exact: d^2 < 2^32 and n < 2^32                              */
    int64_t sum_a;                     /* the sum of a[i] over i < n_cmp, for the SNR                 */
    uint64_t sumsq_a;                  /* the sum of a[i]^2 over i < n_cmp                            */
} s5gpu_sig_diff_t;
#define S5GPU_DIFF_BINS 131071
/* The file-wide accumulator: 1 048 696 bytes that stay in device memory and come back once.  The 64-bit sums WRAP; sum_sq cannot before 2^32
 * samples.  Every member is an integer sum, maximum or count: the result does not depend on the batches, their order or the launch shape. */
typedef struct s5gpu_diff_acc {
    uint64_t n_pairs;
    uint64_t n_failed;                 /* FAILED or BAD_PAIR                                                     */
    uint64_t n_differ;                 /* pairs that are not failed and whose flags are not 0                    */
    uint64_t n_signal, n_len;
    uint64_t n_fields;                 /* any of READ_GROUP .. SAMPLING_RATE                                     */
    uint64_t n_aux, n_id;
    uint64_t n_samples;                /* the sum of n_cmp                                                       */
    uint64_t n_diff;
    int64_t sum_d;
    uint64_t sum_abs, sum_sq;
    int64_t sum_a;
    uint64_t sumsq_a;
    uint32_t max_abs, reserved;
    uint64_t hist[S5GPU_DIFF_BINS];    /* samples with difference d at [d + 65535]                               */
} s5gpu_diff_acc_t;
/* One decoded batch as the kernel takes it: device arrays of n entries, as for s5gpu_signal_stats_dev (sig 16-byte aligned, every sig_off a
 * multiple of 8 samples).  payload (16-byte aligned) / pay_off / pay_cap: the payload slots of the full form of s5gpu_decode_dev; payload == NULL
 * on either side means that ID and AUX are not compared (and pay_off / pay_cap of that side are not read). */
typedef struct s5gpu_diff_side {
    uint32_t n;
    const int16_t *sig;
    const uint64_t *sig_off;
    const uint32_t *sig_cap;
    const s5gpu_rec_fields_t *fields;
    const uint8_t *payload;
    const uint64_t *pay_off;
    const uint32_t *pay_cap;
} s5gpu_diff_side_t;
/* Pair p = (pair_a[p], pair_b[p]) (device arrays of n_pairs u32) -> out[p] and, added with atomics, *acc; either of out (8-byte aligned) and acc
 * (8-byte aligned, reset by s5gpu_diff_acc_reset_dev) may be NULL.  Asynchronous on hip_stream.  The ID and AUX bytes are loaded only after
 * both ranges are shown to lie inside their own payload slots.  A workgroup counts the differences d != 0 inside a window of values around 0
 * in LDS and sends the others straight to acc->hist with 64-bit atomics; d == 0 is never counted sample by sample: bin 65535 receives
 * n_samples - n_diff.  s5gpu_set_option (tests, tools):
 *   "diff_lds_bins"      bins of the window [-bins/2, bins/2): 0 (every differing sample is a global atomic) or a power of two from 8 to 256
 *                        (default 64).  Changes the time, never the result.
 *   "diff_flush_samples" 1 .. 4294967295 (default): a workgroup empties its LDS counters before a pair would take the samples it has counted
 *                        since the last time past this number (no u32 counter can wrap).
 *   "diff_grid"          1 .. 1024 (default): the most workgroups of one launch; below the pair count a workgroup walks several pairs. */
size_t s5gpu_diff_acc_bytes(void);     /* sizeof(s5gpu_diff_acc_t) as the library was built */
int s5gpu_diff_acc_reset_dev(s5gpu_diff_acc_t *acc, void *hip_stream);
int s5gpu_signal_diff_dev(uint32_t n_pairs, const uint32_t *pair_a, const uint32_t *pair_b, const s5gpu_diff_side_t *A, const s5gpu_diff_side_t *B,
                          s5gpu_sig_diff_t *out, s5gpu_diff_acc_t *acc, void *hip_stream);
/* The per-file handle: it owns one accumulator and buffers for side A on the FIRST device in use (NULL + s5gpu_last_error() on failure).
 * add_batch: pair i is record i of each list (bytes without the u64 prefix, anywhere in host memory, as for s5gpu_digest_batch).  A is decoded
 * in full (payloads kept, so that aux and id can be compared) and its signal slab, payload slab, descriptors and fields are copied device to
 * device into the handle's buffers; then B is decoded in the same context, k_sig_diff runs and n x 80 bytes come back into out[] (may be NULL).
 * This costs one extra pass over A's decoded bytes; holding two contexts instead was not built.  status_a / status_b (may be NULL): the
 * decoder's statuses.  A corrupt record on either side fails the call with S5GPU_ERR_DATA: its pair is FAILED and counted in n_failed, the
 * other pairs are valid and the handle stays usable (the batch is decoded again without the corrupt records, at most three more times, as
 * s5gpu_file_stats_add_stream does).  close: the single download into *acc_out (may be NULL) and the end of the handle, whatever it returns.
 * Not built: SLOW5 text input, several devices per file. */
void *s5gpu_diff_open(void);
int s5gpu_diff_add_batch(void *h, uint32_t n, const void *const *rec_a, const size_t *len_a, int rec_a_method, int sig_a_method,
                         const void *const *rec_b, const size_t *len_b, int rec_b_method, int sig_b_method, s5gpu_sig_diff_t *out,
                         int32_t *status_a, int32_t *status_b);
int s5gpu_diff_close(void *h, s5gpu_diff_acc_t *acc_out);

/* ---- events: scrappie-style event segmentation of DECODED reads, on the device (docs/codecs.md §4.15) ----
 * A read of n = n_eff samples (the rule of "signals" above) is cut at the peaks of two sliding t-tests: windows w1 < w2 (1 .. 64), thresholds
 * thr1 / thr2 and a peak height, all finite.  The t-statistic is computed on the raw integers, sqrt(num / den) with integer num and den, so the
 * cut points are reproducible bit for bit; no equality with a float32 implementation is promised at ties.  DNA: 3, 6, 1.4, 9.0, 0.2;
 * RNA: 7, 14, 2.5, 9.0, 1.0.  A read with n > 0 has peaks + 1 events that tile [0, n); n = 0 has none. */
typedef struct s5gpu_event_params {
    uint32_t w1, w2;
    double thr1, thr2, peak_height;
} s5gpu_event_params_t;
typedef struct s5gpu_event {   /* 16 bytes, little-endian */
    uint32_t start;            /* first sample                                                                             */
    uint32_t length;           /* samples (>= 1)                                                                           */
    float mean;                /* S5GPU_NORM_RAW: float32(S / L) in double; S5GPU_NORM_PA: float32((S / L + offset) * (range / digitisation)) */
    float stdv;                /* float32(sqrt(max(Q / L - (S / L)^2, 0))), every operation rounded on its own; PA: times |range / digitisation| */
} s5gpu_event_t;
#define S5GPU_STATUS_EVENTS_OVERFLOW 17   /* ev_status[i]: the read has more events than its slot holds */
/* n records -> n_events[i] = the events of read i (always the number found), ev_status[i] = 0, the decoder's status of a failed record (no
 * events), or S5GPU_STATUS_EVENTS_OVERFLOW; rows [ev_off[i], ev_off[i] + min(n_events[i], ev_cap[i])) of `rows` (16-byte aligned) are written
 * and nothing else.  rows == NULL: the count pass, ev_off / ev_cap are not read.  mode: S5GPU_NORM_RAW or S5GPU_NORM_PA.  p: a HOST struct;
 * everything else device arrays of n entries.  S5GPU_ERR_ARG (nothing launched): w1 = 0, w1 >= w2, w2 > 64, a non-finite parameter, another
 * mode.  Asynchronous on hip_stream. */
int s5gpu_signal_events_dev(uint32_t n, const int16_t *sig, const uint64_t *sig_off, const uint32_t *sig_cap, const s5gpu_rec_fields_t *fields,
                            const s5gpu_event_params_t *p, int mode, const uint64_t *ev_off, const uint32_t *ev_cap, s5gpu_event_t *rows,
                            uint32_t *n_events, int32_t *ev_status, void *hip_stream);
/* The events of n records anywhere in host memory (bytes without the u64 prefix, as for s5gpu_digest_batch), on the FIRST device in use: one
 * upload, the decode, the count pass, an exclusive scan on the device, the fill pass, and the rows come back in one download (the n + 1 row
 * offsets, 8 bytes each, come back before it: the host has to know the room).  ev_first[i] .. ev_first[i + 1]: the rows of read i in
 * rows_out; rows_cap in rows.  Too little room: S5GPU_ERR_NOMEM and ev_first[0] = the rows needed.  A corrupt record fails the call with
 * S5GPU_ERR_DATA: its status_out[i] (may be NULL) is the decoder's and it has no rows; the other reads' events are valid. */
int s5gpu_signal_events_batch(uint32_t n, const void *const *rec, const size_t *rec_len, int rec_method, int sig_method,
                              const s5gpu_event_params_t *p, int mode, s5gpu_event_t *rows_out, size_t rows_cap, uint64_t *ev_first,
                              int32_t *status_out);

/* ---- map: subsequence DTW of each read's events against a reference squiggle, on the device (docs/codecs.md §4.16) ----
 * quant: float32 values m[0 .. L) -> int16.  In double, strictly left to right, every operation rounded on its own: mu = (sum m) / L,
 * sd = sqrt((sum (m - mu)^2) / L); L = 0, sd = 0 or sd not finite: every q = 0; else q[j] = clamp(rint(((m[j] - mu) / sd) * scale), -clip, clip),
 * round-half-even.  A read's QUERY is quant of the means (S5GPU_NORM_RAW: quant is invariant under a positive affine map up to rounding) of
 * its event rows [skip, skip + qlen), qlen = min(qmax, max(E - skip, 0)); qlen < qmin: no query, qlen = 0, S5GPU_STATUS_QUERY_SHORT.
 * sDTW, exact in integers: c(i,j) = |q[i] - r[j]|, D[0][j] = c(0,j) (the start is free), D[i][0] = D[i-1][0] + c(i,0), else
 * D[i][j] = c(i,j) + min(D[i-1][j-1], D[i-1][j], D[i][j-1]); D[i][j] <= 65535 (i + 1) < 2^26 for qlen <= 1024, so uint32 holds it for any R.
 * cost = min_j D[qlen-1][j], end = the smallest such j; start (want_start) = the column in row 0 of the path to (qlen-1, end) that takes at
 * every cell the predecessor of least D, ties to the diagonal, then (i-1, j), then (i, j-1). */
typedef struct s5gpu_map_params {
    uint32_t skip;             /* event rows left out in front (adaptor, stall)                 */
    uint32_t qmax;             /* 1 .. 1024: rows of the query at most, and the query matrix's pitch */
    uint32_t qmin;             /* 1 .. qmax: a read with fewer rows after skip has no query     */
    double scale;              /* finite, > 0; 32.0                                             */
    int32_t clip;              /* 1 .. 32767; 127                                               */
    int32_t want_start;        /* != 0: the row's start is computed                             */
} s5gpu_map_params_t;
typedef struct s5gpu_map_row {  /* 16 bytes, little-endian */
    uint32_t cost;             /* 0xFFFFFFFF: the read has no query                             */
    uint32_t qlen;             /* event rows used                                               */
    int32_t start;             /* first reference index of the path; -1: not asked for, or no query */
    int32_t end;               /* last reference index of the path (inclusive); -1: no query    */
} s5gpu_map_row_t;
#define S5GPU_STATUS_QUERY_SHORT 18   /* status[i]: fewer than qmin event rows behind skip */
/* quant on the host (the same header function the kernel runs, compiled without contraction): for the reference.  S5GPU_ERR_ARG: scale
 * not finite or <= 0, clip outside 1 .. 32767, a NULL pointer with L > 0. */
int s5gpu_quantise_host(const float *m, size_t L, double scale, int32_t clip, int16_t *q);
/* The queries of n reads from their event rows as s5gpu_signal_events_dev / the scan left them: rows, first (n + 1 entries: the rows of read i
 * are rows[first[i] .. first[i + 1])) and ev_status (may be NULL: all 0).  queries: [n, p->qmax] int16, row i = the query of read i and zeros
 * behind qlen[i]; status[i] = ev_status[i] when that is not 0 (no query: a failed record, an overflowed slot), else 0 or
 * S5GPU_STATUS_QUERY_SHORT.  p: a HOST struct (want_start is not read); everything else device arrays.  S5GPU_ERR_ARG (nothing launched):
 * qmax = 0 or > 1024, qmin = 0 or > qmax, scale not finite or <= 0, clip outside 1 .. 32767, a NULL or misaligned pointer.  Asynchronous. */
int s5gpu_event_queries_dev(uint32_t n, const s5gpu_event_t *rows, const uint64_t *first, const int32_t *ev_status, const s5gpu_map_params_t *p,
                            int16_t *queries, uint32_t *qlen, int32_t *status, void *hip_stream);
/* sDTW of n queries (row i of `queries`, pitch qpitch <= 1024 values, its first min(qlen[i], qpitch) values) against ref[0 .. R), a device
 * int16 array, 1 <= R <= 2^31 - 1: out_rows[i] (16-byte aligned) is written for every i and nothing else; qlen[i] = 0: the empty row
 * 0xFFFFFFFF, 0, -1, -1.  One wave per read; the reference is not split, so few reads against a very long reference is not this call's case.
 * S5GPU_ERR_ARG (nothing launched): qpitch = 0 or > 1024, R = 0 or > 2^31 - 1, a NULL or misaligned pointer.  Asynchronous on hip_stream. */
int s5gpu_sdtw_dev(uint32_t n, const int16_t *queries, uint32_t qpitch, const uint32_t *qlen, const int16_t *ref, uint32_t R, int want_start,
                   s5gpu_map_row_t *out_rows, void *hip_stream);
/* n records anywhere in host memory (bytes without the u64 prefix) against the quantised reference ref_host[0 .. R) (HOST memory), on the FIRST
 * device in use: the decode, the event passes (event_params, S5GPU_NORM_RAW), the queries, sDTW, and one download of 16 n bytes into
 * rows_out[0 .. n).  status_out[i] (may be NULL): 0, S5GPU_STATUS_QUERY_SHORT or the decoder's.  A corrupt record fails the call with
 * S5GPU_ERR_DATA: its status_out[i] is the decoder's and its row is the empty row; the other reads' rows are valid.  S5GPU_ERR_ARG before
 * anything is launched: the cases of the two calls above and of s5gpu_signal_events_dev, an unsupported method. */
int s5gpu_map_batch(uint32_t n, const void *const *rec, const size_t *rec_len, int rec_method, int sig_method,
                    const s5gpu_event_params_t *event_params, const s5gpu_map_params_t *map_params, const int16_t *ref_host, uint32_t R,
                    s5gpu_map_row_t *rows_out, int32_t *status_out);

/* ---- map, the second-best hit and a mapping quality (docs/codecs.md §4.19) ----
 * L[j] = D[qlen-1][j], (cost, end) as above.  Column j lies in block j >> bshift, bshift in 6 .. 30.  cost2 = the minimum of L[j] over the columns
 * whose block differs from end's block by at least 2 (the best hit's block and both neighbours are excluded: the same hit shifted by a few
 * columns is no runner-up), end2 the smallest such j; no such column: 0xFFFFFFFF and -1.  mapq = 0 when cost2 is 0xFFFFFFFF or 0, else
 * (60 (cost2 - cost)) / cost2 in integer division, 0 .. 60: a separation ratio, not a calibrated probability. */
typedef struct s5gpu_map_second {  /* 16 bytes, little-endian */
    uint32_t cost2;            /* 0xFFFFFFFF: no runner-up (or no query)                        */
    int32_t end2;              /* last reference index of the runner-up (inclusive); -1: none   */
    uint32_t mapq;             /* 0 .. 60                                                       */
    uint32_t zero;
} s5gpu_map_second_t;
/* s5gpu_sdtw_dev, and out_second[i] (16-byte aligned) beside out_rows[i], which is bit for bit what s5gpu_sdtw_dev writes; qlen[i] = 0:
 * 0xFFFFFFFF, -1, 0, 0.  One pass over the reference.  S5GPU_ERR_ARG (nothing launched): the cases of s5gpu_sdtw_dev, bshift outside 6 .. 30,
 * a NULL or misaligned out_second. */
int s5gpu_sdtw2_dev(uint32_t n, const int16_t *queries, uint32_t qpitch, const uint32_t *qlen, const int16_t *ref, uint32_t R, int want_start,
                    uint32_t bshift, s5gpu_map_row_t *out_rows, s5gpu_map_second_t *out_second, void *hip_stream);
/* s5gpu_map_batch with the second-best hit: one download of 32 n bytes; second_out[i] of a read without a query or of a dropped record is
 * 0xFFFFFFFF, -1, 0, 0.  S5GPU_ERR_ARG before anything is launched: the cases of s5gpu_map_batch, bshift outside 6 .. 30, a NULL second_out. */
int s5gpu_map2_batch(uint32_t n, const void *const *rec, const size_t *rec_len, int rec_method, int sig_method,
                     const s5gpu_event_params_t *event_params, const s5gpu_map_params_t *map_params, const int16_t *ref_host, uint32_t R,
                     uint32_t bshift, s5gpu_map_row_t *rows_out, s5gpu_map_second_t *second_out, int32_t *status_out);

/* ---- a reference squiggle from sequences and a k-mer model, on the host (docs/codecs.md §4.19; no device is needed) ----
 * Model: 4^k float levels, k in 1 .. 10, indexed by the k-mer's rank in base 4 (A, C, G, T = 0 .. 3, the first base most significant).  A contig
 * of L >= k bases has Lk = L - k + 1 levels, lev[p] = the level of seq[p .. p + k); a k-mer that holds any other letter takes the table's mean
 * (the double sum in rank order, divided, rounded to float).  Bases are read without case, U as T.  Segments, in this order per contig:
 * the forward levels, then (strands = 2) the levels of the reverse complement, whose column p' is forward k-mer start Lk - 1 - p'; rna != 0: one
 * segment, the forward levels in reversed order (strands is not read).  A contig shorter than k has no segment.  All segments' levels are
 * quantised together (s5gpu_quantise_host(scale, clip)); between consecutive segments stand W = (2048 clip) / (32768 - clip) + 1 columns of
 * -32768, which no best path of a query within +-clip of at most 1024 rows touches, so a hit's start and end lie in one segment. */
typedef struct s5gpu_refseq_segment {
    uint32_t contig;           /* index of the contig                                           */
    int32_t strand;            /* '+' or '-'                                                    */
    uint32_t offset;           /* the segment's first column in the reference                   */
    uint32_t Lk;               /* its columns                                                   */
    int32_t reversed;          /* != 0: column p' is forward k-mer start Lk - 1 - p'            */
    uint32_t zero;
    const char *name;          /* the contig's name (the handle's: valid until it is closed)    */
} s5gpu_refseq_segment_t;
typedef struct s5gpu_refseq_loc {  /* 16 bytes */
    uint32_t contig;           /* 0xFFFFFFFF: a wall column                                     */
    int32_t strand;            /* '+' or '-'; 0: a wall column                                  */
    uint32_t pos;              /* 0-based start of the column's k-mer on the forward strand     */
    uint32_t segment;          /* the segment; for a wall column the one in front of it         */
} s5gpu_refseq_loc_t;
#define S5GPU_REFSEQ_WALL 1      /* s5gpu_refseq_locate: the column is a wall column */
/* The levels of a model file -> *levels_out (4^k floats, to be freed with s5gpu_kmer_model_free) and *k_out.  One line per k-mer: the k-mer
 * (ACGT), a tab or spaces, level_mean in strtod syntax; further columns are ignored; empty lines and lines that start with '#' or "kmer" are
 * skipped.  S5GPU_ERR_ARG: the file cannot be read; S5GPU_ERR_DATA: a line that is neither, k-mers of different lengths or of k outside
 * 1 .. 10, a k-mer twice, or not every one of the 4^k there. */
int s5gpu_kmer_model_load(const char *path, float **levels_out, uint32_t *k_out);
void s5gpu_kmer_model_free(float *levels);
/* A reference from n_contigs sequences in memory (seqs[i]: lens[i] bytes, no terminator needed; names[i]: a C string).  NULL
 * (s5gpu_last_error says why): a NULL argument, k outside 1 .. 10, strands not 1 or 2, the cases of s5gpu_quantise_host, W > 64, no contig
 * of k or more bases, more than 2^31 - 1 columns. */
void *s5gpu_refseq_build(uint32_t n_contigs, const char *const *names, const char *const *seqs, const size_t *lens, const float *model_levels,
                         uint32_t k, int strands, int rna, double scale, int32_t clip);
/* ... from a FASTA file (>name up to the first white space; the sequence may span lines) and a model file.  NULL also for an unreadable
 * file, a FASTA without a '>' line or with sequence in front of the first, and the cases of s5gpu_kmer_model_load. */
void *s5gpu_refseq_open(const char *fasta_path, const char *model_path, int strands, int rna, double scale, int32_t clip);
const int16_t *s5gpu_refseq_ref(const void *h, uint32_t *R_out);            /* the quantised reference with its walls; the handle's */
uint32_t s5gpu_refseq_n_segments(const void *h);
int s5gpu_refseq_segment(const void *h, uint32_t i, s5gpu_refseq_segment_t *info);     /* S5GPU_ERR_ARG: i is no segment */
uint32_t s5gpu_refseq_n_contigs(const void *h);
/* contig i as it was given: its name, its bases and its levels (0: shorter than k, no segment); any output may be NULL */
int s5gpu_refseq_contig(const void *h, uint32_t i, const char **name_out, uint64_t *len_out, uint32_t *Lk_out);
/* k, the wall width W and the clip the reference was built with (a map call has to use the same clip: the wall argument needs it) */
int s5gpu_refseq_params(const void *h, uint32_t *k_out, uint32_t *W_out, int32_t *clip_out);
/* reference column -> contig, strand, forward k-mer start: S5GPU_OK; S5GPU_REFSEQ_WALL for a wall column; S5GPU_ERR_ARG: col >= R */
int s5gpu_refseq_locate(const void *h, uint32_t col, s5gpu_refseq_loc_t *loc);
void s5gpu_refseq_close(void *h);

/* ---- align: the whole path of a read's sDTW alignment, event to reference (docs/codecs.md §4.17) ----
 * The path of a read starts at (qlen - 1, end) and follows the chosen predecessor (the rule of map) to row 0, where it arrives at (0, start).
 * It is monotone, so two values per query row i describe it: lo[i] <= hi[i], the first and last reference column that event i is aligned
 * to.  lo[0] = start, hi[qlen - 1] = end, lo[i] - hi[i - 1] is 0 or 1, and the c(i,j) of all its cells add up to cost.  lo and hi are
 * [n, qpitch] int32 matrices, -1 behind qlen and in every row of a read without a path. */
#define S5GPU_STATUS_PATH_WIDE 19     /* status[i]: the span end - start + 1 is above wmax: no path */
#define S5GPU_STATUS_PATH_ROW 20      /* status[i]: the read has a query but its row is unusable: start < 0 (made without want_start),
                                         start > end, end >= R, a qlen that is not the query's, or decisions that do not lead to (0, start) */
/* The scratch bytes one read needs in s5gpu_sdtw_path_dev: 2 bits per cell of its 64 lanes over wmax + 63 steps; 0 for a qpitch or wmax that
 * call refuses.  Monotone in both arguments. */
size_t s5gpu_sdtw_path_slot_bytes(uint32_t qpitch, uint32_t wmax);
/* The paths of n reads: queries, qpitch, qlen, ref, R as for s5gpu_sdtw_dev, and rows = what that call wrote with want_start, all DEVICE
 * arrays.  The recurrence is run again over the columns [start, end] of each read only, its decisions are kept in `scratch` and walked
 * back.  wmax (1 .. 2^20): the widest span that gets a path; it bounds the scratch, not the quality.  lo, hi ([n, qpitch]) and status ([n]:
 * 0, S5GPU_STATUS_PATH_WIDE or S5GPU_STATUS_PATH_ROW; a read with qlen = 0 has 0 and no path) are written, and nothing else outside the
 * scratch.  Reads are handled in groups of scratch_bytes / slot reads, one after the other on the stream.  S5GPU_ERR_NOMEM: the scratch is
 * smaller than one slot.  S5GPU_ERR_ARG (nothing launched): the cases of s5gpu_sdtw_dev, wmax = 0 or > 2^20, a NULL or misaligned pointer
 * (scratch: 16 bytes; rows: 16; lo, hi, status: 4).  Asynchronous on hip_stream.
 * s5gpu_set_option (tests, tools): "sdtw_path_passes" (1 .. 3, default 3): 1 launches the pass that writes the decisions only, 2 the walk
 * only (over what an earlier call left in the scratch and the outputs); tools/sdtw_path_time.py times the passes apart with it. */
int s5gpu_sdtw_path_dev(uint32_t n, const int16_t *queries, uint32_t qpitch, const uint32_t *qlen, const int16_t *ref, uint32_t R,
                        const s5gpu_map_row_t *rows, uint32_t wmax, void *scratch, size_t scratch_bytes, int32_t *lo, int32_t *hi,
                        int32_t *status, void *hip_stream);
/* s5gpu_map_batch with want_start forced on, then the paths, on the FIRST device in use; one download brings back rows_out[0 .. n),
 * lo_out and hi_out ([n, qmax] int32) and events_out (may be NULL; [n, qmax]: the event rows [skip, skip + qlen) of the read's query, zeros
 * behind qlen).  The scratch is at most 256 MiB (one slot above that: S5GPU_ERR_NOMEM).  status_out[i] (may be NULL): the decoder's,
 * S5GPU_STATUS_QUERY_SHORT, S5GPU_STATUS_PATH_WIDE, S5GPU_STATUS_PATH_ROW or 0.  A corrupt record fails the call with S5GPU_ERR_DATA: its
 * status is the decoder's, its row the empty row, its lo and hi -1 and its events zero; the other reads are valid.  S5GPU_ERR_ARG before
 * anything is launched: the cases of s5gpu_map_batch, wmax = 0 or > 2^20. */
int s5gpu_align_batch(uint32_t n, const void *const *rec, const size_t *rec_len, int rec_method, int sig_method,
                      const s5gpu_event_params_t *event_params, const s5gpu_map_params_t *map_params, uint32_t wmax, const int16_t *ref_host,
                      uint32_t R, s5gpu_map_row_t *rows_out, int32_t *lo_out, int32_t *hi_out, s5gpu_event_t *events_out, int32_t *status_out);

/* ---- pileup: per-reference-position statistics of aligned events, accumulated on the device (docs/codecs.md §4.18) ----
 * The transpose of align: what the reads say about reference column j.  Inputs are those of s5gpu_sdtw_path_dev and what it wrote: queries,
 * qlen (Q = min(qlen[i], qpitch)), ref, lo, hi, status, and optionally the query's event rows as an [n, qpitch] matrix.  A read is USED iff
 * status = 0, Q >= 1, every row i < Q has 0 <= lo[i] <= hi[i] < R and every row 1 <= i < Q has lo[i] - hi[i-1] in {0, 1}; status != 0 or
 * Q = 0: SKIPPED; a failed row check: BAD, and nothing of the read is accumulated.  The cells of a used read are (i, j), i < Q,
 * lo[i] <= j <= hi[i]; a cell is first in its column iff i = 0 or j > hi[i-1].  Every member is an integer sum, minimum or maximum over
 * all used reads, so the result does not depend on the order of reads, batches, streams or atomics. */
typedef struct s5gpu_pile_col {  /* 48 bytes, little-endian: column j of the table */
    uint32_t depth;            /* cells that are first in their column: the reads with start <= j <= end */
    uint32_t n_events;         /* cells in the column (fewer than 2^32)                         */
    uint64_t n_samples;        /* sum of events[i].length; 0 when no events are given; an event that spans several columns counts in each */
    int64_t sum_q;             /* sum of q[i]                                                   */
    uint64_t sumsq_q;          /* sum of q[i]^2                                                 */
    uint64_t sum_cost;         /* sum of |q[i] - r[j]|                                          */
    int32_t min_q, max_q;      /* 32767 / -32768 while the column is empty                      */
} s5gpu_pile_col_t;
typedef struct s5gpu_pile_total {  /* 64 bytes in front of the columns */
    uint64_t reads_used, reads_skipped, reads_bad;
    uint64_t cells;            /* = sum of n_events over the columns                            */
    uint64_t cost;             /* = sum of sum_cost over the columns; for paths of s5gpu_sdtw_path_dev the sum of the rows' cost */
    uint32_t R;
    uint32_t reserved[5];
} s5gpu_pile_total_t;
/* 64 + 48 R: the bytes of an accumulator of R columns; 0 for R = 0 or R > 2^26 */
size_t s5gpu_pileup_bytes(uint32_t R);
/* Writes the empty accumulator (zeros, the 32767 / -32768 pairs, R) to acc (DEVICE memory, 16-byte aligned, s5gpu_pileup_bytes(R)).
 * S5GPU_ERR_ARG (nothing launched): R = 0 or > 2^26, a NULL or misaligned acc.  Asynchronous on hip_stream. */
int s5gpu_pileup_reset_dev(void *acc, uint32_t R, void *hip_stream);
/* Adds n reads to acc, which s5gpu_pileup_reset_dev wrote for the same R, and writes nothing else; all pointers DEVICE memory.  Calls on
 * one acc may run on several streams at once.  n = 0: S5GPU_OK, nothing launched.  S5GPU_ERR_ARG (nothing launched): qpitch = 0 or
 * > 1024, R = 0 or > 2^26, a NULL pointer (events may be NULL) or a misaligned one (acc, events: 16 bytes; qlen, lo, hi, status: 4).
 * Asynchronous on hip_stream.
 * s5gpu_set_option (tests, tools): "pileup_lds_cols" (0, or a power of two 64 .. 1024; default 1024): the columns a workgroup keeps in LDS
 * (0: every cell is a global atomic); "pileup_grid" (1 .. 1024, default 1024): the most workgroups of one launch.  Neither changes the result. */
int s5gpu_pileup_accum_dev(uint32_t n, const int16_t *queries, uint32_t qpitch, const uint32_t *qlen, const int16_t *ref, uint32_t R,
                           const int32_t *lo, const int32_t *hi, const int32_t *status, const s5gpu_event_t *events, void *acc, void *hip_stream);
/* The per-file handle: an accumulator of R columns on the FIRST device in use and the parameters of the chain.  ref_host[0 .. R) (HOST
 * memory) is copied.  NULL (s5gpu_last_error says why): the S5GPU_ERR_ARG cases of s5gpu_align_batch, R > 2^26, a read's scratch above
 * 256 MiB, no device, no memory. */
void *s5gpu_pileup_open(const s5gpu_event_params_t *event_params, const s5gpu_map_params_t *map_params, uint32_t wmax, const int16_t *ref_host,
                        uint32_t R);
/* The chain of s5gpu_align_batch on n records, then their cells added to the handle's accumulator; lo and hi never leave the device:
 * rows_out[0 .. n) (may be NULL) and status_out[0 .. n) (may be NULL) are all that comes back.  A record that is not used counts in
 * reads_skipped or reads_bad.  A corrupt record makes the call return S5GPU_ERR_DATA: its status is the decoder's, the other reads are
 * accumulated and the handle stays usable. */
int s5gpu_pileup_add_batch(void *handle, uint32_t n, const void *const *rec, const size_t *rec_len, int rec_method, int sig_method,
                           s5gpu_map_row_t *rows_out, int32_t *status_out);
/* Downloads the accumulator to acc_out (HOST memory, s5gpu_pileup_bytes(R); may be NULL) and ends the handle, whatever it returns. */
int s5gpu_pileup_close(void *handle, void *acc_out);

/* ---- refine: per-read level rescaling from the path, and a windowed realign (docs/codecs.md §4.20) ----
 * The query of a read and the reference were normalised apart (§4.16).  refine fits the line r = a q + b by least squares over the cells
 * (i, j), lo[i] <= j <= hi[i], of the read's path, requantises the query q'[i] = clamp(rint(a q[i] + b), -clip, clip), and aligns q' again
 * in the window [start - pad, end + pad] of the reference (clipped to [0, R - 1]), `iters` times, each round from the query that came in and
 * along the path of the round before.  The reference stays as it is, so costs before and after compare.  Everything is reproducible bit
 * for bit: the sums are exact integers, the solve is in double with every operation rounded on its own (§4.20 gives the order). */
#define S5GPU_STATUS_FIT_FLAT 21      /* status[i]: fewer than min_cells cells, or a query without variance along the path: no fit */
#define S5GPU_STATUS_FIT_RANGE 22     /* status[i]: the slope is not finite or outside [a_min, a_max], or |b| > b_max: the fit is refused */
typedef struct s5gpu_refine_params {  /* 40 bytes */
    double a_min, a_max;       /* the slopes that are accepted: finite, 0 < a_min <= a_max; 0.5 and 2.0 */
    double b_max;              /* the largest |b| that is accepted: finite, >= 0; 64.0                   */
    int32_t clip;              /* q' is clamped to +-clip: 1 .. 32767; 127                               */
    uint32_t pad;              /* columns added on either side of [start, end]: 0 .. 65535; 16           */
    uint32_t min_cells;        /* the fewest cells that are fitted: >= 2; 16                             */
    uint32_t iters;            /* rounds of s5gpu_refine_dev and s5gpu_refine_batch: 1 .. 4; 2           */
} s5gpu_refine_params_t;
typedef struct s5gpu_fit {     /* 64 bytes */
    double a, b;               /* 1 and 0 where the read was not fitted or the fit was refused */
    int64_t n, sq, sr, sqq, sqr, srr;   /* the cells, and the sums of q, r, q^2, q r, r^2 over them; 0 where the read has no path to fit */
} s5gpu_fit_t;
/* The fit of n reads along their paths: queries, qpitch, qlen, ref, R, lo, hi as s5gpu_sdtw_path_dev took and left them, status_in what it
 * wrote (or any caller's: a read whose status_in is not 0 is passed over and keeps it), all DEVICE arrays; params a HOST struct (pad and
 * iters are checked, not used).  A read is fitted iff status_in = 0, it has a query, every row passes the rules of s5gpu_pileup_accum_dev
 * (else S5GPU_STATUS_PATH_ROW) and the path spans at most wmax columns (else S5GPU_STATUS_PATH_WIDE).  fit_out[i]: a, b and the sums;
 * queries_out (may be NULL; [n, qpitch]): q', zeros behind qlen; status_out[i]: 0, S5GPU_STATUS_FIT_FLAT or S5GPU_STATUS_FIT_RANGE (a = 1,
 * b = 0, the sums as they are, and q' a copy of q), or the status of a read that was not fitted (a = 1, b = 0, sums 0, q' zeros).  Nothing
 * else is written.  n = 0: S5GPU_OK, nothing launched.  S5GPU_ERR_ARG (nothing launched): the cases of s5gpu_sdtw_path_dev, a parameter
 * outside its range, a NULL or misaligned pointer (fit_out: 16 bytes; lo, hi, the statuses: 4; queries: 2).  Asynchronous on hip_stream. */
int s5gpu_path_fit_dev(uint32_t n, const int16_t *queries, uint32_t qpitch, const uint32_t *qlen, const int16_t *ref, uint32_t R, const int32_t *lo,
                       const int32_t *hi, const int32_t *status_in, uint32_t wmax, const s5gpu_refine_params_t *params, s5gpu_fit_t *fit_out,
                       int16_t *queries_out, int32_t *status_out, void *hip_stream);
/* sDTW and its path in one call, in a window of the reference around a row that is known: for each read with a query, ws = max(0, start -
 * pad), we = min(R - 1, end + pad) of rows_in[i]; rows_out[i] = (cost', qlen, start', end') and lo, hi are §4.16's alignment and §4.17's path
 * of the query against r[ws .. we] (a free start anywhere in it, the smallest column of least cost as the end), in absolute columns.
 * status[i]: 0; S5GPU_STATUS_PATH_ROW (rows_in[i] is unusable, as in s5gpu_sdtw_path_dev); S5GPU_STATUS_PATH_WIDE (we - ws + 1 > wmax).  A
 * read with another status than 0, or without a query (status 0), has the empty row (0xFFFFFFFF, 0, -1, -1) and -1 in lo and hi.  scratch,
 * scratch_bytes and the groups as in s5gpu_sdtw_path_dev (slots of s5gpu_sdtw_path_slot_bytes(qpitch, wmax)); rows_out must not be
 * rows_in.  S5GPU_ERR_ARG (nothing launched): the cases of s5gpu_sdtw_path_dev, pad > 65535.  Asynchronous on hip_stream. */
int s5gpu_sdtw_window_dev(uint32_t n, const int16_t *queries, uint32_t qpitch, const uint32_t *qlen, const int16_t *ref, uint32_t R,
                          const s5gpu_map_row_t *rows_in, uint32_t pad, uint32_t wmax, void *scratch, size_t scratch_bytes,
                          s5gpu_map_row_t *rows_out, int32_t *lo, int32_t *hi, int32_t *status, void *hip_stream);
/* The bytes of `work` that s5gpu_refine_dev needs for n reads of pitch qpitch (a trial round's query, row, path, fit and statuses); 0 for
 * a qpitch the call refuses. */
size_t s5gpu_refine_work_bytes(uint32_t n, uint32_t qpitch);
/* params->iters rounds of the two calls above on DEVICE buffers; nothing comes to the host in between.  Round k + 1 fits the query that came
 * in along the path of round k (round 0: lo_in, hi_in), requantises from the query that came in, and realigns in the window around round
 * k's row (round 0: rows_in).  A round succeeds for a read when the fit is accepted and the window is at most wmax wide; its outputs then
 * become the round's.  A read that fails a round (S5GPU_STATUS_FIT_FLAT, S5GPU_STATUS_FIT_RANGE, S5GPU_STATUS_PATH_WIDE) keeps the outputs
 * of the last round that succeeded (none yet: copies of what came in, a = 1, b = 0), takes no further part, and has that status;
 * rounds_out[i]: the rounds that succeeded.  A read with status_in != 0, without a query, or whose lo_in, hi_in do not pass
 * s5gpu_path_fit_dev's checks has zeros in queries_out, the empty row, -1 in lo_out and hi_out, a = 1, b = 0, 0 rounds, and status_in or that
 * check's status.  What comes out feeds s5gpu_pileup_accum_dev as it is.  work: s5gpu_refine_work_bytes(n, qpitch) bytes, 16-byte
 * aligned; no output may be an input.  S5GPU_ERR_ARG (nothing launched): the cases of the two calls above.  Asynchronous on hip_stream. */
int s5gpu_refine_dev(uint32_t n, const int16_t *queries, uint32_t qpitch, const uint32_t *qlen, const int16_t *ref, uint32_t R,
                     const s5gpu_map_row_t *rows_in, const int32_t *lo_in, const int32_t *hi_in, const int32_t *status_in, uint32_t wmax,
                     const s5gpu_refine_params_t *params, void *scratch, size_t scratch_bytes, void *work, size_t work_bytes, int16_t *queries_out,
                     s5gpu_map_row_t *rows_out, int32_t *lo_out, int32_t *hi_out, s5gpu_fit_t *fit_out, int32_t *status_out, uint32_t *rounds_out,
                     void *hip_stream);
/* The chain of s5gpu_align_batch, then s5gpu_refine_dev, on the FIRST device in use; one download brings back rows_out[0 .. n) (the first
 * mapping), rows_refined_out[0 .. n), fit_out[0 .. n), lo_out and hi_out ([n, qmax]: the refined path), events_out (may be NULL) as in
 * s5gpu_align_batch, status_out (may be NULL: the statuses of s5gpu_align_batch, S5GPU_STATUS_FIT_FLAT, S5GPU_STATUS_FIT_RANGE) and
 * rounds_out (may be NULL).  A corrupt record: as in s5gpu_align_batch, its refined row the empty row and its fit a = 1, b = 0.
 * S5GPU_ERR_ARG before anything is launched: the cases of s5gpu_align_batch, a refine parameter outside its range, a NULL output. */
int s5gpu_refine_batch(uint32_t n, const void *const *rec, const size_t *rec_len, int rec_method, int sig_method,
                       const s5gpu_event_params_t *event_params, const s5gpu_map_params_t *map_params, uint32_t wmax,
                       const s5gpu_refine_params_t *refine_params, const int16_t *ref_host, uint32_t R, s5gpu_map_row_t *rows_out,
                       s5gpu_map_row_t *rows_refined_out, s5gpu_fit_t *fit_out, int32_t *lo_out, int32_t *hi_out, s5gpu_event_t *events_out,
                       int32_t *status_out, uint32_t *rounds_out);

/* ---- extend: whole-read banded alignment in tiles from a known anchor (docs/codecs.md §4.21) ----
 * map, align and refine stop at the first 1024 events of a read.  extend follows the path of ALL of a read's events (up to 2^20) from the
 * column where its prefix mapped: the query is cut into tiles of tile_rows rows, each tile is §4.16's recurrence over a window of `band`
 * reference columns, the window of the next tile is placed around the column where this tile's last row is cheapest, and the last row is
 * carried into the next tile less its minimum.  The cost is O(events x band) whatever R is.  The band is a heuristic: where the true path
 * leaves it the result is a worse alignment, not an error; cost / qlen is the only sign.  Integer throughout, reproducible bit for bit. */
typedef struct s5gpu_band_params {    /* 32 bytes */
    uint32_t skip;             /* event rows passed over at the head of a read: >= 0                          */
    uint32_t emin, emax;       /* the fewest rows that make a query, and the most that are used: 1 <= emin <= emax <= 2^20 */
    uint32_t tile_rows;        /* rows of a tile: 64, 128, 256, 512 or 1024; 256                              */
    uint32_t band;             /* columns of a tile's window: a multiple of 64 in 64 .. 4096; 512             */
    int32_t clip;              /* as in s5gpu_map_params_t: 1 .. 32767                                         */
    double scale;              /* as in s5gpu_map_params_t: finite, > 0                                        */
} s5gpu_band_params_t;
typedef struct s5gpu_ext_row {        /* 32 bytes; a read without a path: ~0, 0, 0, -1, -1, -1, status */
    uint64_t cost;             /* the sum of |q - r| over the cells of the path                                */
    uint32_t qlen, tiles;      /* the rows of the query, and its tiles                                         */
    int32_t start, end;        /* the columns of the path in row 0 and in row qlen - 1                         */
    int32_t a_last;            /* the first column of the last tile's window                                   */
    int32_t status;            /* 0, the status that came in, or S5GPU_STATUS_PATH_ROW                         */
} s5gpu_ext_row_t;
/* The long queries of n reads from their event rows: Q_i = min(emax, max(E_i - skip, 0)) with E_i = first[i + 1] - first[i]; Q_i < emin: no
 * query, qlen = 0, S5GPU_STATUS_QUERY_SHORT; a read whose ev_status (may be NULL) is not 0 has no query and keeps that status.  The query is
 * §4.16's quant of the means of rows [skip, skip + Q_i) and lives at queries[first[i] .. first[i] + Q_i), zeros behind it up to
 * first[i + 1]: the layout is ragged, `first` (n + 1 entries, as s5gpu_signal_events_dev leaves it) is its index, total_rows the length of
 * `queries`.  A read whose rows do not lie in [0, total_rows) is treated as one without rows.  params: a HOST struct (tile_rows and band
 * are checked, not used); everything else DEVICE arrays.  S5GPU_ERR_ARG (nothing launched): a parameter outside its range, a NULL or
 * misaligned pointer (rows: 16 bytes).  n = 0: S5GPU_OK.  Asynchronous on hip_stream. */
int s5gpu_event_queries_long_dev(uint32_t n, const s5gpu_event_t *rows, const uint64_t *first, const int32_t *ev_status,
                                 const s5gpu_band_params_t *params, uint64_t total_rows, int16_t *queries, uint32_t *qlen, int32_t *status,
                                 void *hip_stream);
/* The scratch s5gpu_sdtw_band_dev needs for n reads of total_rows rows in all: floor(total_rows / tile_rows) + n slots of
 * s5gpu_sdtw_path_slot_bytes(tile_rows, band), and 4 bytes a slot (rounded up to 16) for the tiles' first columns.  0 for a tile_rows or a
 * band the call refuses. */
size_t s5gpu_sdtw_band_scratch_bytes(uint32_t n, uint64_t total_rows, uint32_t tile_rows, uint32_t band);
/* The banded alignment of n long queries (queries, first, qlen, total_rows as s5gpu_event_queries_long_dev left them) against ref[0 .. R)
 * from anchor[i], a column 0 <= anchor[i] < R (in the chain: `start` of the read's prefix mapping made with the same skip).  rows_out[i]:
 * the result row; lo, hi ([total_rows], at first[i] as the query): the first and last column of every row of the path, -1 behind qlen up to
 * first[i + 1].  A read whose status_in is not 0 has no path and that status; one with a query whose anchor is out of range, or whose walk
 * fails, S5GPU_STATUS_PATH_ROW; one without a query and with status 0 has the empty row with status 0.  All reads are handled in one group:
 * scratch (16-byte aligned) has at least s5gpu_sdtw_band_scratch_bytes(n, total_rows, tile_rows, band) bytes, else S5GPU_ERR_NOMEM and
 * nothing is written.  Nothing but rows_out, lo, hi and the scratch is written.  params: a HOST struct (only tile_rows and band are used).
 * S5GPU_ERR_ARG (nothing launched): a parameter outside its range, R outside 1 .. 2^31 - 1, a NULL or misaligned pointer (rows_out,
 * scratch: 16 bytes; first: 8).  n = 0: S5GPU_OK.  Asynchronous on hip_stream.
 * s5gpu_set_option (tests, tools): "sdtw_band_passes" (1 .. 3, default 3): 1 launches k_sdtw_band only, 2 the walk only, over what an
 * earlier call left in the scratch and in rows_out. */
int s5gpu_sdtw_band_dev(uint32_t n, const int16_t *queries, const uint64_t *first, const uint32_t *qlen, uint64_t total_rows, const int16_t *ref,
                        uint32_t R, const int32_t *anchor, const int32_t *status_in, const s5gpu_band_params_t *params, void *scratch,
                        size_t scratch_bytes, s5gpu_ext_row_t *rows_out, int32_t *lo, int32_t *hi, void *hip_stream);
/* The chain on the FIRST device in use: the front of s5gpu_map_batch (map_params->want_start is taken as on), sDTW of the prefix query, the
 * long queries from the event rows that are resident already (a read is segmented once), the banded alignment from anchor = the prefix
 * row's start, one download.  band_params->skip, scale and clip must equal map_params' (else S5GPU_ERR_ARG).  map_rows_out[0 .. n): the
 * prefix mapping; rows_out[0 .. n): the result rows.  The paths come back ragged: ev_first_out (n + 1 entries) is the prefix of
 * rows_out[i].qlen, and lo_out, hi_out and events_out (may be NULL; the query's event rows [skip, skip + qlen) of the read) hold the rows of
 * record i at [ev_first_out[i], ev_first_out[i + 1]); rows_cap: their room in rows.  Too little room: S5GPU_ERR_NOMEM and ev_first_out[0] =
 * the rows that suffice (the sum of the reads' Q).  The reads are aligned in groups of consecutive reads whose scratch is at most
 * scratch_max bytes (0: 1 GiB); a read whose scratch alone is above it has S5GPU_STATUS_PATH_WIDE and no path, the others stay valid.
 * status_out (may be NULL): 0, S5GPU_STATUS_QUERY_SHORT, S5GPU_STATUS_PATH_ROW (a read with a long query but no anchor: emin below
 * map_params->qmin), S5GPU_STATUS_PATH_WIDE or the decoder's.  A corrupt record fails the call with S5GPU_ERR_DATA as in
 * s5gpu_align_batch: its rows are empty, the other reads' outputs are valid.  S5GPU_ERR_ARG before a device is needed: the cases of
 * s5gpu_map_batch, a band parameter outside its range, a NULL output. */
int s5gpu_extend_batch(uint32_t n, const void *const *rec, const size_t *rec_len, int rec_method, int sig_method,
                       const s5gpu_event_params_t *event_params, const s5gpu_map_params_t *map_params, const s5gpu_band_params_t *band_params,
                       size_t scratch_max, const int16_t *ref_host, uint32_t R, s5gpu_map_row_t *map_rows_out, s5gpu_ext_row_t *rows_out,
                       uint64_t *ev_first_out, int32_t *lo_out, int32_t *hi_out, s5gpu_event_t *events_out, size_t rows_cap, int32_t *status_out);

/* ---- pileup of whole reads: the ragged paths of extend added to the table (docs/codecs.md §4.22) ----
 * The accumulator is that of "pileup" above; fixed-pitch and ragged calls may add to one accumulator in any order and on several streams.
 * The inputs are laid out as s5gpu_sdtw_band_dev leaves them: read k's rows at [first[k], first[k] + qlen[k]) of queries, lo and hi
 * ([total_rows] each).  Read k is SKIPPED iff status[k] != 0 or qlen[k] == 0; else BAD iff qlen[k] > 2^20, first[k] > first[k + 1],
 * first[k + 1] > total_rows, qlen[k] + ev_skip > first[k + 1] - first[k], or a row fails the path rule of "pileup" against the row before
 * it in the ragged array; else USED, with the cells of "pileup", i the row within the read.  Nothing of a read is accumulated unless every
 * row of it passed.  events (may be NULL; ev_skip then counts as 0): the samples of row i of read k are
 * events[first[k] + ev_skip + i].length.  For reads of at most 1024 rows the table is byte for byte s5gpu_pileup_accum_dev's. */
/* The bytes of the work area of a ragged call (0: total_rows above 2^40). */
size_t s5gpu_pileup_long_work_bytes(uint32_t n, uint64_t total_rows);
/* Asynchronous on hip_stream; writes nothing but acc and work (DEVICE memory, 16-byte aligned; a work area per call in flight).
 * n = 0: S5GPU_OK and nothing is launched.  S5GPU_ERR_ARG, nothing launched: a NULL or misaligned pointer (first: 8 bytes; events, work,
 * acc: 16), R outside 1 .. 2^26, total_rows above 2^40.  S5GPU_ERR_NOMEM, nothing written: work_bytes below
 * s5gpu_pileup_long_work_bytes(n, total_rows). */
int s5gpu_pileup_accum_long_dev(uint32_t n, const int16_t *queries, const uint64_t *first, const uint32_t *qlen, uint64_t total_rows,
                                const int16_t *ref, uint32_t R, const int32_t *lo, const int32_t *hi, const int32_t *status,
                                const s5gpu_event_t *events, uint32_t ev_skip, void *work, size_t work_bytes, void *acc, void *hip_stream);
/* A per-file handle as s5gpu_pileup_open's, for whole reads: s5gpu_pileup_add_batch_whole runs the device side of s5gpu_extend_batch
 * (band_params and map_params must agree as there; scratch_max as there) and adds the ragged paths; s5gpu_pileup_close serves both kinds.
 * The add of the other kind returns S5GPU_ERR_ARG and leaves the handle usable.  NULL: the S5GPU_ERR_ARG cases of s5gpu_extend_batch,
 * R > 2^26, no device, no memory. */
void *s5gpu_pileup_open_whole(const s5gpu_event_params_t *event_params, const s5gpu_map_params_t *map_params,
                              const s5gpu_band_params_t *band_params, size_t scratch_max, const int16_t *ref_host, uint32_t R);
/* map_rows_out, ext_rows_out and status_out ([n] each, may be NULL) are what s5gpu_extend_batch returns for the batch; the paths never
 * leave the device.  Records that never reached the device count in reads_skipped; a corrupt record behaves as in s5gpu_pileup_add_batch. */
int s5gpu_pileup_add_batch_whole(void *handle, uint32_t n, const void *const *rec, const size_t *rec_len, int rec_method, int sig_method,
                                 s5gpu_map_row_t *map_rows_out, s5gpu_ext_row_t *ext_rows_out, int32_t *status_out);

/* ---- refine, whole reads: the fit along extend's ragged paths, and rounds of the banded alignment (docs/codecs.md §4.24) ----
 * "refine" above works on the fixed-pitch matrices of at most 1024 events.  These calls do the same on the ragged layout of "extend": read
 * k's rows at [first[k], first[k] + qlen[k]) of queries, lo and hi ([total_rows] each), qlen[k] <= 2^20.  Who is fitted is decided as in
 * "pileup of whole reads" with ev_skip = 0: a read whose status_in is not 0 or whose qlen is 0 is SKIPPED (it keeps its status and has no
 * fit); one with a flaw in its layout or a row that fails the path rule is BAD (S5GPU_STATUS_PATH_ROW, no fit); the others are fitted over
 * all the cells of their paths, whole or not at all.  There is no wmax.  The sums are exact in int64, the solve is that of "refine":
 * S5GPU_STATUS_FIT_FLAT and S5GPU_STATUS_FIT_RANGE as there.  refine_params->pad must be in its range and is not used: the band is the
 * window.  Integer-exact but for the one solve in double; reproducible bit for bit whatever the launch shape. */
/* The bytes of the work area of s5gpu_path_fit_long_dev (0: total_rows above 2^40). */
size_t s5gpu_path_fit_long_work_bytes(uint32_t n, uint64_t total_rows);
/* fit_out[k]: a, b and the six sums (a = 1, b = 0 and zeros for a read that is not fitted; a = 1, b = 0 and its sums for one whose fit is
 * refused); status_out[k]: 0, the status that came in, S5GPU_STATUS_PATH_ROW, S5GPU_STATUS_FIT_FLAT or S5GPU_STATUS_FIT_RANGE; queries_out
 * (may be NULL; [total_rows]): q' = clamp(rint(a q + b), -clip, clip) at the rows of the reads whose status_out is 0, zeros everywhere
 * else.  Asynchronous on hip_stream; writes nothing but the outputs and work (DEVICE memory, 16-byte aligned, a work area per call in
 * flight).  refine_params: a HOST struct.  n = 0: S5GPU_OK and nothing is launched.  S5GPU_ERR_ARG, nothing launched: a refine parameter
 * outside its range, R outside 1 .. 2^31 - 1, total_rows above 2^40, a NULL or misaligned pointer (first: 8 bytes; fit_out, work: 16),
 * queries_out == queries.  S5GPU_ERR_NOMEM, nothing written: work_bytes below s5gpu_path_fit_long_work_bytes(n, total_rows).
 * s5gpu_set_option (tests, tools): "refine_long_passes" (1 .. 63, default 63) says which kernels these calls launch: 1 the plan and the
 * check, 2 the sums, 4 the solve, 8 the requantiser, 16 the bookkeeping of the rounds, 32 the band call. */
int s5gpu_path_fit_long_dev(uint32_t n, const int16_t *queries, const uint64_t *first, const uint32_t *qlen, uint64_t total_rows,
                            const int16_t *ref, uint32_t R, const int32_t *lo, const int32_t *hi, const int32_t *status_in,
                            const s5gpu_refine_params_t *refine_params, void *work, size_t work_bytes, s5gpu_fit_t *fit_out,
                            int16_t *queries_out, int32_t *status_out, void *hip_stream);
/* The bytes of the work area of s5gpu_extend_refine_dev: the fit's and a trial round (0: total_rows above 2^40). */
size_t s5gpu_extend_refine_work_bytes(uint32_t n, uint64_t total_rows);
/* refine_params->iters rounds on device buffers, nothing downloaded in between.  What comes in is what s5gpu_sdtw_band_dev left: the long
 * queries, rows_in (a read's status_in is rows_in[k].status), lo_in, hi_in.  Round 0 makes the outputs copies of what came in, with a = 1,
 * b = 0 and rounds 0; a SKIPPED or BAD read has "no result": zeros in queries_out, -1 in lo_out and hi_out, the empty row with its
 * status, and takes no part.  Round j >= 1: the fit of the query that CAME IN along the path the read has, q' from it, and the banded
 * alignment of q' (band_params->tile_rows and band; anchor: `start` of the row the read has) into a trial; where both succeed the trial
 * becomes the read's result and rounds_out[k] = j; a read that gets a fit status or a band status keeps the last round that succeeded,
 * takes no further part, and reports that status in rows_out[k].status.  queries_out holds zeros and lo_out, hi_out -1 at every row that
 * is behind a read's query or belongs to no read.  What comes out feeds s5gpu_pileup_accum_long_dev as it is (status: rows_out[k].status).
 * scratch: that of s5gpu_sdtw_band_scratch_bytes(n, total_rows, tile_rows, band), used again every round; too small: S5GPU_ERR_NOMEM and
 * nothing is written, as with a work area below s5gpu_extend_refine_work_bytes(n, total_rows).  S5GPU_ERR_ARG, nothing launched: a band
 * or refine parameter outside its range, R outside 1 .. 2^31 - 1, total_rows above 2^40, a NULL or misaligned pointer (rows, fit_out,
 * scratch, work: 16 bytes; first: 8), an output that is an input.  n = 0: S5GPU_OK.  Asynchronous on hip_stream. */
int s5gpu_extend_refine_dev(uint32_t n, const int16_t *queries, const uint64_t *first, const uint32_t *qlen, uint64_t total_rows,
                            const int16_t *ref, uint32_t R, const s5gpu_ext_row_t *rows_in, const int32_t *lo_in, const int32_t *hi_in,
                            const s5gpu_band_params_t *band_params, const s5gpu_refine_params_t *refine_params, void *scratch,
                            size_t scratch_bytes, void *work, size_t work_bytes, int16_t *queries_out, s5gpu_ext_row_t *rows_out,
                            int32_t *lo_out, int32_t *hi_out, s5gpu_fit_t *fit_out, uint32_t *rounds_out, void *hip_stream);
/* s5gpu_extend_batch with the rounds behind each group's band call: rows_first_out[0 .. n) are the rows of the first alignment (what
 * s5gpu_extend_batch returns), rows_out, lo_out, hi_out the refined ones (ev_first_out: the prefix of rows_out[i].qlen), queries_out (may
 * be NULL) the refined long queries laid out as lo_out, fit_out[0 .. n) and rounds_out (may be NULL) the fits and the rounds that
 * succeeded.  status_out (may be NULL): those of s5gpu_extend_batch, S5GPU_STATUS_FIT_FLAT, S5GPU_STATUS_FIT_RANGE.  The results do not
 * depend on how scratch_max cuts the groups.  S5GPU_ERR_ARG before a device is needed: the cases of s5gpu_extend_batch, a refine
 * parameter outside its range, a NULL rows_first_out or fit_out. */
int s5gpu_extend_refine_batch(uint32_t n, const void *const *rec, const size_t *rec_len, int rec_method, int sig_method,
                              const s5gpu_event_params_t *event_params, const s5gpu_map_params_t *map_params,
                              const s5gpu_band_params_t *band_params, const s5gpu_refine_params_t *refine_params, size_t scratch_max,
                              const int16_t *ref_host, uint32_t R, s5gpu_map_row_t *map_rows_out, s5gpu_ext_row_t *rows_first_out,
                              s5gpu_ext_row_t *rows_out, uint64_t *ev_first_out, int32_t *lo_out, int32_t *hi_out, s5gpu_event_t *events_out,
                              int16_t *queries_out, size_t rows_cap, s5gpu_fit_t *fit_out, uint32_t *rounds_out, int32_t *status_out);
/* Refinement inside the whole-read handles: behind this call s5gpu_pileup_add_batch_whole (s5gpu_contrast_add_batch) runs the rounds and
 * feeds the table (and the histograms) with the refined queries, paths and statuses: the table's sums of levels and the histograms' bins
 * are then in the reference's units, and a read whose rounds ended with a status is skipped.  ext_rows_out of the add are the refined
 * rows.  NULL turns refinement off.  S5GPU_ERR_ARG: a NULL handle, a handle that is not a whole-read one, one that has added a batch
 * already, a parameter outside its range. */
int s5gpu_pileup_set_refine(void *handle, const s5gpu_refine_params_t *refine_params);
int s5gpu_contrast_set_refine(void *handle, const s5gpu_refine_params_t *refine_params);

/* ---- contrast: per-position level histograms and a two-sample comparison of them (docs/codecs.md §4.23) ----
 * A histogram is a head and R columns of 64 uint32_t counts that stay on the device beside (or without) the table of "pileup".  The bin of a
 * quantised level q: d = (int32)q - q0; bin = d < 0 ? 0 : min(d >> shift, 63), q0 in -32768 .. 32767, shift in 0 .. 10.  Which reads are
 * USED, SKIPPED and BAD and which cells (i, j) a used read has is "pileup of whole reads"' rule with ev_skip = 0; column j, bin b counts the
 * cells (i, j) of used reads with bin(q[i]) = b.  Every member is an integer sum: the bytes do not depend on the order of reads, segments,
 * calls, streams or atomics, and fed the same reads the bins of column j add up to the table's n_events[j], the head's counts to its totals. */
typedef struct s5gpu_pile_hist_head {  /* 64 bytes in front of the columns */
    uint64_t cells;                    /* the cells counted: the sum of every bin */
    uint64_t reads_used, reads_skipped, reads_bad;
    uint32_t R;
    int32_t q0;
    uint32_t shift, bins;              /* bins: 64 */
    uint64_t reserved[2];
} s5gpu_pile_hist_head_t;
typedef struct s5gpu_pile_contrast {   /* 40 bytes: column j of two histograms A and B held against each other.  c*_b: the inclusive prefix sums */
    uint32_t n_a, n_b;                 /* nA, nB: the columns' cells (0xFFFFFFFF: that or more) */
    uint32_t depth_a, depth_b;         /* the tables' depth (0 without tables) */
    uint64_t ks_num;                   /* max_b |cA_b nB - cB_b nA|: the two-sample Kolmogorov-Smirnov statistic is D = ks_num / (nA nB) */
    uint64_t ov_num;                   /* sum_b min(A_b nB, B_b nA): 1 - ov_num / (nA nB) is the total-variation distance */
    uint16_t ks_bin;                   /* the smallest b that attains ks_num */
    uint16_t med_a, med_b;             /* the smallest b with 2 c_b >= n (0 for an empty column) */
    uint16_t flags;                    /* S5GPU_CONTRAST_* */
} s5gpu_pile_contrast_t;
#define S5GPU_CONTRAST_EMPTY_A 1u      /* nA = 0 */
#define S5GPU_CONTRAST_EMPTY_B 2u      /* nB = 0 */
#define S5GPU_CONTRAST_A_LOWER 4u      /* at ks_bin cA_b nB > cB_b nA: A's levels lie lower */
#define S5GPU_CONTRAST_BIG 8u          /* nA or nB >= 2^31: the products would not fit; ks_num = ov_num = 0 and ks_bin = 0, the rest filled */
#define S5GPU_CONTRAST_TABLE_A 16u     /* a table was given and its n_events is not nA */
#define S5GPU_CONTRAST_TABLE_B 32u     /* ... nB */
#define S5GPU_CONTRAST_HEADS 128u      /* the two heads disagree (R, q0, shift, bins): set in every row, and nothing else is */
/* 64 + 256 R, the bytes of a histogram of R columns; 0 for R = 0 or R > 2^22 (1 GiB). */
size_t s5gpu_pile_hist_bytes(uint32_t R);
/* Writes the empty histogram (zeros and the head) to hist (DEVICE memory, 16-byte aligned, s5gpu_pile_hist_bytes(R)).  Asynchronous on
 * hip_stream.  S5GPU_ERR_ARG: R, q0 or shift outside its range, a NULL or misaligned pointer. */
int s5gpu_pile_hist_reset_dev(void *hist, uint32_t R, int32_t q0, uint32_t shift, void *hip_stream);
/* Adds n reads in the ragged layout of s5gpu_pileup_accum_long_dev (neither a reference nor events are needed) to hist, which
 * s5gpu_pile_hist_reset_dev wrote for the same R; q0 and shift are the reset's.  Asynchronous on hip_stream; writes nothing but hist and
 * work (s5gpu_pileup_long_work_bytes(n, total_rows); a work area per call in flight).  Calls on several streams may share a histogram.
 * n = 0: S5GPU_OK and nothing is launched.  S5GPU_ERR_ARG, nothing launched: a NULL or misaligned pointer (first: 8 bytes; work, hist: 16),
 * R outside 1 .. 2^22, total_rows above 2^40.  S5GPU_ERR_NOMEM, nothing written: a short work area.
 * s5gpu_set_option (tests, tools): "pile_hist_cols" (0, or a power of two 16 .. 256; default 256): the columns a workgroup keeps in LDS, 256
 * bytes each (0: every cell is a global atomic); "pile_hist_grid" (1 .. 1024, default 1024); "pileup_long_seg" and "pileup_long_sort" count
 * as they do for the table.  None changes the result. */
int s5gpu_pile_hist_accum_long_dev(uint32_t n, const int16_t *queries, const uint64_t *first, const uint32_t *qlen, uint64_t total_rows, uint32_t R,
                                   const int32_t *lo, const int32_t *hi, const int32_t *status, void *work, size_t work_bytes, void *hist,
                                   void *hip_stream);
/* Writes R rows to out (DEVICE memory, 8-byte aligned) from two histograms of R columns and, when given, the two tables of the same reads
 * (acc_a and acc_b: both or neither).  The heads are read on the device.  Asynchronous on hip_stream; all integer and exact for
 * nA, nB < 2^31.  S5GPU_ERR_ARG: R outside 1 .. 2^22, a NULL or misaligned pointer, one table without the other. */
int s5gpu_pile_contrast_dev(const void *hist_a, const void *hist_b, const void *acc_a, const void *acc_b, uint32_t R, s5gpu_pile_contrast_t *out,
                            void *hip_stream);
/* A per-file handle over the chain of s5gpu_pileup_open_whole with two sides: a table and a histogram each, on the first device in use.
 * NULL: the cases of s5gpu_pileup_open_whole, R > 2^22, q0 or shift outside its range. */
void *s5gpu_contrast_open(const s5gpu_event_params_t *event_params, const s5gpu_map_params_t *map_params, const s5gpu_band_params_t *band_params,
                          size_t scratch_max, const int16_t *ref_host, uint32_t R, int32_t q0, uint32_t shift);
/* s5gpu_pileup_add_batch_whole into the table and the histogram of side 0 or 1 (any other: S5GPU_ERR_ARG).  Records that never reached the
 * device count as skipped in both; a corrupt record: S5GPU_ERR_DATA, the rest of the batch added, the handle usable. */
int s5gpu_contrast_add_batch(void *handle, int side, uint32_t n, const void *const *rec, const size_t *rec_len, int rec_method, int sig_method,
                             s5gpu_map_row_t *map_rows_out, s5gpu_ext_row_t *ext_rows_out, int32_t *status_out);
/* Runs the comparison, downloads the R rows to rows_out and, where not NULL, the two tables (HOST memory, s5gpu_pileup_bytes(R) each), and
 * ends the handle, whatever it returns.  rows_out NULL: the handle is abandoned. */
int s5gpu_contrast_close(void *handle, void *acc_a_out, void *acc_b_out, s5gpu_pile_contrast_t *rows_out);

/* ---- sites: per-read levels at chosen reference columns, each held against a control histogram (docs/codecs.md §4.25) ----
 * sites[0 .. M) are reference columns, strictly increasing, each < R.  Which reads are USED, SKIPPED and BAD is "pileup of whole reads"'
 * rule with ev_skip = 0.  The cell of read k at site t sums the rows i of a used read with lo[i] <= sites[t] <= hi[i]; the matrix is
 * site-major, out[t * n + k].  Sums and a minimum only: the bytes do not depend on the order of segments, calls or atomics. */
typedef struct s5gpu_site_cell {       /* 16 bytes */
    int64_t sum_q;                     /* the sum of q[i] over the rows that cross the site */
    uint32_t cells;                    /* how many rows do */
    uint32_t row0;                     /* the smallest such i; 0xFFFFFFFF in the empty entry {0, 0, 0xFFFFFFFF} */
} s5gpu_site_cell_t;
typedef struct s5gpu_site_score {      /* 16 bytes: a cell held against column sites[t] of a control histogram with counts C */
    int16_t level;                     /* floor((2 sum_q + cells) / (2 cells)): the mean rounded half up */
    uint16_t flags;                    /* S5GPU_SITE_* */
    uint32_t below, above, n;          /* with b the bin of level: the sum of C_x over x <= b, over x >= b, over all x; 0xFFFFFFFF: that or more */
} s5gpu_site_score_t;
#define S5GPU_SITE_NO_CELL 1u          /* the read has no cell at the site: level = below = above = 0, n is filled */
#define S5GPU_SITE_EMPTY 2u            /* n = 0 */
#define S5GPU_SITE_COLUMN 64u          /* sites[t] >= R: no column is read and it counts as empty (S5GPU_SITE_EMPTY is set beside it) */
#define S5GPU_SITE_HEAD 128u           /* the histogram's head disagrees with R or with 64 bins: set in every row, and nothing else is */
/* Writes all M n cells to cells_out (DEVICE memory, 16-byte aligned): the empty entries first, then the cells of the n reads of a ragged
 * batch as s5gpu_pile_hist_accum_long_dev takes it, at the M columns sites_dev (DEVICE memory) lists.  verdict_out (DEVICE memory, [n], or
 * NULL): 0 used, 1 skipped, 2 bad.  Asynchronous on hip_stream; writes nothing but cells_out, verdict_out and work
 * (s5gpu_pileup_long_work_bytes(n, total_rows); a work area per call in flight).  A list that is not strictly increasing gives unspecified
 * counts inside cells_out, never an access outside the arrays; the host-side callers (the handle, the Python module, the tool) validate it.
 * n = 0: S5GPU_OK and nothing is launched.  S5GPU_ERR_ARG, nothing launched: a NULL or misaligned pointer (first: 8 bytes; work, cells_out:
 * 16), R outside 1 .. 2^22, total_rows above 2^40, M outside 1 .. 65536, M n above 2^27.  S5GPU_ERR_NOMEM, nothing written: a short work
 * area.  "pileup_long_seg" and "pileup_long_grid" of s5gpu_set_option count as they do for the table; neither changes the result. */
int s5gpu_site_cells_long_dev(uint32_t n, const int16_t *queries, const uint64_t *first, const uint32_t *qlen, uint64_t total_rows, uint32_t R,
                              const int32_t *lo, const int32_t *hi, const int32_t *status, const uint32_t *sites_dev, uint32_t M, void *work,
                              size_t work_bytes, s5gpu_site_cell_t *cells_out, uint32_t *verdict_out, void *hip_stream);
/* Writes the M n score rows of cells (as s5gpu_site_cells_long_dev left them) against hist, a histogram of "contrast" with R columns, to out
 * (DEVICE memory, 16-byte aligned as cells).  The head is read on the device.  All integer; below / n is an empirical share of the control's
 * cells, not a calibrated probability, and a read that was itself added to the control counts among its own control.  Asynchronous on
 * hip_stream.  n = 0: S5GPU_OK and nothing is launched.  S5GPU_ERR_ARG: a NULL or misaligned pointer, R outside 1 .. 2^22, M outside
 * 1 .. 65536, M n above 2^27. */
int s5gpu_site_score_dev(const s5gpu_site_cell_t *cells, uint32_t n, const uint32_t *sites_dev, uint32_t M, const void *hist, uint32_t R,
                         s5gpu_site_score_t *out, void *hip_stream);
/* A per-file handle over the chain of s5gpu_pileup_open_whole: the site list and an empty control histogram on the first device in use.
 * NULL: the cases of s5gpu_contrast_open, M outside 1 .. 65536, a list that is not strictly increasing, a column >= R. */
void *s5gpu_sites_open(const s5gpu_event_params_t *event_params, const s5gpu_map_params_t *map_params, const s5gpu_band_params_t *band_params,
                       size_t scratch_max, const int16_t *ref_host, uint32_t R, const uint32_t *sites_host, uint32_t M, int32_t q0, uint32_t shift);
/* As s5gpu_contrast_set_refine: the control, the cells and the scores are then fed with the refined queries, paths and statuses. */
int s5gpu_sites_set_refine(void *handle, const s5gpu_refine_params_t *refine_params);
/* The chain of s5gpu_pileup_add_batch_whole into the control histogram only.  A corrupt record: S5GPU_ERR_DATA, the rest added. */
int s5gpu_sites_add_control(void *handle, uint32_t n, const void *const *rec, const size_t *rec_len, int rec_method, int sig_method,
                            int32_t *status_out);
/* Replaces the control with a histogram made elsewhere (HOST memory, s5gpu_pile_hist_bytes(R)).  S5GPU_ERR_ARG: a head that disagrees with
 * the handle's R, q0, shift or 64 bins. */
int s5gpu_sites_set_control(void *handle, const void *hist_host);
/* The chain into cells_out (HOST memory, [M][n], record k at [t * n + k]) and, where not NULL, scores_out ([M][n], against the control as it
 * stands).  Records that never reached the device have empty entries (and the scores of one).  The control is not changed.  A corrupt
 * record: S5GPU_ERR_DATA, the rest of the batch valid, the handle usable.  S5GPU_ERR_ARG: a NULL handle or cells_out, M n above 2^27. */
int s5gpu_sites_add_batch(void *handle, uint32_t n, const void *const *rec, const size_t *rec_len, int rec_method, int sig_method,
                          s5gpu_ext_row_t *ext_rows_out, s5gpu_site_cell_t *cells_out, s5gpu_site_score_t *scores_out, int32_t *status_out);
/* Downloads the control histogram to hist_out where not NULL (HOST memory, s5gpu_pile_hist_bytes(R)) and ends the handle, whatever it returns. */
int s5gpu_sites_close(void *handle, void *hist_out);

/* ---- model: the pileup folded onto k-mers, and a level table re-estimated from it (docs/codecs.md §4.26) ----
 * A fold adds the columns of a table of "pileup", or of a histogram of "contrast", that share a class: cls[j] is the class of input column
 * j, and column j is KEPT iff cls[j] < K.  Every member of output column c is the sum over the kept j with cls[j] = c (min_q and max_q the
 * minimum and maximum over those j that are not empty), so the result is an ordinary table (histogram) of K columns: to_host, the line
 * printers and s5gpu_pile_contrast_dev take it as it stands.  The head's reads are the input's; its cells and cost are the sums over the
 * kept columns only, so cells = sum of n_events and cost = sum of sum_cost hold on the output.  All integer: the bytes do not depend on
 * the launch shape or on the order of the adds. */
#define S5GPU_FOLD_NONE 0xFFFFFFFFu    /* cls[j]: the column belongs to no class (any value >= K is dropped the same way) */
#define S5GPU_FOLD_REFUSED 1u          /* reserved[0] of the output's head: a fold added nothing (see below) */
/* the mean and the standard deviation "quant" takes of m[0 .. L) (double, left to right): with scale they invert s5gpu_quantise_host.
 * S5GPU_ERR_ARG: a NULL pointer or L = 0. */
int s5gpu_quant_stats_host(const float *m, size_t L, double *mu_out, double *sd_out);
/* One class per column of a reference of s5gpu_refseq_build / _open, cls_out[0 .. R): the base-4 rank of the k-mer the column shows, which
 * is the rank whose model level the column took -- on a forward segment, on a reverse-complement segment (the k-mer of the reverse-
 * complement sequence) and under the RNA rule (the columns are reversed, the ranks are not); S5GPU_FOLD_NONE for a wall column and for a
 * k-mer that holds a letter other than ACGT.  *K_out = 4^k.  Either output may be NULL. */
int s5gpu_refseq_classes(const void *h, uint32_t *cls_out, uint32_t *K_out);
/* mu and sd of the levels of all segments together, as the reference's quantiser took them, and its scale: a quantised level q stands for
 * mu + (sd / scale) q.  Any output may be NULL. */
int s5gpu_refseq_quant(const void *h, double *mu_out, double *sd_out, double *scale_out);
/* Adds the fold of acc_in (R columns) to acc_out, which s5gpu_pileup_reset_dev wrote for K columns; cls[0 .. R) and both tables DEVICE
 * memory.  Asynchronous on hip_stream.  The fold ADDS: several inputs may go into one output.  depth and n_events are 32-bit: the kernel
 * reads the input's total cells, and where that is 2^32 or more (or a head's R is not the R or K of the call) it adds nothing and sets
 * S5GPU_FOLD_REFUSED; otherwise every sum of this call fits.  The caller answers for the sums over several calls into one output.
 * S5GPU_ERR_ARG (nothing launched): a NULL or misaligned pointer (tables: 16 bytes; cls: 4), R or K outside 1 .. 2^26, acc_out = acc_in.
 * s5gpu_set_option (tests, tools): "pile_fold_lds" (0 / 1): for K <= 1024 a workgroup keeps the whole class table in LDS and adds its
 * non-empty classes to the output at its end (1), or every merge is a global atomic (0); "pile_fold_grid" (1 .. 1024): the most
 * workgroups of a launch.  Neither changes the result. */
int s5gpu_pileup_fold_dev(const void *acc_in, uint32_t R, const uint32_t *cls, uint32_t K, void *acc_out, void *hip_stream);
/* The same for a histogram of "contrast": hist_out was written by s5gpu_pile_hist_reset_dev for K columns.  q0, shift and bins of the two
 * heads are compared on the device: where they disagree, or the input's cells are 2^32 or more, nothing is added and S5GPU_FOLD_REFUSED is
 * set in reserved[0] of hist_out's head.  S5GPU_ERR_ARG as above, with R and K in 1 .. 2^22. */
int s5gpu_pile_hist_fold_dev(const void *hist_in, uint32_t R, const uint32_t *cls, uint32_t K, void *hist_out, void *hip_stream);
/* s5gpu_pileup_close for a handle of either kind, folded: cls_host[0 .. R) (HOST memory) is uploaded, the table folded onto K columns
 * on the device, and 64 + 48 K bytes come to acc_out (HOST memory).  Ends the handle, whatever it returns. */
int s5gpu_pileup_close_folded(void *handle, const uint32_t *cls_host, uint32_t K, void *acc_out);
/* s5gpu_contrast_close, folded: both sides' table and histogram folded onto K columns, s5gpu_pile_contrast_dev over the K rows; rows_out
 * [K], acc_a_out and acc_b_out (64 + 48 K bytes each, may be NULL).  Ends the handle, whatever it returns. */
int s5gpu_contrast_close_folded(void *handle, const uint32_t *cls_host, uint32_t K, void *acc_a_out, void *acc_b_out,
                                s5gpu_pile_contrast_t *rows_out);
typedef struct s5gpu_kmer_row {    /* 40 bytes: a k-mer of a re-estimated table */
    double level, stdv;            /* in the units of the table that made the reference */
    double dwell;                  /* n_samples / cells: samples per event (0 when no event lengths were given) */
    uint32_t cells;                /* n_events of the class */
    uint32_t kept;                 /* 1: fewer than min_cells cells; level is levels_in's, stdv and dwell are 0 */
    uint64_t zero;
} s5gpu_kmer_row_t;
/* The estimate, on the host, from a folded table (HOST memory, 64 + 48 K bytes) and s5gpu_refseq_quant's mu, sd and scale.  For a class
 * with n = n_events >= min_cells: mean_q = sum_q / n, var_q = max(0, sumsq_q / n - mean_q^2), level = mu + (sd / scale) mean_q,
 * stdv = (sd / scale) sqrt(var_q), dwell = n_samples / n; double, left to right, without contraction.  A class below min_cells keeps
 * levels_in[c] (kept = 1).  Two limits: queries are clamped to +-clip, so a k-mer whose level lies near +-clip / scale standard deviations
 * is biased inwards; and the estimate is in the units of the table that made the reference, so a round changes the table's shape, not
 * its overall scale.  S5GPU_ERR_ARG: a NULL pointer, K = 0, a head whose R is not K, sd or scale not finite or <= 0. */
int s5gpu_kmer_model_solve(const void *acc_folded, uint32_t K, double mu, double sd, double scale, uint32_t min_cells, const float *levels_in,
                           s5gpu_kmer_row_t *rows_out);

#ifdef __cplusplus
}
#endif
#endif
