"""ctypes binding of libslow5gpu.so (the C ABI in include/slow5gpu.h).

There is no fallback: if the library is missing it is built (hipcc); if that fails, or a call is
made without a gfx950 GPU, the error is raised to the caller.
"""
import ctypes as C
import os

import numpy as np

from . import build as _build

_LIB = None

REC_NONE, REC_ZLIB, REC_ZSTD = 0, 1, 2
SIG_NONE, SIG_SVB_ZD, SIG_EX_ZD = 0, 1, 2

# numpy mirrors of the C structs (same field order / padding as include/slow5gpu.h)
READ_DESC = np.dtype([("sig_off", "<u8"), ("hdr_off", "<u8"), ("aux_off", "<u8"), ("out_off", "<u8"),
                      ("n_samples", "<u4"), ("hdr_len", "<u4"), ("aux_len", "<u4"), ("slot_cap", "<u4")])
REC_DESC = np.dtype([("in_off", "<u8"), ("pay_off", "<u8"), ("sig_off", "<u8"),
                     ("in_len", "<u4"), ("pay_cap", "<u4"), ("sig_cap", "<u4"), ("reserved", "<u4")])
REC_FIELDS = np.dtype([("status", "<i4"), ("payload_len", "<u4"), ("n_samples", "<u4"), ("read_id_len", "<u4"),
                       ("read_group", "<u4"), ("aux_off", "<u4"), ("aux_len", "<u4"), ("reserved", "<u4"),
                       ("digitisation", "<f8"), ("offset", "<f8"), ("range", "<f8"), ("sampling_rate", "<f8")])
assert READ_DESC.itemsize == 48 and REC_DESC.itemsize == 40 and REC_FIELDS.itemsize == 64
# s5gpu_file_stats_t: the file-wide accumulator of "stats" (slow5tools_amd/fstats.py)
FILE_STATS = np.dtype([("n_reads", "<u8"), ("n_failed", "<u8"), ("n_samples", "<u8"), ("sum", "<i8"), ("sumsq", "<u8"),
                       ("min", "<i4"), ("max", "<i4"), ("or_bits", "<u4"), ("and_bits", "<u4"), ("len_min", "<u4"), ("len_max", "<u4"),
                       ("len_hist", "<u8", (33,)), ("rg_reads", "<u8", (256,)), ("rg_samples", "<u8", (256,)), ("rg_other", "<u8"),
                       ("hist", "<u8", (65536,))])
assert FILE_STATS.itemsize == 528720
# s5gpu_sig_diff_t / s5gpu_diff_acc_t: a pair's row and the file-wide accumulator of "diff" (slow5tools_amd/diff.py)
SIG_DIFF = np.dtype([("status_a", "<i4"), ("status_b", "<i4"), ("n_a", "<u4"), ("n_b", "<u4"), ("flags", "<u4"), ("n_diff", "<u4"),
                     ("first_diff", "<u4"), ("max_abs", "<u4"), ("max_at", "<u4"), ("reserved", "<u4"), ("sum_d", "<i8"), ("sum_abs", "<u8"),
                     ("sum_sq", "<u8"), ("sum_a", "<i8"), ("sumsq_a", "<u8")])
DIFF_BINS = 131071
DIFF_ACC = np.dtype([("n_pairs", "<u8"), ("n_failed", "<u8"), ("n_differ", "<u8"), ("n_signal", "<u8"), ("n_len", "<u8"), ("n_fields", "<u8"),
                     ("n_aux", "<u8"), ("n_id", "<u8"), ("n_samples", "<u8"), ("n_diff", "<u8"), ("sum_d", "<i8"), ("sum_abs", "<u8"),
                     ("sum_sq", "<u8"), ("sum_a", "<i8"), ("sumsq_a", "<u8"), ("max_abs", "<u4"), ("reserved", "<u4"), ("hist", "<u8", (DIFF_BINS,))])
assert SIG_DIFF.itemsize == 80 and DIFF_ACC.itemsize == 1048696
DIFF_SIGNAL, DIFF_LEN, DIFF_READ_GROUP, DIFF_DIGITISATION, DIFF_OFFSET, DIFF_RANGE, DIFF_SAMPLING_RATE, DIFF_ID, DIFF_AUX = (1 << k for k in range(9))
DIFF_FAILED, DIFF_BAD_PAIR, DIFF_NONE = 0x4000, 0x8000, 0xFFFFFFFF


class EncodeArgs(C.Structure):
    _fields_ = [("n_reads", C.c_uint32), ("rec_method", C.c_int32), ("sig_method", C.c_int32),
                ("desc", C.c_void_p), ("sig", C.c_void_p), ("hdr", C.c_void_p), ("aux", C.c_void_p),
                ("slots", C.c_void_p), ("out_len", C.c_void_p), ("max_payload", C.c_uint32),
                ("lds_payload_cap", C.c_uint32), ("ovf", C.c_void_p)]


DEC_NO_PAYLOAD = 1


class DecodeArgs(C.Structure):
    _fields_ = [("n_recs", C.c_uint32), ("rec_method", C.c_int32), ("sig_method", C.c_int32), ("flags", C.c_uint32),
                ("desc", C.c_void_p), ("in_", C.c_void_p), ("payload", C.c_void_p), ("sig_out", C.c_void_p),
                ("fields", C.c_void_p), ("payload_bytes", C.c_uint64), ("max_pay_cap", C.c_uint32), ("max_in_len", C.c_uint32)]


assert C.sizeof(DecodeArgs) == 72


SKIM_MAX_AUX, SKIM_MAX_LABELS, SKIM_TEXT = 64, 1024, 16384
SKIM_DOT, SKIM_STRING, SKIM_DOUBLE, SKIM_FLOAT, SKIM_INT32, SKIM_UINT8, SKIM_UINT32, SKIM_UINT64, SKIM_ENUM = range(9)
STATUS_BAD_ENUM = 8

NORM_RAW, NORM_PA, NORM_MEDMAD, NORM_QUANT = range(4)
SIG_F32, SIG_F16 = 0, 1


class SkimLayout(C.Structure):
    """s5gpu_skim_layout_t"""
    _fields_ = [("n_aux", C.c_uint32), ("n_labels_total", C.c_uint32), ("text_len", C.c_uint32), ("n_unhandled", C.c_uint32),
                ("type", C.c_uint8 * SKIM_MAX_AUX), ("role", C.c_uint8 * SKIM_MAX_AUX), ("n_labels", C.c_uint16 * SKIM_MAX_AUX),
                ("label_first", C.c_uint16 * SKIM_MAX_AUX), ("name_off", C.c_uint32 * SKIM_MAX_AUX), ("name_len", C.c_uint32 * SKIM_MAX_AUX),
                ("label_off", C.c_uint32 * SKIM_MAX_LABELS), ("label_len", C.c_uint16 * SKIM_MAX_LABELS), ("text", C.c_char * SKIM_TEXT)]


class DiffSide(C.Structure):
    """s5gpu_diff_side_t"""
    _fields_ = [("n", C.c_uint32), ("sig", C.c_void_p), ("sig_off", C.c_void_p), ("sig_cap", C.c_void_p), ("fields", C.c_void_p),
                ("payload", C.c_void_p), ("pay_off", C.c_void_p), ("pay_cap", C.c_void_p)]


assert C.sizeof(DiffSide) == 64


class EventParams(C.Structure):
    """s5gpu_event_params_t"""
    _fields_ = [("w1", C.c_uint32), ("w2", C.c_uint32), ("thr1", C.c_double), ("thr2", C.c_double), ("peak_height", C.c_double)]


assert C.sizeof(EventParams) == 32
STATUS_EVENTS_OVERFLOW = 17


class MapParams(C.Structure):
    """s5gpu_map_params_t"""
    _fields_ = [("skip", C.c_uint32), ("qmax", C.c_uint32), ("qmin", C.c_uint32), ("scale", C.c_double), ("clip", C.c_int32), ("want_start", C.c_int32)]


assert C.sizeof(MapParams) == 32
STATUS_QUERY_SHORT = 18
STATUS_PATH_WIDE, STATUS_PATH_ROW = 19, 20


class RefSeqSegment(C.Structure):
    """s5gpu_refseq_segment_t"""
    _fields_ = [("contig", C.c_uint32), ("strand", C.c_int32), ("offset", C.c_uint32), ("Lk", C.c_uint32), ("reversed", C.c_int32), ("zero", C.c_uint32),
                ("name", C.c_char_p)]


class RefSeqLoc(C.Structure):
    """s5gpu_refseq_loc_t"""
    _fields_ = [("contig", C.c_uint32), ("strand", C.c_int32), ("pos", C.c_uint32), ("segment", C.c_uint32)]


assert C.sizeof(RefSeqSegment) == 32 and C.sizeof(RefSeqLoc) == 16
REFSEQ_WALL = 1
# s5gpu_pile_col_t / s5gpu_pile_total_t: a column and the totals row of "pileup" (slow5tools_amd/pileup.py)
PileCol = np.dtype([("depth", "<u4"), ("n_events", "<u4"), ("n_samples", "<u8"), ("sum_q", "<i8"), ("sumsq_q", "<u8"), ("sum_cost", "<u8"),
                    ("min_q", "<i4"), ("max_q", "<i4")])
PileTotal = np.dtype([("reads_used", "<u8"), ("reads_skipped", "<u8"), ("reads_bad", "<u8"), ("cells", "<u8"), ("cost", "<u8"), ("R", "<u4"),
                      ("reserved", "<u4", (5,))])
assert PileCol.itemsize == 48 and PileTotal.itemsize == 64
# s5gpu_pile_hist_head_t / s5gpu_pile_contrast_t: the head of a level histogram and a row of "contrast" (slow5tools_amd/contrast.py)
PileHistHead = np.dtype([("cells", "<u8"), ("reads_used", "<u8"), ("reads_skipped", "<u8"), ("reads_bad", "<u8"), ("R", "<u4"), ("q0", "<i4"), ("shift", "<u4"),
                         ("bins", "<u4"), ("reserved", "<u8", (2,))])
PileContrast = np.dtype([("n_a", "<u4"), ("n_b", "<u4"), ("depth_a", "<u4"), ("depth_b", "<u4"), ("ks_num", "<u8"), ("ov_num", "<u8"), ("ks_bin", "<u2"),
                         ("med_a", "<u2"), ("med_b", "<u2"), ("flags", "<u2")])
assert PileHistHead.itemsize == 64 and PileContrast.itemsize == 40
# s5gpu_site_cell_t / s5gpu_site_score_t: an entry of the read x site matrix of "sites" and its row against a control (slow5tools_amd/sites.py)
SiteCell = np.dtype([("sum_q", "<i8"), ("cells", "<u4"), ("row0", "<u4")])
SiteScore = np.dtype([("level", "<i2"), ("flags", "<u2"), ("below", "<u4"), ("above", "<u4"), ("n", "<u4")])
assert SiteCell.itemsize == 16 and SiteScore.itemsize == 16
# s5gpu_kmer_row_t: a k-mer of a re-estimated level table (slow5tools_amd/model.py)
KmerRow = np.dtype([("level", "<f8"), ("stdv", "<f8"), ("dwell", "<f8"), ("cells", "<u4"), ("kept", "<u4"), ("zero", "<u8")])
assert KmerRow.itemsize == 40
FOLD_NONE, FOLD_REFUSED = 0xFFFFFFFF, 1
STATUS_FIT_FLAT, STATUS_FIT_RANGE = 21, 22
# s5gpu_fit_t: the fit of "refine" (slow5tools_amd/refine.py)
Fit = np.dtype([("a", "<f8"), ("b", "<f8"), ("n", "<i8"), ("sq", "<i8"), ("sr", "<i8"), ("sqq", "<i8"), ("sqr", "<i8"), ("srr", "<i8")])
assert Fit.itemsize == 64


class RefineParams(C.Structure):
    """s5gpu_refine_params_t"""
    _fields_ = [("a_min", C.c_double), ("a_max", C.c_double), ("b_max", C.c_double), ("clip", C.c_int32), ("pad", C.c_uint32), ("min_cells", C.c_uint32),
                ("iters", C.c_uint32)]


assert C.sizeof(RefineParams) == 40


class BandParams(C.Structure):
    """s5gpu_band_params_t"""
    _fields_ = [("skip", C.c_uint32), ("emin", C.c_uint32), ("emax", C.c_uint32), ("tile_rows", C.c_uint32), ("band", C.c_uint32), ("clip", C.c_int32),
                ("scale", C.c_double)]


assert C.sizeof(BandParams) == 32


class S5GpuError(RuntimeError):
    pass


def lib_path():
    return _build.LIB


def lib():
    global _LIB
    if _LIB is not None:
        return _LIB
    path = os.environ.get("S5GPU_LIB") or _build.LIB   # S5GPU_LIB: an experimental build made by tools/variant.sh
    if not os.path.exists(path):
        _build.build()
    # One HIP runtime per process: the torch wheel carries its own libamdhip64 / libhsa-runtime64.  If libslow5gpu.so pulled in
    # /opt/rocm's copies first, a later `import torch` would find "No HIP GPUs".  Python callers use torch for HBM buffers and
    # streams anyway, so let it load its runtime first; the library then binds to the copies already in the process.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(path)
    vp, u32, u64, i32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int
    L.s5gpu_last_error.restype = C.c_char_p
    L.s5gpu_init.argtypes = [i32]
    L.s5gpu_init_mask.argtypes = [u64]
    L.s5gpu_devices_in_use.restype = i32
    L.s5gpu_recompress_batch.argtypes = [u32, vp, vp, i32, i32, i32, i32, vp, i32, vp, vp, vp]
    L.s5gpu_device_count.restype = i32
    L.s5gpu_slot_bound.restype = u64
    L.s5gpu_slot_bound.argtypes = [u32, u32, u32, i32, i32]
    L.s5gpu_payload_bound.restype = u64
    L.s5gpu_payload_bound.argtypes = [u32, u32, u32, i32]
    L.s5gpu_encode_dev.argtypes = [C.POINTER(EncodeArgs), vp]
    L.s5gpu_svbzd_encode_dev.argtypes = [C.POINTER(EncodeArgs), vp]
    L.s5gpu_decode_dev.argtypes = [C.POINTER(DecodeArgs), vp]
    L.s5gpu_compact_dev.argtypes = [u32, vp, vp, vp, vp, vp, vp, vp]
    L.s5gpu_synth_dev.argtypes = [vp, u64, u64, u64, u64, u64, vp]
    L.s5gpu_synth_hdr_dev.argtypes = [vp, u64, u64, vp]
    L.s5gpu_event_create.argtypes = [C.POINTER(vp)]
    L.s5gpu_event_record.argtypes = [vp, vp]
    L.s5gpu_event_elapsed_ms.argtypes = [vp, vp, C.POINTER(C.c_float)]
    L.s5gpu_event_destroy.argtypes = [vp]
    L.s5gpu_encode_batch.argtypes = [u32, vp, vp, vp, vp, vp, vp, i32, i32, vp, vp]
    L.s5gpu_decode_batch.argtypes = [u32, vp, vp, i32, i32, vp, vp, vp]
    L.s5gpu_encode_stream_dev.argtypes = [C.POINTER(EncodeArgs), vp, vp, vp, vp, vp]
    L.s5gpu_svbzd_encode_stream_dev.argtypes = [C.POINTER(EncodeArgs), vp, vp, vp, vp, vp]
    L.s5gpu_set_option.argtypes = [C.c_char_p, C.c_long]
    L.s5gpu_solo_batch.argtypes = [i32, u32, vp, vp, vp, vp, vp]
    L.s5gpu_deflate_parked_dev.argtypes = [C.POINTER(EncodeArgs), vp]
    L.s5gpu_pack_parked_dev.argtypes = [C.POINTER(EncodeArgs), vp]
    L.s5gpu_inflate_dev.argtypes = [C.POINTER(DecodeArgs), vp]
    L.s5gpu_svbzd_decode_dev.argtypes = [C.POINTER(DecodeArgs), vp]
    L.s5gpu_ascii_parse_dev.argtypes = [u32, vp, vp, vp, vp, vp]
    L.s5gpu_ascii_format_dev.argtypes = [u32, vp, vp, vp, vp, vp, vp]
    L.s5gpu_gather_dev.argtypes = [u32, vp, vp, vp, vp, vp, vp]
    L.s5gpu_aux_types_parse.argtypes = [C.c_char_p, C.c_size_t, vp, u32]
    L.s5gpu_ascii_to_blow5_batch.argtypes = [u32, vp, vp, u32, vp, i32, i32, vp, i32, vp, vp, vp]
    L.s5gpu_blow5_to_ascii_batch.argtypes = [u32, vp, vp, i32, i32, u32, vp, vp, i32, vp, vp, vp]
    L.s5gpu_ascii_to_ascii_batch.argtypes = [u32, vp, vp, u32, vp, vp, i32, vp, vp, vp]
    L.s5gpu_ascii_to_ascii_stream.argtypes = [u32, vp, C.c_size_t, vp, vp, u32, vp, vp, i32, vp, C.c_size_t, vp, vp]
    # degrade (qts rounding): the device entry and the _qts twins of the convert calls (trailing uint32_t qts_bits)
    L.s5gpu_qts_round_dev.argtypes = [vp, u32, vp, vp, u32, vp]
    L.s5gpu_recompress_batch_qts.argtypes = [u32, vp, vp, i32, i32, i32, i32, vp, i32, vp, vp, vp, u32]
    L.s5gpu_recompress_stream_qts.argtypes = [u32, vp, C.c_size_t, vp, vp, i32, i32, i32, i32, vp, i32, vp, C.c_size_t, vp, vp, u32]
    L.s5gpu_ascii_to_blow5_batch_qts.argtypes = [u32, vp, vp, u32, vp, i32, i32, vp, i32, vp, vp, vp, u32]
    L.s5gpu_ascii_to_blow5_stream_qts.argtypes = [u32, vp, C.c_size_t, vp, vp, u32, vp, i32, i32, vp, i32, vp, C.c_size_t, vp, vp, u32]
    L.s5gpu_blow5_to_ascii_batch_qts.argtypes = [u32, vp, vp, i32, i32, u32, vp, vp, i32, vp, vp, vp, u32]
    L.s5gpu_blow5_to_ascii_stream_qts.argtypes = [u32, vp, C.c_size_t, vp, vp, i32, i32, u32, vp, vp, i32, vp, C.c_size_t, vp, vp, u32]
    # skim: the header's layout, the chunk call and the pointer-array call
    L.s5gpu_skim_layout_parse.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(SkimLayout)]
    L.s5gpu_skim_stream.argtypes = [u32, vp, C.c_size_t, vp, vp, i32, i32, C.POINTER(SkimLayout), vp, C.c_size_t, vp, vp]
    L.s5gpu_skim_batch.argtypes = [u32, vp, vp, i32, i32, C.POINTER(SkimLayout), vp, vp, vp]
    # signals: statistics and normalised windows of decoded reads on the device, and the chunk call (q: a host array of doubles)
    L.s5gpu_signal_stats_dev.argtypes = [u32, vp, vp, vp, vp, u32, vp, vp, vp]
    L.s5gpu_signal_windows_dev.argtypes = [u32, vp, vp, vp, vp, vp, u32, vp, vp, u32, i32, C.c_double, C.c_double, i32, vp, vp, vp]
    L.s5gpu_signal_stats_stream.argtypes = [u32, vp, C.c_size_t, vp, vp, i32, i32, u32, vp, vp, vp]
    # sum: per-record content digests of decoded records on the device, of a file chunk and of records anywhere in host memory
    L.s5gpu_digest_dev.argtypes = [u32, vp, vp, vp, vp, i32, vp, vp]
    L.s5gpu_digest_stream.argtypes = [u32, vp, C.c_size_t, vp, vp, i32, i32, vp, vp]
    L.s5gpu_digest_batch.argtypes = [u32, vp, vp, i32, i32, vp, vp]
    # stats: the file-wide accumulator on the device, and the per-file handle of the chunk calls
    L.s5gpu_file_stats_bytes.restype = C.c_size_t
    L.s5gpu_file_stats_bytes.argtypes = []
    L.s5gpu_file_stats_reset_dev.argtypes = [vp, vp]
    L.s5gpu_file_stats_accum_dev.argtypes = [u32, vp, vp, vp, vp, vp, vp]
    L.s5gpu_file_stats_open.restype = vp
    L.s5gpu_file_stats_open.argtypes = []
    L.s5gpu_file_stats_add_stream.argtypes = [vp, u32, vp, C.c_size_t, vp, vp, i32, i32, vp]
    L.s5gpu_file_stats_close.argtypes = [vp, vp]
    # diff: two decoded batches compared pair by pair on the device, the accumulator, and the per-file handle
    L.s5gpu_diff_acc_bytes.restype = C.c_size_t
    L.s5gpu_diff_acc_bytes.argtypes = []
    L.s5gpu_diff_acc_reset_dev.argtypes = [vp, vp]
    L.s5gpu_signal_diff_dev.argtypes = [u32, vp, vp, C.POINTER(DiffSide), C.POINTER(DiffSide), vp, vp, vp]
    L.s5gpu_diff_open.restype = vp
    L.s5gpu_diff_open.argtypes = []
    L.s5gpu_diff_add_batch.argtypes = [vp, u32, vp, vp, i32, i32, vp, vp, i32, i32, vp, vp, vp]
    L.s5gpu_diff_close.argtypes = [vp, vp]
    # events: event segmentation of decoded reads on the device, and of records anywhere in host memory
    L.s5gpu_signal_events_dev.argtypes = [u32, vp, vp, vp, vp, C.POINTER(EventParams), i32, vp, vp, vp, vp, vp, vp]
    L.s5gpu_signal_events_batch.argtypes = [u32, vp, vp, i32, i32, C.POINTER(EventParams), i32, vp, C.c_size_t, vp, vp]
    # map: the quantiser on the host, the queries of event rows and sDTW on the device, and records anywhere in host memory
    L.s5gpu_quantise_host.argtypes = [vp, C.c_size_t, C.c_double, C.c_int32, vp]
    L.s5gpu_event_queries_dev.argtypes = [u32, vp, vp, vp, C.POINTER(MapParams), vp, vp, vp, vp]
    L.s5gpu_sdtw_dev.argtypes = [u32, vp, u32, vp, vp, u32, i32, vp, vp]
    L.s5gpu_map_batch.argtypes = [u32, vp, vp, i32, i32, C.POINTER(EventParams), C.POINTER(MapParams), vp, u32, vp, vp]
    # map with the second-best hit, and a reference from sequences and a k-mer model (host only)
    L.s5gpu_sdtw2_dev.argtypes = [u32, vp, u32, vp, vp, u32, i32, u32, vp, vp, vp]
    L.s5gpu_map2_batch.argtypes = [u32, vp, vp, i32, i32, C.POINTER(EventParams), C.POINTER(MapParams), vp, u32, u32, vp, vp, vp]
    L.s5gpu_kmer_model_load.argtypes = [C.c_char_p, C.POINTER(C.POINTER(C.c_float)), C.POINTER(u32)]
    L.s5gpu_kmer_model_free.argtypes = [C.POINTER(C.c_float)]
    L.s5gpu_kmer_model_free.restype = None
    L.s5gpu_refseq_build.restype = vp
    L.s5gpu_refseq_build.argtypes = [u32, vp, vp, vp, vp, u32, i32, i32, C.c_double, i32]
    L.s5gpu_refseq_open.restype = vp
    L.s5gpu_refseq_open.argtypes = [C.c_char_p, C.c_char_p, i32, i32, C.c_double, i32]
    L.s5gpu_refseq_ref.restype = vp
    L.s5gpu_refseq_ref.argtypes = [vp, C.POINTER(u32)]
    L.s5gpu_refseq_n_segments.restype = u32
    L.s5gpu_refseq_n_segments.argtypes = [vp]
    L.s5gpu_refseq_n_contigs.restype = u32
    L.s5gpu_refseq_n_contigs.argtypes = [vp]
    L.s5gpu_refseq_segment.argtypes = [vp, u32, C.POINTER(RefSeqSegment)]
    L.s5gpu_refseq_contig.argtypes = [vp, u32, C.POINTER(C.c_char_p), C.POINTER(C.c_uint64), C.POINTER(u32)]
    L.s5gpu_refseq_params.argtypes = [vp, C.POINTER(u32), C.POINTER(u32), C.POINTER(i32)]
    L.s5gpu_refseq_locate.argtypes = [vp, u32, C.POINTER(RefSeqLoc)]
    L.s5gpu_refseq_close.argtypes = [vp]
    L.s5gpu_refseq_close.restype = None
    # align: the scratch a read's path needs, the paths of mapped queries on the device, and records anywhere in host memory
    L.s5gpu_sdtw_path_slot_bytes.argtypes = [u32, u32]
    L.s5gpu_sdtw_path_slot_bytes.restype = C.c_size_t
    L.s5gpu_sdtw_path_dev.argtypes = [u32, vp, u32, vp, vp, u32, vp, u32, vp, C.c_size_t, vp, vp, vp, vp]
    L.s5gpu_align_batch.argtypes = [u32, vp, vp, i32, i32, C.POINTER(EventParams), C.POINTER(MapParams), u32, vp, u32, vp, vp, vp, vp, vp]
    # pileup: the per-reference-position table on the device, and the per-file handle
    L.s5gpu_pileup_bytes.argtypes = [u32]
    L.s5gpu_pileup_bytes.restype = C.c_size_t
    L.s5gpu_pileup_reset_dev.argtypes = [vp, u32, vp]
    L.s5gpu_pileup_accum_dev.argtypes = [u32, vp, u32, vp, vp, u32, vp, vp, vp, vp, vp, vp]
    L.s5gpu_pileup_open.restype = vp
    L.s5gpu_pileup_open.argtypes = [C.POINTER(EventParams), C.POINTER(MapParams), u32, vp, u32]
    L.s5gpu_pileup_add_batch.argtypes = [vp, u32, vp, vp, i32, i32, vp, vp]
    L.s5gpu_pileup_close.argtypes = [vp, vp]
    # refine: the fit along a path, the windowed realign, their rounds on the device, and records anywhere in host memory
    L.s5gpu_path_fit_dev.argtypes = [u32, vp, u32, vp, vp, u32, vp, vp, vp, u32, C.POINTER(RefineParams), vp, vp, vp, vp]
    L.s5gpu_sdtw_window_dev.argtypes = [u32, vp, u32, vp, vp, u32, vp, u32, u32, vp, C.c_size_t, vp, vp, vp, vp, vp]
    L.s5gpu_refine_work_bytes.argtypes = [u32, u32]
    L.s5gpu_refine_work_bytes.restype = C.c_size_t
    L.s5gpu_refine_dev.argtypes = [u32, vp, u32, vp, vp, u32, vp, vp, vp, vp, u32, C.POINTER(RefineParams), vp, C.c_size_t, vp, C.c_size_t, vp, vp, vp, vp, vp,
                                   vp, vp, vp]
    L.s5gpu_refine_batch.argtypes = [u32, vp, vp, i32, i32, C.POINTER(EventParams), C.POINTER(MapParams), u32, C.POINTER(RefineParams), vp, u32, vp, vp, vp,
                                     vp, vp, vp, vp, vp]
    # extend: the long queries of event rows, and the banded alignment in tiles from an anchor, on the device
    L.s5gpu_event_queries_long_dev.argtypes = [u32, vp, vp, vp, C.POINTER(BandParams), u64, vp, vp, vp, vp]
    L.s5gpu_sdtw_band_scratch_bytes.argtypes = [u32, u64, u32, u32]
    L.s5gpu_sdtw_band_scratch_bytes.restype = C.c_size_t
    L.s5gpu_sdtw_band_dev.argtypes = [u32, vp, vp, vp, u64, vp, u32, vp, vp, C.POINTER(BandParams), vp, C.c_size_t, vp, vp, vp, vp]
    L.s5gpu_extend_batch.argtypes = [u32, vp, vp, i32, i32, C.POINTER(EventParams), C.POINTER(MapParams), C.POINTER(BandParams), C.c_size_t, vp, u32, vp, vp,
                                     vp, vp, vp, vp, C.c_size_t, vp]
    # pileup of whole reads: the ragged call, and the per-file handle over extend's chain
    L.s5gpu_pileup_long_work_bytes.argtypes = [u32, u64]
    L.s5gpu_pileup_long_work_bytes.restype = C.c_size_t
    L.s5gpu_pileup_accum_long_dev.argtypes = [u32, vp, vp, vp, u64, vp, u32, vp, vp, vp, vp, u32, vp, C.c_size_t, vp, vp]
    L.s5gpu_pileup_open_whole.restype = vp
    L.s5gpu_pileup_open_whole.argtypes = [C.POINTER(EventParams), C.POINTER(MapParams), C.POINTER(BandParams), C.c_size_t, vp, u32]
    L.s5gpu_pileup_add_batch_whole.argtypes = [vp, u32, vp, vp, i32, i32, vp, vp, vp]
    # contrast: per-position level histograms, the comparison of two, and the per-file handle with two sides
    L.s5gpu_pile_hist_bytes.argtypes = [u32]
    L.s5gpu_pile_hist_bytes.restype = C.c_size_t
    L.s5gpu_pile_hist_reset_dev.argtypes = [vp, u32, i32, u32, vp]
    L.s5gpu_pile_hist_accum_long_dev.argtypes = [u32, vp, vp, vp, u64, u32, vp, vp, vp, vp, C.c_size_t, vp, vp]
    L.s5gpu_pile_contrast_dev.argtypes = [vp, vp, vp, vp, u32, vp, vp]
    L.s5gpu_contrast_open.restype = vp
    L.s5gpu_contrast_open.argtypes = [C.POINTER(EventParams), C.POINTER(MapParams), C.POINTER(BandParams), C.c_size_t, vp, u32, i32, u32]
    L.s5gpu_contrast_add_batch.argtypes = [vp, i32, u32, vp, vp, i32, i32, vp, vp, vp]
    L.s5gpu_contrast_close.argtypes = [vp, vp, vp, vp]
    # refine, whole reads: the fit along ragged paths, the rounds of the banded alignment, the chain, and the switch of the whole-read handles
    L.s5gpu_path_fit_long_work_bytes.argtypes = [u32, u64]
    L.s5gpu_path_fit_long_work_bytes.restype = C.c_size_t
    L.s5gpu_path_fit_long_dev.argtypes = [u32, vp, vp, vp, u64, vp, u32, vp, vp, vp, C.POINTER(RefineParams), vp, C.c_size_t, vp, vp, vp, vp]
    L.s5gpu_extend_refine_work_bytes.argtypes = [u32, u64]
    L.s5gpu_extend_refine_work_bytes.restype = C.c_size_t
    L.s5gpu_extend_refine_dev.argtypes = [u32, vp, vp, vp, u64, vp, u32, vp, vp, vp, C.POINTER(BandParams), C.POINTER(RefineParams), vp, C.c_size_t, vp,
                                          C.c_size_t, vp, vp, vp, vp, vp, vp, vp]
    L.s5gpu_extend_refine_batch.argtypes = [u32, vp, vp, i32, i32, C.POINTER(EventParams), C.POINTER(MapParams), C.POINTER(BandParams), C.POINTER(RefineParams),
                                            C.c_size_t, vp, u32, vp, vp, vp, vp, vp, vp, vp, vp, C.c_size_t, vp, vp, vp]
    L.s5gpu_pileup_set_refine.argtypes = [vp, C.POINTER(RefineParams)]
    L.s5gpu_contrast_set_refine.argtypes = [vp, C.POINTER(RefineParams)]
    # sites: the read x site matrix of a ragged batch, its scores against a control histogram, and the per-file handle
    L.s5gpu_site_cells_long_dev.argtypes = [u32, vp, vp, vp, u64, u32, vp, vp, vp, vp, u32, vp, C.c_size_t, vp, vp, vp]
    L.s5gpu_site_score_dev.argtypes = [vp, u32, vp, u32, vp, u32, vp, vp]
    L.s5gpu_sites_open.restype = vp
    L.s5gpu_sites_open.argtypes = [C.POINTER(EventParams), C.POINTER(MapParams), C.POINTER(BandParams), C.c_size_t, vp, u32, vp, u32, i32, u32]
    L.s5gpu_sites_set_refine.argtypes = [vp, C.POINTER(RefineParams)]
    L.s5gpu_sites_add_control.argtypes = [vp, u32, vp, vp, i32, i32, vp]
    L.s5gpu_sites_set_control.argtypes = [vp, vp]
    L.s5gpu_sites_add_batch.argtypes = [vp, u32, vp, vp, i32, i32, vp, vp, vp, vp]
    L.s5gpu_sites_close.argtypes = [vp, vp]
    # model: a reference's classes and quantiser, the fold of a table and a histogram onto classes, the folded closes, and the estimate
    L.s5gpu_quant_stats_host.argtypes = [vp, C.c_size_t, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.s5gpu_refseq_classes.argtypes = [vp, vp, C.POINTER(u32)]
    L.s5gpu_refseq_quant.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.s5gpu_pileup_fold_dev.argtypes = [vp, u32, vp, u32, vp, vp]
    L.s5gpu_pile_hist_fold_dev.argtypes = [vp, u32, vp, u32, vp, vp]
    L.s5gpu_pileup_close_folded.argtypes = [vp, vp, u32, vp]
    L.s5gpu_contrast_close_folded.argtypes = [vp, vp, u32, vp, vp, vp]
    L.s5gpu_kmer_model_solve.argtypes = [vp, u32, C.c_double, C.c_double, C.c_double, u32, vp, vp]
    _LIB = L
    return L


def check(rc, what=""):
    if rc != 0:
        msg = lib().s5gpu_last_error().decode(errors="replace")
        raise S5GpuError("%s failed (rc=%d): %s" % (what or "libslow5gpu call", rc, msg))


EXPORTS = [
    "s5gpu_init", "s5gpu_init_mask", "s5gpu_devices_in_use", "s5gpu_shutdown", "s5gpu_last_error", "s5gpu_device_count", "s5gpu_slot_bound", "s5gpu_payload_bound",
    "s5gpu_encode_dev", "s5gpu_decode_dev", "s5gpu_svbzd_encode_dev", "s5gpu_compact_dev", "s5gpu_synth_dev",
    "s5gpu_synth_hdr_dev", "s5gpu_event_create", "s5gpu_event_record", "s5gpu_event_elapsed_ms", "s5gpu_event_destroy",
    "s5gpu_encode_batch", "s5gpu_decode_batch", "s5gpu_solo_batch", "s5gpu_deflate_parked_dev", "s5gpu_inflate_dev",
    "s5gpu_svbzd_decode_dev", "s5gpu_set_option", "s5gpu_recompress_batch", "s5gpu_patch_u32_dev", "s5gpu_encode_stream_dev",
    "s5gpu_svbzd_encode_stream_dev", "s5gpu_pack_parked_dev", "s5gpu_warmup",
    "s5gpu_signal_stats_dev", "s5gpu_signal_windows_dev", "s5gpu_signal_stats_stream",
    "s5gpu_digest_dev", "s5gpu_digest_stream", "s5gpu_digest_batch",
    "s5gpu_file_stats_bytes", "s5gpu_file_stats_reset_dev", "s5gpu_file_stats_accum_dev", "s5gpu_file_stats_open", "s5gpu_file_stats_add_stream",
    "s5gpu_file_stats_close",
    "s5gpu_diff_acc_bytes", "s5gpu_diff_acc_reset_dev", "s5gpu_signal_diff_dev", "s5gpu_diff_open", "s5gpu_diff_add_batch", "s5gpu_diff_close",
    "s5gpu_signal_events_dev", "s5gpu_signal_events_batch",
    "s5gpu_quantise_host", "s5gpu_event_queries_dev", "s5gpu_sdtw_dev", "s5gpu_map_batch",
    "s5gpu_sdtw2_dev", "s5gpu_map2_batch", "s5gpu_kmer_model_load", "s5gpu_kmer_model_free", "s5gpu_refseq_build", "s5gpu_refseq_open", "s5gpu_refseq_ref",
    "s5gpu_refseq_n_segments", "s5gpu_refseq_segment", "s5gpu_refseq_n_contigs", "s5gpu_refseq_contig", "s5gpu_refseq_params", "s5gpu_refseq_locate",
    "s5gpu_refseq_close",
    "s5gpu_sdtw_path_slot_bytes", "s5gpu_sdtw_path_dev", "s5gpu_align_batch",
    "s5gpu_pileup_bytes", "s5gpu_pileup_reset_dev", "s5gpu_pileup_accum_dev", "s5gpu_pileup_open", "s5gpu_pileup_add_batch", "s5gpu_pileup_close",
    "s5gpu_path_fit_dev", "s5gpu_sdtw_window_dev", "s5gpu_refine_work_bytes", "s5gpu_refine_dev", "s5gpu_refine_batch",
    "s5gpu_event_queries_long_dev", "s5gpu_sdtw_band_scratch_bytes", "s5gpu_sdtw_band_dev", "s5gpu_extend_batch",
    "s5gpu_pileup_long_work_bytes", "s5gpu_pileup_accum_long_dev", "s5gpu_pileup_open_whole", "s5gpu_pileup_add_batch_whole",
    "s5gpu_pile_hist_bytes", "s5gpu_pile_hist_reset_dev", "s5gpu_pile_hist_accum_long_dev", "s5gpu_pile_contrast_dev", "s5gpu_contrast_open",
    "s5gpu_contrast_add_batch", "s5gpu_contrast_close",
    "s5gpu_path_fit_long_work_bytes", "s5gpu_path_fit_long_dev", "s5gpu_extend_refine_work_bytes", "s5gpu_extend_refine_dev", "s5gpu_extend_refine_batch",
    "s5gpu_pileup_set_refine", "s5gpu_contrast_set_refine",
    "s5gpu_site_cells_long_dev", "s5gpu_site_score_dev", "s5gpu_sites_open", "s5gpu_sites_set_refine", "s5gpu_sites_add_control", "s5gpu_sites_set_control",
    "s5gpu_sites_add_batch", "s5gpu_sites_close",
    "s5gpu_quant_stats_host", "s5gpu_refseq_classes", "s5gpu_refseq_quant", "s5gpu_pileup_fold_dev", "s5gpu_pile_hist_fold_dev", "s5gpu_pileup_close_folded",
    "s5gpu_contrast_close_folded", "s5gpu_kmer_model_solve",
]
