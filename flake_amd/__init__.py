"""flake_amd -- MI355X-native FLAC prediction/entropy path behind libflake's
``flake_encode_frame()`` surface.

This package is only the Python view (ctypes) of two native libraries:

* ``lib/libflakehip.so``  -- gfx950 kernels + the C ABI of ``include/flakehip.h``
* ``lib/libflake_amd.so`` -- the host C layer of ``include/flake_amd.h``

There is no Python or CPU implementation of the path here: if the HIP library
is missing, importing the encoder fails loudly.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_DIR = os.path.join(_HERE, "lib")

MAX_ORDER = 32
MAX_PARTS = 256
MAX_LAGS = 33
MAX_BLOCK = 65535

OK, E_GENERIC, E_HIP, E_UNSUPPORTED, E_INVALID, E_NOMEM, E_VERIFY = 0, -1, -2, -3, -4, -5, -6
PCM_S32, PCM_S16 = 0, 1      # FHIP_PCM_*: what a handle's pcm pointers address (fhip_set_pcm_format)

SUB_CONSTANT, SUB_VERBATIM, SUB_FIXED, SUB_LPC = 0, 1, 8, 32
CH_NOT_STEREO, CH_LEFT_RIGHT, CH_LEFT_SIDE, CH_RIGHT_SIDE, CH_MID_SIDE = 0, 1, 8, 9, 10

# FLAKE_ORDER_METHOD_* (flake.h:38-46), FLAKE_PREDICTION_* (flake.h:53-57)
OM_MAX, OM_EST, OM_2LEVEL, OM_4LEVEL, OM_8LEVEL, OM_SEARCH, OM_LOG = range(7)
PRED_NONE, PRED_FIXED, PRED_LEVINSON = range(3)
STEREO_INDEPENDENT, STEREO_ESTIMATE = range(2)


class Params(C.Structure):
    """``fhip_params``: the fields of FlakeContext/FlakeEncodeParams the path reads."""
    _fields_ = [(k, C.c_int) for k in (
        "channels", "sample_rate", "bits_per_sample", "block_size", "order_method",
        "stereo_method", "prediction_type", "min_prediction_order", "max_prediction_order",
        "min_partition_order", "max_partition_order", "variable_block_size", "allow_vbs",
        "lpc_precision")]

    def copy(self) -> "Params":
        q = Params()
        C.memmove(C.byref(q), C.byref(self), C.sizeof(Params))
        return q

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_}


def level_params(level: int, channels: int = 2, bits_per_sample: int = 16,
                 sample_rate: int = 44100, **over) -> Params:
    """Compression-level presets, the table of flake_set_defaults() (encode.c:158-266)."""
    if not 0 <= level <= 12:
        raise ValueError("compression level must be 0..12")
    p = Params(channels=channels, sample_rate=sample_rate, bits_per_sample=bits_per_sample,
               block_size=4096, order_method=OM_EST, stereo_method=STEREO_ESTIMATE,
               prediction_type=PRED_LEVINSON, min_prediction_order=1, max_prediction_order=8,
               min_partition_order=0, max_partition_order=5, variable_block_size=0,
               allow_vbs=0, lpc_precision=15)
    if level <= 2:
        p.block_size = 1152
        p.prediction_type = PRED_FIXED
        p.min_prediction_order = (2, 2, 0)[level]
        p.max_prediction_order = (2, 4, 4)[level]
        p.max_partition_order = 3
        if level == 0:
            p.stereo_method = STEREO_INDEPENDENT
    elif level == 3:
        p.stereo_method = STEREO_INDEPENDENT
        p.max_prediction_order = 6
        p.max_partition_order = 4
    elif level == 4:
        p.max_partition_order = 4
    elif level in (6, 7):
        p.max_partition_order = 6
        if level == 7:
            p.order_method = OM_4LEVEL
    elif level >= 8:
        p.order_method = OM_SEARCH if level in (10, 12) else OM_LOG
        p.max_prediction_order = 32 if level >= 11 else 12
        p.max_partition_order = 6 if level == 8 else 8
        if level >= 11:
            p.block_size = 8192
        if level >= 9:
            p.allow_vbs = 1
            p.variable_block_size = 1
    for k, v in over.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, v)
    return p


# numpy view of fhip_subframe_info (1328 bytes)
INFO_DTYPE = np.dtype([
    ("type", "<i4"), ("type_code", "<i4"), ("order", "<i4"), ("shift", "<i4"),
    ("obits", "<i4"), ("wasted", "<i4"), ("rice_method", "<i4"), ("porder", "<i4"),
    ("est_bits", "<u4"), ("ch_mode", "<i4"), ("rice_nbits", "<i4"), ("reserved", "<i4"),
    ("coefs", "<i4", (MAX_ORDER,)), ("rparams", "<i4", (MAX_PARTS,)),
    ("warmup", "<i4", (MAX_ORDER,)),
])
assert INFO_DTYPE.itemsize == 1328


class Batch(C.Structure):
    """``fhip_batch``"""
    _fields_ = [
        ("pcm", C.c_void_p), ("nframes", C.c_int), ("block_size", C.c_int),
        ("info", C.c_void_p), ("residual", C.c_void_p), ("rice_bits", C.c_void_p),
        ("rice_slot_bytes", C.c_int64), ("samples", C.c_void_p), ("autoc", C.c_void_p),
        ("frames", C.c_void_p), ("frame_stride", C.c_int64), ("frame_bytes", C.c_void_p),
        ("first_frame_number", C.c_uint32), ("frame_numbers", C.c_void_p),
    ]


class VbsOut(C.Structure):
    """``fhip_vbs_out`` (device pointers)"""
    _fields_ = [("packed", C.c_void_p), ("packed_cap", C.c_int64), ("frame_bytes", C.c_void_p),
                ("block_bytes", C.c_void_p), ("block_frames", C.c_void_p), ("totals", C.c_void_p)]


class VerifyIn(C.Structure):
    """``fhip_verify_in``"""
    _fields_ = [("stream", C.c_void_p), ("stream_bytes", C.c_int64), ("frame_bytes", C.c_void_p),
                ("nframes", C.c_int32), ("pcm", C.c_void_p), ("nsamples", C.c_int64), ("first_sample", C.c_int64)]


class VerifyOut(C.Structure):
    """``fhip_verify_out``"""
    _fields_ = [("frames", C.c_void_p), ("summary", C.c_void_p)]


class DecodeIn(C.Structure):
    """``fhip_decode_in``"""
    _fields_ = [("stream", C.c_void_p), ("stream_bytes", C.c_int64), ("frame_bytes", C.c_void_p),
                ("nframes", C.c_int32), ("variable_blocks", C.c_int32), ("first_number", C.c_int64)]


class DecodeOut(C.Structure):
    """``fhip_decode_out``"""
    _fields_ = [("pcm", C.c_void_p), ("pcm_cap", C.c_int64), ("frames", C.c_void_p), ("summary", C.c_void_p),
                ("nsamples", C.c_void_p)]


class DecodeSegments(C.Structure):
    """``fhip_decode_segments``"""
    _fields_ = [("seg_first", C.c_void_p), ("nsegs", C.c_int32), ("seg_number", C.c_void_p),
                ("seg_variable", C.c_void_p), ("seg_start", C.c_void_p), ("seg_samples", C.c_void_p),
                ("seg_failed", C.c_void_p)]


class DecodeWindows(C.Structure):
    """``fhip_decode_windows``"""
    _fields_ = [("seg_skip", C.c_void_p), ("seg_take", C.c_void_p)]


class RowsOut(C.Structure):
    """``fhip_rows_out``"""
    _fields_ = [("rows", C.c_void_p), ("nrows", C.c_int32), ("format", C.c_int32), ("row_len", C.c_int64)]


# FHIP_ROWS_* / FLAKE_AMD_ROWS_*: what an element of a row is
ROWS_I32, ROWS_I16, ROWS_F32 = 0, 1, 2


class SpanRows(C.Structure):
    """``fhip_span_rows``: K13's tables -- every segment's span's first row, its rows and the segment's position in it --
    with the hop, and for the device entry the CSR of the tiles"""
    _fields_ = [("seg_row0", C.c_void_p), ("seg_nrows", C.c_void_p), ("seg_pos", C.c_void_p), ("hop", C.c_int64),
                ("tile_first", C.c_void_p), ("ntiles", C.c_int32)]


class RowsIn(C.Structure):
    """``fhip_rows_in``"""
    _fields_ = [("rows", C.c_void_p), ("nrows", C.c_int32), ("format", C.c_int32), ("row_len", C.c_int64)]


class RowPiece(C.Structure):
    """``fhip_row_piece``: count samples per channel from column col of row `row` to sample dst of the destination"""
    _fields_ = [("row", C.c_int32), ("count", C.c_int32), ("col", C.c_int64), ("dst", C.c_int64)]


# numpy view of fhip_row_piece (24 bytes): K12's unit, in samples per channel
ROW_PIECE_DTYPE = np.dtype([("row", "<i4"), ("count", "<i4"), ("col", "<i8"), ("dst", "<i8")])
assert ROW_PIECE_DTYPE.itemsize == 24 == C.sizeof(RowPiece)


def row_pieces(rows) -> np.ndarray:
    """[(row, col, dst, count)] as a fhip_row_piece table."""
    t = np.zeros(len(rows), dtype=ROW_PIECE_DTYPE)
    for k, (row, col, dst, count) in enumerate(rows):
        t[k] = (row, count, col, dst)
    return t


class IndexIn(C.Structure):
    """``fhip_index_in``"""
    _fields_ = [("stream", C.c_void_p), ("stream_bytes", C.c_int64), ("range_first", C.c_void_p),
                ("nranges", C.c_int32), ("max_block_size", C.c_int32), ("frame_cap", C.c_int32)]


class IndexOut(C.Structure):
    """``fhip_index_out``"""
    _fields_ = [("frame_bytes", C.c_void_p), ("range_frames", C.c_void_p), ("range_consumed", C.c_void_p),
                ("range_variable", C.c_void_p)]


# numpy view of fhip_frame_head (16 bytes): what a frame's header says.  flags: bit 0 ok, bit 1 variable block size,
# bits 8..15 the header's length
FRAME_HEAD_DTYPE = np.dtype([("number", "<u8"), ("n", "<i4"), ("flags", "<i4")])
assert FRAME_HEAD_DTYPE.itemsize == 16


class DecodeMd5(C.Structure):
    """``fhip_decode_md5``"""
    _fields_ = [("states", C.c_void_p), ("nstreams", C.c_int32), ("seg_stream", C.c_void_p)]


# numpy view of fhip_md5_state (96 bytes): K6's running hash of one stream
MD5_STATE_DTYPE = np.dtype([("h", "<u4", (4,)), ("nbytes", "<u8"), ("fill", "<u4"), ("reserved", "<u4"),
                            ("tail", "u1", (64,))])
assert MD5_STATE_DTYPE.itemsize == 96
MD5_STATE_BYTES = 96


# FHIP_VERIFY_*: a frame's status, the first failing check in stream order
VERIFY_STATUS = ("OK", "HEADER", "CRC8", "NUMBER", "SYNTAX", "SAMPLES", "PADDING", "CRC16", "LENGTH")
(V_OK, V_HEADER, V_CRC8, V_NUMBER, V_SYNTAX, V_SAMPLES, V_PADDING, V_CRC16, V_LENGTH) = range(9)
# fhip_verify_rec
VERIFY_REC_DTYPE = np.dtype([("status", "<i4"), ("bit", "<i4"), ("subframe", "<i4"), ("sample", "<i4")])


class FlakeHipError(RuntimeError):
    def __init__(self, code: int, what: str, detail: str = ""):
        self.code = code
        super().__init__(f"{what}: {code} ({detail})" if detail else f"{what}: {code}")


_lib = None


def load_library() -> C.CDLL:
    """Load libflakehip.so; raises if it has not been built (no fallback exists)."""
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get("FHIP_LIB") or os.path.join(LIB_DIR, "libflakehip.so")
    if not os.path.exists(path):
        raise ImportError(
            f"{path} is missing: build it with `python -m flake_amd.build` "
            "(the HIP library is the only implementation of this path)")
    lib = C.CDLL(path)
    vp, i, i64 = C.c_void_p, C.c_int, C.c_int64
    sig = {
        "fhip_device_count": (i, []),
        "fhip_frame_stride": (i64, [C.POINTER(Params), i]),
        "fhip_create": (i, [C.POINTER(vp), i, C.POINTER(Params), i]),
        "fhip_destroy": (None, [vp]),
        "fhip_set_stream": (i, [vp, vp]),
        "fhip_sync": (i, [vp]),
        "fhip_set_pcm_format": (i, [vp, i]),
        "fhip_strerror": (C.c_char_p, [i]),
        "fhip_last_error": (C.c_char_p, [vp]),
        "fhip_version": (C.c_char_p, []),
        "fhip_encode_subframes_dev": (i, [vp, C.POINTER(Batch)]),
        "fhip_encode_subframes": (i, [vp, C.POINTER(Batch)]),
        "fhip_prepare_ahead": (i, [vp, C.POINTER(Batch)]),
        "fhip_encode_frames_packed": (i, [vp, C.POINTER(Batch), vp, i64, C.POINTER(i64)]),
        "fhip_frames_packed_begin": (i, [vp, C.POINTER(Batch), C.POINTER(i64)]),
        "fhip_frames_packed_fetch": (i, [vp, vp, i64]),
        "fhip_encode_blocks_vbs_packed": (i, [vp, vp, i, i, C.c_uint32, vp, i64, vp, vp, C.POINTER(i64),
                                              C.POINTER(i), C.POINTER(C.c_uint32)]),
        "fhip_encode_blocks_vbs_dev": (i, [vp, vp, i, i, C.c_uint32, C.POINTER(VbsOut)]),
        "fhip_lpc_calc_coefs": (i, [vp, vp, i, i, i, i, i, vp, vp, vp, vp]),
        "fhip_encode_residual": (i, [vp, vp, i, i, vp, vp, vp, i64]),
        "fhip_order_search_bits": (i, [vp, vp, i, i, vp, vp]),
        "fhip_prepare_frames": (i, [vp, vp, i, i, vp, vp]),
        "fhip_calc_rice_params": (i, [vp, vp, i, i, i, i, i, i, i, vp, vp, i64]),
        "fhip_vbs_split": (i, [vp, vp, i, i, vp, vp]),
        "fhip_set_profiling": (i, [vp, i]),
        "fhip_set_verify": (i, [vp, i]),
        "fhip_verify_frames_dev": (i, [vp, C.POINTER(VerifyIn), C.POINTER(VerifyOut)]),
        "fhip_verify_frames": (i, [vp, C.POINTER(VerifyIn), C.POINTER(VerifyOut)]),
        "fhip_verify_frames_numbered_dev": (i, [vp, C.POINTER(VerifyIn), vp, C.POINTER(VerifyOut)]),
        "fhip_verify_frames_numbered": (i, [vp, C.POINTER(VerifyIn), vp, C.POINTER(VerifyOut)]),
        "fhip_last_verify_failure": (i, [vp, vp, vp]),
        "fhip_decode_frames_dev": (i, [vp, C.POINTER(DecodeIn), C.POINTER(DecodeOut)]),
        "fhip_decode_frames": (i, [vp, C.POINTER(DecodeIn), C.POINTER(DecodeOut)]),
        "fhip_decode_frames_segments_dev": (i, [vp, C.POINTER(DecodeIn), C.POINTER(DecodeSegments),
                                                C.POINTER(DecodeOut)]),
        "fhip_decode_frames_segments": (i, [vp, C.POINTER(DecodeIn), C.POINTER(DecodeSegments), C.POINTER(DecodeOut),
                                            C.POINTER(DecodeMd5)]),
        "fhip_md5_update_ranges_dev": (i, [vp, vp, i, vp, vp, vp, vp, vp]),
        "fhip_index_frames_dev": (i, [vp, C.POINTER(IndexIn), C.POINTER(IndexOut)]),
        "fhip_index_frames": (i, [vp, C.POINTER(IndexIn), C.POINTER(IndexOut)]),
        "fhip_index_geometry": (None, [C.POINTER(i), C.POINTER(i), C.POINTER(i), C.POINTER(i)]),
        "fhip_get_kernel_times": (i, [vp, C.POINTER(C.c_char_p), C.POINTER(C.c_double),
                                      C.POINTER(i), i, i]),
        "fhip_last_launches": (i, [vp, C.POINTER(C.c_char_p), i]),
        "fhip_md5_init_dev": (i, [vp, vp, i]),
        "fhip_md5_update_dev": (i, [vp, vp, i, vp, i, vp, vp]),
        "fhip_md5_final_dev": (i, [vp, vp, i, vp]),
        "fhip_md5_final": (i, [vp, vp, i, vp]),
        "fhip_md5_update_uploaded": (i, [vp, vp, i, i, i, vp, vp]),
        "fhip_frames_packed_upload": (i, [vp, C.POINTER(Batch)]),
        "fhip_frames_packed_upload_ragged": (i, [vp, C.POINTER(Batch), vp]),
        "fhip_frames_packed_begin_ragged": (i, [vp, C.POINTER(Batch), vp, C.POINTER(i64)]),
        "fhip_md5_update_uploaded_ragged": (i, [vp, vp, i, i, vp, vp, vp]),
        "fhip_verify_frames_ragged_dev": (i, [vp, C.POINTER(VerifyIn), vp, vp, vp, C.POINTER(VerifyOut)]),
        "fhip_verify_frames_ragged": (i, [vp, C.POINTER(VerifyIn), vp, vp, C.POINTER(VerifyOut)]),
        "fhip_encode_blocks_vbs_packed_numbered": (i, [vp, vp, i, i, vp, vp, i64, vp, vp, vp, C.POINTER(i64)]),
        "fhip_set_block_numbering": (i, [vp, i]),
        "fhip_verify_frames_blocks_dev": (i, [vp, C.POINTER(VerifyIn), vp, i, i, C.POINTER(VerifyOut)]),
        "fhip_verify_frames_blocks": (i, [vp, C.POINTER(VerifyIn), vp, i, i, C.POINTER(VerifyOut)]),
        "fhip_last_verify_number": (i, [vp, C.POINTER(C.c_uint32)]),
        "fhip_encode_blocks_vbs_ragged_numbered": (i, [vp, vp, i, vp, vp, vp, i64, vp, vp, vp, C.POINTER(i64)]),
        "fhip_vbs_split_ragged": (i, [vp, vp, i, vp, vp, vp]),
        "fhip_verify_frames_blocks_ragged_dev": (i, [vp, C.POINTER(VerifyIn), vp, i, vp, C.POINTER(VerifyOut)]),
        "fhip_verify_frames_blocks_ragged": (i, [vp, C.POINTER(VerifyIn), vp, i, vp, C.POINTER(VerifyOut)]),
        "fhip_device_alloc": (vp, [C.c_size_t]),
        "fhip_device_free": (None, [vp]),
        "fhip_autocorr_tile": (i, [i, i, i]),
        "fhip_gather_spans_dev": (i, [vp, vp, i64, vp, i64, vp, i64, vp, i]),
        "fhip_frames_packed_gather": (i, [vp, C.POINTER(Batch), vp, vp, i64, vp, i64, vp, i]),
        "fhip_decode_frames_windows_dev": (i, [vp, C.POINTER(DecodeIn), C.POINTER(DecodeSegments),
                                               C.POINTER(DecodeWindows), C.POINTER(DecodeOut)]),
        "fhip_decode_frames_windows": (i, [vp, C.POINTER(DecodeIn), C.POINTER(DecodeSegments), C.POINTER(DecodeWindows),
                                           C.POINTER(DecodeOut)]),
        "fhip_decode_frames_segments_keep": (i, [vp, C.POINTER(DecodeIn), C.POINTER(DecodeSegments), C.POINTER(DecodeOut),
                                                 C.POINTER(DecodeMd5)]),
        "fhip_rows_from_segments_dev": (i, [vp, vp, i64, C.c_int32, vp, vp, vp, vp, vp, C.POINTER(RowsOut)]),
        "fhip_rows_zero_dev": (i, [vp, C.POINTER(RowsOut), C.c_int32, C.c_int32]),
        "fhip_decode_frames_windows_rows": (i, [vp, C.POINTER(DecodeIn), C.POINTER(DecodeSegments),
                                                C.POINTER(DecodeWindows), vp, vp, C.POINTER(RowsOut),
                                                C.POINTER(DecodeOut)]),
        "fhip_frame_heads_dev": (i, [vp, vp, i64, vp, vp, C.c_int32, C.c_int32, vp]),
        "fhip_gather_frames_dev": (i, [vp, vp, i64, vp, vp, i64, vp, vp, C.c_int32]),
        "fhip_decode_frames_windows_held": (i, [vp, vp, i64, vp, vp, C.c_int32, C.POINTER(DecodeSegments),
                                                C.POINTER(DecodeWindows), C.POINTER(DecodeOut)]),
        "fhip_decode_frames_windows_rows_held": (i, [vp, vp, i64, vp, vp, C.c_int32, C.POINTER(DecodeSegments),
                                                     C.POINTER(DecodeWindows), vp, vp, C.POINTER(RowsOut),
                                                     C.POINTER(DecodeOut)]),
        "fhip_hold_frames": (i, [vp, vp, vp]),
        "fhip_pcm_from_rows_dev": (i, [vp, vp, i64, C.POINTER(RowsIn), vp, i]),
        "fhip_frames_packed_from_rows": (i, [vp, C.POINTER(Batch), vp, C.POINTER(RowsIn), vp, i]),
        "fhip_span_rows_from_segments_dev": (i, [vp, vp, i64, C.c_int32, vp, vp, vp, C.POINTER(SpanRows),
                                                 C.POINTER(RowsOut)]),
        "fhip_decode_frames_windows_spans": (i, [vp, C.POINTER(DecodeIn), C.POINTER(DecodeSegments),
                                                 C.POINTER(DecodeWindows), C.POINTER(SpanRows), C.POINTER(RowsOut),
                                                 C.POINTER(DecodeOut)]),
        "fhip_decode_frames_windows_spans_held": (i, [vp, vp, i64, vp, vp, C.c_int32, C.POINTER(DecodeSegments),
                                                      C.POINTER(DecodeWindows), C.POINTER(SpanRows), C.POINTER(RowsOut),
                                                      C.POINTER(DecodeOut)]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


ABI_SYMBOLS = (
    "fhip_frame_stride", "fhip_device_count", "fhip_create", "fhip_destroy", "fhip_set_stream", "fhip_sync",
    "fhip_strerror", "fhip_last_error", "fhip_version", "fhip_encode_subframes_dev",
    "fhip_encode_subframes", "fhip_lpc_calc_coefs", "fhip_encode_residual",
    "fhip_prepare_frames", "fhip_calc_rice_params", "fhip_vbs_split", "fhip_set_profiling",
    "fhip_get_kernel_times", "fhip_prepare_ahead", "fhip_encode_frames_packed",
    "fhip_frames_packed_begin", "fhip_frames_packed_fetch", "fhip_encode_blocks_vbs_packed",
    "fhip_encode_blocks_vbs_dev", "fhip_order_search_bits",
    "fhip_host_alloc", "fhip_host_free", "fhip_host_register", "fhip_host_unregister", "fhip_frames_packed_upload", "fhip_frames_packed_fetch_async", "fhip_frames_packed_fetch_wait",
    "fhip_set_verify", "fhip_verify_frames_dev", "fhip_verify_frames", "fhip_last_launches",
    "fhip_verify_frames_numbered_dev", "fhip_verify_frames_numbered", "fhip_last_verify_failure",
    "fhip_set_pcm_format",
    "fhip_md5_init_dev", "fhip_md5_update_dev", "fhip_md5_final_dev", "fhip_md5_final", "fhip_md5_update_uploaded",
    "fhip_device_alloc", "fhip_device_free",
    "fhip_frames_packed_upload_ragged", "fhip_frames_packed_begin_ragged", "fhip_md5_update_uploaded_ragged",
    "fhip_verify_frames_ragged_dev", "fhip_verify_frames_ragged",
    "fhip_encode_blocks_vbs_packed_numbered", "fhip_set_block_numbering", "fhip_verify_frames_blocks_dev",
    "fhip_verify_frames_blocks", "fhip_last_verify_number",
    "fhip_encode_blocks_vbs_ragged_numbered", "fhip_vbs_split_ragged", "fhip_verify_frames_blocks_ragged_dev",
    "fhip_verify_frames_blocks_ragged",
    "fhip_autocorr_tile",
    "fhip_decode_frames_dev", "fhip_decode_frames",
    "fhip_decode_frames_segments_dev", "fhip_decode_frames_segments", "fhip_md5_update_ranges_dev",
    "fhip_index_frames_dev", "fhip_index_frames", "fhip_index_geometry",
    "fhip_gather_spans_dev", "fhip_frames_packed_gather", "fhip_decode_frames_segments_keep",
    "fhip_decode_frames_windows_dev", "fhip_decode_frames_windows",
    "fhip_rows_from_segments_dev", "fhip_rows_zero_dev", "fhip_decode_frames_windows_rows",
)
# ... and what include/flakehip_held.h, which it includes, declares: the held-streams entries (K11)
HELD_ABI_SYMBOLS = (
    "fhip_frame_heads_dev", "fhip_gather_frames_dev", "fhip_decode_frames_windows_held",
    "fhip_decode_frames_windows_rows_held", "fhip_hold_frames",
)
# ... and include/flakehip_rows_in.h: the encode-rows entries (K12)
ROWS_IN_ABI_SYMBOLS = ("fhip_pcm_from_rows_dev", "fhip_frames_packed_from_rows")
# ... and include/flakehip_spans.h: the span-rows entries (K13)
SPANS_ABI_SYMBOLS = ("fhip_span_rows_from_segments_dev", "fhip_decode_frames_windows_spans",
                     "fhip_decode_frames_windows_spans_held")

# fhip_gather_piece (24 bytes): K9's unit, in samples per channel
GATHER_PIECE_DTYPE = np.dtype([("src_buf", "<i4"), ("count", "<i4"), ("src", "<i8"), ("dst", "<i8")])
assert GATHER_PIECE_DTYPE.itemsize == 24


def gather_pieces(rows) -> np.ndarray:
    """[(src_buf, src, dst, count)] as a fhip_gather_piece table."""
    t = np.zeros(len(rows), dtype=GATHER_PIECE_DTYPE)
    for k, (buf, src, dst, count) in enumerate(rows):
        t[k] = (buf, count, src, dst)
    return t


def _ptr(a) -> int | None:
    if a is None:
        return None
    if isinstance(a, int):          # a raw address
        return a
    if isinstance(a, np.ndarray):
        if not a.flags["C_CONTIGUOUS"]:
            raise ValueError("arrays handed to the C ABI must be C-contiguous")
        return a.ctypes.data
    return int(a.data_ptr())        # torch tensor


def _u8(data) -> np.ndarray:
    """bytes, a bytearray or an array as a C-contiguous uint8 array."""
    return np.ascontiguousarray(np.frombuffer(bytes(data), dtype=np.uint8) if isinstance(data, (bytes, bytearray)) else data,
                                dtype=np.uint8)


def rice_slot_bytes(p: Params, n: int) -> int:
    """Slot that any residual section of a frame that will not fall back to
    verbatim fits in: the frame's verbatim size (encode.c:521-527), rounded up."""
    bps = p.bits_per_sample
    if p.channels == 2:
        v = 16 + ((n * (bps + bps + 1) + 7) >> 3)
    else:
        v = 16 + ((n * p.channels * bps + 7) >> 3)
    return (v + 3) & ~3


class Encoder:
    """One ``fhip_ctx``: a device, a stream, workspaces for ``max_frames`` frames."""

    def __init__(self, params: Params, max_frames: int, device: int = 0):
        self.lib = load_library()
        self.params = params.copy()
        self.max_frames = int(max_frames)
        h = C.c_void_p()
        rc = self.lib.fhip_create(C.byref(h), int(device), C.byref(self.params), self.max_frames)
        if rc != OK:
            raise FlakeHipError(rc, "fhip_create", self.lib.fhip_strerror(rc).decode())
        self._h = h
        self.pcm_format = PCM_S32

    # -- plumbing ---------------------------------------------------------
    def close(self) -> None:
        if getattr(self, "_h", None):
            self.lib.fhip_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _check(self, rc: int, what: str) -> None:
        if rc != OK:
            raise FlakeHipError(rc, what, self.lib.fhip_last_error(self._h).decode())

    def set_stream(self, stream_handle: int | None) -> None:
        self._check(self.lib.fhip_set_stream(self._h, stream_handle), "fhip_set_stream")

    def sync(self) -> None:
        self._check(self.lib.fhip_sync(self._h), "fhip_sync")

    def set_profiling(self, on: bool) -> None:
        self._check(self.lib.fhip_set_profiling(self._h, int(on)), "fhip_set_profiling")

    def set_pcm_format(self, fmt: int) -> None:
        """PCM_S32 (default) or PCM_S16: every pcm handed to this handle then addresses interleaved int16
        (fhip_set_pcm_format); the host-array methods below convert to that dtype.  For tests and tools."""
        self._check(self.lib.fhip_set_pcm_format(self._h, int(fmt)), "fhip_set_pcm_format")
        self.pcm_format = int(fmt)

    @property
    def pcm_dtype(self):
        return np.int16 if self.pcm_format == PCM_S16 else np.int32

    def set_verify(self, on: bool) -> None:
        """Verify the handle's own packed output on the device (fhip_set_verify)."""
        self._check(self.lib.fhip_set_verify(self._h, int(on)), "fhip_set_verify")

    def verify_frames_dev(self, stream, stream_bytes: int, frame_bytes, nframes: int, pcm, nsamples: int,
                          first_sample: int, summary, records=None, frame_numbers=None) -> None:
        """K5 on device-resident data (torch tensors or raw device addresses); async.  summary: int64[4]
        (frames checked, failed, first failing frame or -1, its status); records: VERIFY_REC_DTYPE-sized
        int32[nframes][4], optional.  frame_numbers: device uint32[nframes], the number each frame must carry
        (fhip_verify_frames_numbered_dev; first_sample is ignored then)."""
        vi = VerifyIn(_ptr(stream), stream_bytes, _ptr(frame_bytes), nframes, _ptr(pcm), nsamples, first_sample)
        vo = VerifyOut(_ptr(records), _ptr(summary))
        if frame_numbers is not None:
            self._check(self.lib.fhip_verify_frames_numbered_dev(self._h, C.byref(vi), _ptr(frame_numbers),
                                                                 C.byref(vo)), "fhip_verify_frames_numbered_dev")
            return
        self._check(self.lib.fhip_verify_frames_dev(self._h, C.byref(vi), C.byref(vo)), "fhip_verify_frames_dev")

    def _verify_host(self, what: str, args, stream, frame_bytes, pcm, first_sample: int = 0, pcm_dtype=None):
        """One host verify entry: lib.<what>(handle, VerifyIn, *args, VerifyOut) on host arrays, its rc mapped to
        (ok, records as a VERIFY_REC_DTYPE array, summary int64[4], error text)."""
        st = _u8(stream)
        fb = np.ascontiguousarray(frame_bytes, dtype=np.int32)
        pc = np.ascontiguousarray(pcm, dtype=pcm_dtype or self.pcm_dtype).reshape(-1, self.params.channels)
        recs = np.zeros(len(fb), dtype=VERIFY_REC_DTYPE)
        summary = np.zeros(4, dtype=np.int64)
        vi = VerifyIn(st.ctypes.data if st.size else None, st.size, fb.ctypes.data if fb.size else None, len(fb),
                      pc.ctypes.data if pc.size else None, pc.shape[0], first_sample)
        vo = VerifyOut(recs.ctypes.data if len(fb) else None, summary.ctypes.data)
        rc = getattr(self.lib, what)(self._h, C.byref(vi), *args, C.byref(vo))
        if rc not in (OK, E_VERIFY):
            self._check(rc, what)
        return rc == OK, recs, summary, self.lib.fhip_last_error(self._h).decode() if rc else ""

    def verify_frames(self, stream, frame_bytes, pcm, first_sample: int = 0, frame_numbers=None):
        """K5 on host data.  stream: uint8 bytes, frame_bytes: int32[nframes], pcm: [nsamples][channels]
        int32.  frame_numbers: uint32[nframes], the number each frame must carry (fhip_verify_frames_numbered).
        Returns (ok, records as a VERIFY_REC_DTYPE array, summary int64[4], error text)."""
        if frame_numbers is None:
            return self._verify_host("fhip_verify_frames", (), stream, frame_bytes, pcm, first_sample)
        fn = np.ascontiguousarray(frame_numbers, dtype=np.uint32)
        if len(fn) != len(frame_bytes):
            raise ValueError("frame_numbers needs one entry per frame")
        return self._verify_host("fhip_verify_frames_numbered", (fn.ctypes.data if fn.size else None,), stream,
                                 frame_bytes, pcm, first_sample)

    def verify_frames_ragged(self, stream, frame_bytes, pcm, frame_numbers, block_sizes):
        """fhip_verify_frames_ragged on host data: frame f carries frame_numbers[f] and holds block_sizes[f] samples,
        the blocks back to back in pcm.  Returns what verify_frames returns."""
        fn = np.ascontiguousarray(frame_numbers, dtype=np.uint32)
        sz = np.ascontiguousarray(block_sizes, dtype=np.int32)
        if len(fn) != len(frame_bytes) or len(sz) != len(frame_bytes):
            raise ValueError("frame_numbers and block_sizes need one entry per frame")
        return self._verify_host("fhip_verify_frames_ragged", (fn.ctypes.data, sz.ctypes.data), stream, frame_bytes, pcm)

    # -- variable block size for blocks of many streams (the stream set's path at levels 9-12) ------------
    def set_block_numbering(self, on: bool) -> None:
        """fhip_set_block_numbering: frame_numbers of the packed path are first-sample numbers of one-frame blocks
        of independent streams (allow_vbs handles only)."""
        self._check(self.lib.fhip_set_block_numbering(self._h, int(on)), "fhip_set_block_numbering")

    def encode_blocks_vbs_packed_numbered(self, pcm: np.ndarray, block_size: int, block_first):
        """fhip_encode_blocks_vbs_packed_numbered on host data: pcm [nblocks * block_size][channels] int32, block b
        numbered from block_first[b].  Returns (bytes, block_bytes, block_frames, block_max_frame); raises
        FlakeHipError (code E_VERIFY while set_verify is on and a frame fails)."""
        ch = self.params.channels
        pcm = np.ascontiguousarray(pcm, dtype=np.int32).reshape(-1, block_size, ch)
        bf = np.ascontiguousarray(block_first, dtype=np.uint32)
        nb = pcm.shape[0]
        if len(bf) != nb:
            raise ValueError("block_first needs one entry per block")
        cap = 64 + pcm.size * 5 + 64 * (nb + 1) * 8
        out = np.zeros(cap, dtype=np.uint8)
        bb, bfr, bmx = (np.zeros(max(nb, 1), dtype=np.int32) for _ in range(3))
        wrote = C.c_int64(0)
        self._check(self.lib.fhip_encode_blocks_vbs_packed_numbered(
            self._h, pcm.ctypes.data, nb, block_size, bf.ctypes.data, out.ctypes.data, cap, bb.ctypes.data,
            bfr.ctypes.data, bmx.ctypes.data, C.byref(wrote)), "fhip_encode_blocks_vbs_packed_numbered")
        return out[:wrote.value].copy(), bb[:nb], bfr[:nb], bmx[:nb]

    def verify_frames_blocks(self, stream, frame_bytes, pcm, block_first, block_size: int, nblocks: int | None = None):
        """K5's block-table mode on host data (fhip_verify_frames_blocks): pcm holds nblocks blocks of block_size
        samples, block b starts at sample block_first[b] of its stream.  nblocks defaults to len(block_first).
        Returns (ok, records, summary int64[4], error text) as verify_frames does."""
        bf = np.ascontiguousarray(block_first, dtype=np.uint32)
        nb = len(bf) if nblocks is None else int(nblocks)
        if nb > len(bf):
            raise ValueError("block_first is shorter than nblocks")
        return self._verify_host("fhip_verify_frames_blocks", (bf.ctypes.data if bf.size else None, nb, block_size),
                                 stream, frame_bytes, pcm, pcm_dtype=np.int32)

    def encode_blocks_vbs_ragged_numbered(self, pcm: np.ndarray, block_sizes, block_first):
        """fhip_encode_blocks_vbs_ragged_numbered on host data: pcm [sum(block_sizes)][channels] int32, the blocks back
        to back, block b numbered from block_first[b].  Returns (bytes, block_bytes, block_frames, block_max_frame);
        raises FlakeHipError (code E_VERIFY while set_verify is on and a frame fails)."""
        ch = self.params.channels
        pcm = np.ascontiguousarray(pcm, dtype=np.int32).reshape(-1, ch)
        sz = np.ascontiguousarray(block_sizes, dtype=np.int32)
        bf = np.ascontiguousarray(block_first, dtype=np.uint32)
        nb = len(sz)
        if len(bf) != nb or int(sz.sum()) != pcm.shape[0]:
            raise ValueError("block_first needs one entry per block and pcm the blocks' samples")
        cap = 64 + pcm.size * 5 + 64 * (nb + 1) * 8
        out = np.zeros(cap, dtype=np.uint8)
        bb, bfr, bmx = (np.zeros(max(nb, 1), dtype=np.int32) for _ in range(3))
        wrote = C.c_int64(0)
        self._check(self.lib.fhip_encode_blocks_vbs_ragged_numbered(
            self._h, pcm.ctypes.data, nb, sz.ctypes.data, bf.ctypes.data, out.ctypes.data, cap, bb.ctypes.data,
            bfr.ctypes.data, bmx.ctypes.data, C.byref(wrote)), "fhip_encode_blocks_vbs_ragged_numbered")
        return out[:wrote.value].copy(), bb[:nb], bfr[:nb], bmx[:nb]

    def verify_frames_blocks_ragged(self, stream, frame_bytes, pcm, block_first, block_sizes):
        """K5's block-table mode with a length per block, on host data (fhip_verify_frames_blocks_ragged): pcm holds
        the blocks back to back, block b is block_sizes[b] samples and starts at sample block_first[b] of its stream.
        Returns (ok, records, summary int64[4], error text) as verify_frames does."""
        bf = np.ascontiguousarray(block_first, dtype=np.uint32)
        sz = np.ascontiguousarray(block_sizes, dtype=np.int32)
        if len(bf) != len(sz):
            raise ValueError("block_first and block_sizes need one entry per block")
        return self._verify_host("fhip_verify_frames_blocks_ragged",
                                 (bf.ctypes.data if bf.size else None, len(sz), sz.ctypes.data if sz.size else None),
                                 stream, frame_bytes, pcm, pcm_dtype=np.int32)

    def vbs_split_ragged(self, pcm: np.ndarray, block_sizes):
        """fhip_vbs_split_ragged on host data: (frames int32[nblocks], sizes int32[nblocks][8])."""
        pcm = np.ascontiguousarray(pcm, dtype=np.int32).reshape(-1, self.params.channels)
        sz = np.ascontiguousarray(block_sizes, dtype=np.int32)
        if int(sz.sum()) != pcm.shape[0]:
            raise ValueError("pcm must hold the blocks' samples")
        frames = np.zeros(max(len(sz), 1), dtype=np.int32)
        sizes = np.zeros((max(len(sz), 1), 8), dtype=np.int32)
        self._check(self.lib.fhip_vbs_split_ragged(self._h, pcm.ctypes.data, len(sz), sz.ctypes.data, frames.ctypes.data,
                                                   sizes.ctypes.data), "fhip_vbs_split_ragged")
        return frames[:len(sz)], sizes[:len(sz)]

    def verify_frames_blocks_dev(self, stream, stream_bytes: int, frame_bytes, nframes: int, pcm, nsamples: int,
                                 block_first, nblocks: int, block_size: int, summary, records=None) -> None:
        """The same on device-resident data (torch tensors or raw device addresses); async."""
        vi = VerifyIn(_ptr(stream), stream_bytes, _ptr(frame_bytes), nframes, _ptr(pcm), nsamples, 0)
        vo = VerifyOut(_ptr(records), _ptr(summary))
        self._check(self.lib.fhip_verify_frames_blocks_dev(self._h, C.byref(vi), _ptr(block_first), nblocks,
                                                           block_size, C.byref(vo)), "fhip_verify_frames_blocks_dev")

    def last_verify_failure(self):
        """(summary int64[4], record, required number or None) of the handle's most recent host-synchronising
        verification (fhip_last_verify_failure, fhip_last_verify_number); None when no frame failed."""
        summary = np.zeros(4, dtype=np.int64)
        rec = np.zeros(1, dtype=VERIFY_REC_DTYPE)
        if self.lib.fhip_last_verify_failure(self._h, summary.ctypes.data, rec.ctypes.data) != 1:
            return None
        num = C.c_uint32(0)
        have = self.lib.fhip_last_verify_number(self._h, C.byref(num)) == 1
        return summary, rec[0], (num.value if have else None)

    # -- K7: decoding ----------------------------------------------------
    @staticmethod
    def _decode_in(stream, frame_bytes):
        """(DecodeIn of host data for a segment-table entry, frame_bytes as int32[], the stream as uint8[]): the arrays
        outlive the call."""
        st = _u8(stream)
        fb = np.ascontiguousarray(frame_bytes, dtype=np.int32)
        di = DecodeIn(st.ctypes.data if st.size else None, st.size, fb.ctypes.data if fb.size else None, len(fb), 0, -1)
        return di, fb, st

    def _decode_out(self, pcm_cap, out):
        """A host entry's PCM destination: out, or a new array, held to the handle's PCM dtype and to pcm_cap."""
        if out is None:
            out = np.zeros((pcm_cap, self.params.channels), dtype=self.pcm_dtype)
        if out.dtype != self.pcm_dtype or out.size < pcm_cap * self.params.channels:
            raise ValueError("out must hold pcm_cap * channels values of the handle's PCM dtype")
        return out

    def _segments_call(self, call, nframes, out, pcm_cap, seg_first, seg_number, seg_variable, *groups):
        """The body of every host entry over a segment table.  Builds the tables (seg_number defaults to all -1,
        seg_variable to all 0; the three outputs filled with -7, so that what the device did not write shows), the
        records, the summary, DecodeOut (out None: no PCM pointer) and DecodeSegments.  groups: the entry's further
        tables, each group (how the refusal names them, {name: (values, dtype)}): they must hold one value per segment.
        call(sg, do, t) makes the library call with references to the two structures and the groups' tables as arrays by
        name, and returns its code.  Returns (rc, out, nsamples, records, summary, seg_start, seg_samples, seg_failed, error text)."""
        sf = np.ascontiguousarray(seg_first, dtype=np.int32)
        ns = len(sf) - 1
        k = max(ns, 1)
        num = np.full(k, -1, np.int64) if seg_number is None else np.ascontiguousarray(seg_number, dtype=np.int64)
        var = np.zeros(k, np.int32) if seg_variable is None else np.ascontiguousarray(seg_variable, dtype=np.int32)
        t = {}
        for names, group in groups:
            t.update({name: np.ascontiguousarray(values, dtype=dtype) for name, (values, dtype) in group.items()})
            if any(len(t[name]) != ns for name in group):
                raise ValueError(names + " hold one value per segment")
        s_start, s_samples = np.full(k, -7, np.int64), np.full(k, -7, np.int64)
        s_failed = np.full(k, -7, np.int32)
        recs = np.zeros(nframes, dtype=VERIFY_REC_DTYPE)
        summary = np.zeros(4, dtype=np.int64)
        nsm = np.zeros(1, dtype=np.int64)
        do = DecodeOut(_ptr(out) if out is not None and out.size else None, pcm_cap, recs.ctypes.data if nframes else None,
                       summary.ctypes.data, nsm.ctypes.data)
        sg = DecodeSegments(sf.ctypes.data, ns, num.ctypes.data, var.ctypes.data, s_start.ctypes.data,
                            s_samples.ctypes.data, s_failed.ctypes.data)
        rc = call(C.byref(sg), C.byref(do), t)
        return (rc, out, int(nsm[0]), recs, summary, s_start[:ns], s_samples[:ns], s_failed[:ns],
                self.lib.fhip_last_error(self._h).decode() if rc else "")

    def decode_frames(self, stream, frame_bytes, pcm_cap: int, variable_blocks: bool = False, first_number: int = -1,
                      out=None):
        """fhip_decode_frames on host data.  stream: uint8 bytes, frame_bytes: int32[nframes]; pcm_cap: samples per
        channel the output may take.  out (optional): a C-contiguous array of the handle's PCM dtype to decode into
        (at least pcm_cap * channels values), else one is made.  Returns (ok, pcm [pcm_cap][channels], nsamples,
        records as a VERIFY_REC_DTYPE array, summary int64[4], error text); pcm[:nsamples] is the decoded audio
        when ok."""
        st = _u8(stream)
        fb = np.ascontiguousarray(frame_bytes, dtype=np.int32)
        ch = self.params.channels
        if out is None:
            out = np.zeros((pcm_cap, ch), dtype=self.pcm_dtype)
        if out.dtype != self.pcm_dtype or out.size < pcm_cap * ch:
            raise ValueError("out must hold pcm_cap * channels values of the handle's PCM dtype")
        recs = np.zeros(len(fb), dtype=VERIFY_REC_DTYPE)
        summary = np.zeros(4, dtype=np.int64)
        ns = np.zeros(1, dtype=np.int64)
        di = DecodeIn(st.ctypes.data if st.size else None, st.size, fb.ctypes.data if fb.size else None, len(fb),
                      int(bool(variable_blocks)), int(first_number))
        do = DecodeOut(_ptr(out) if out.size else None, pcm_cap, recs.ctypes.data if len(fb) else None,
                       summary.ctypes.data, ns.ctypes.data)
        rc = self.lib.fhip_decode_frames(self._h, C.byref(di), C.byref(do))
        if rc not in (OK, E_VERIFY):
            self._check(rc, "fhip_decode_frames")
        return rc == OK, out, int(ns[0]), recs, summary, self.lib.fhip_last_error(self._h).decode() if rc else ""

    def decode_frames_dev(self, stream, stream_bytes: int, frame_bytes, nframes: int, pcm, pcm_cap: int, summary,
                          nsamples, records=None, variable_blocks: bool = False, first_number: int = -1) -> None:
        """K7 on device-resident data (torch tensors or raw device addresses); async.  pcm: the handle's PCM dtype,
        [pcm_cap][channels]; summary: int64[4]; nsamples: int64[1]; records: int32[nframes][4], optional."""
        di = DecodeIn(_ptr(stream), stream_bytes, _ptr(frame_bytes), nframes, int(bool(variable_blocks)),
                      int(first_number))
        do = DecodeOut(_ptr(pcm), pcm_cap, _ptr(records), _ptr(summary), _ptr(nsamples))
        self._check(self.lib.fhip_decode_frames_dev(self._h, C.byref(di), C.byref(do)), "fhip_decode_frames_dev")

    def decode_frames_segments(self, stream, frame_bytes, pcm_cap: int, seg_first, seg_number=None, seg_variable=None,
                               out=None, md5_states=None, md5_nstreams: int = 0, seg_stream=None, use_segments=True):
        """fhip_decode_frames_segments on host data: the frames of many streams, cut into segments (CSR seg_first
        [nsegs + 1]); seg_number int64[nsegs] (default: all -1, unchecked) and seg_variable int32[nsegs] (default: all
        0).  md5_states (a device address of md5_nstreams fhip_md5_state records) with seg_stream int32[nsegs] also
        hashes each segment into its stream's state on the device.  use_segments=False passes no table (the call is
        then fhip_decode_frames with variable_blocks 0 and first_number -1).  Returns (rc, pcm [pcm_cap][channels],
        nsamples, records, summary, seg_start, seg_samples, seg_failed, error text); rc is OK or E_VERIFY, any other
        code is returned too (E_INVALID: nothing was queued)."""
        di, fb, _st = self._decode_in(stream, frame_bytes)
        out = self._decode_out(pcm_cap, out)
        md = None
        if md5_states is not None:
            ss = np.ascontiguousarray(seg_stream, dtype=np.int32)
            md = DecodeMd5(_ptr(md5_states) if not isinstance(md5_states, int) else md5_states, md5_nstreams,
                           ss.ctypes.data)
        return self._segments_call(
            lambda sg, do, t: self.lib.fhip_decode_frames_segments(self._h, C.byref(di), sg if use_segments else None, do,
                                                                   C.byref(md) if md is not None else None),
            len(fb), out, pcm_cap, seg_first, seg_number, seg_variable)

    def decode_frames_segments_dev(self, stream, stream_bytes: int, frame_bytes, nframes: int, pcm, pcm_cap: int,
                                   summary, nsamples, seg_first, nsegs: int, seg_number, seg_variable, seg_start,
                                   seg_samples, seg_failed, records=None) -> None:
        """K7's segment mode on device-resident data (torch tensors or raw device addresses); async."""
        di = DecodeIn(_ptr(stream), stream_bytes, _ptr(frame_bytes), nframes, 0, -1)
        do = DecodeOut(_ptr(pcm), pcm_cap, _ptr(records), _ptr(summary), _ptr(nsamples))
        sg = DecodeSegments(_ptr(seg_first), nsegs, _ptr(seg_number), _ptr(seg_variable), _ptr(seg_start),
                            _ptr(seg_samples), _ptr(seg_failed))
        self._check(self.lib.fhip_decode_frames_segments_dev(self._h, C.byref(di), C.byref(sg), C.byref(do)),
                    "fhip_decode_frames_segments_dev")

    def decode_frames_windows(self, stream, frame_bytes, pcm_cap: int, seg_first, seg_skip, seg_take, seg_number=None,
                              seg_variable=None, out=None, null_table=None):
        """fhip_decode_frames_windows on host data: decode_frames_segments' arguments plus, per segment, the samples to
        drop from its front (seg_skip int64[nsegs]) and the most to deliver behind them (seg_take int64[nsegs], -1: to
        the segment's end).  The delivered samples lie back to back in pcm; seg_start / seg_samples / nsamples are
        about them.  null_table ("skip" / "take" / "win" / "segs"): pass a null pointer there (the refusals).  Returns
        decode_frames_segments' tuple."""
        di, fb, _st = self._decode_in(stream, frame_bytes)

        def call(sg, do, t):
            wn = DecodeWindows(None if null_table == "skip" else t["seg_skip"].ctypes.data,
                               None if null_table == "take" else t["seg_take"].ctypes.data)
            return self.lib.fhip_decode_frames_windows(self._h, C.byref(di), None if null_table == "segs" else sg,
                                                       None if null_table == "win" else C.byref(wn), do)
        return self._segments_call(call, len(fb), self._decode_out(pcm_cap, out), pcm_cap, seg_first, seg_number,
                                   seg_variable, ("seg_skip and seg_take", {"seg_skip": (seg_skip, np.int64),
                                                                            "seg_take": (seg_take, np.int64)}))

    def decode_frames_windows_dev(self, stream, stream_bytes: int, frame_bytes, nframes: int, pcm, pcm_cap: int,
                                  summary, nsamples, seg_first, nsegs: int, seg_number, seg_variable, seg_start,
                                  seg_samples, seg_failed, seg_skip, seg_take, records=None) -> int:
        """K7's window mode on device-resident data (torch tensors or raw device addresses); async.  Returns the
        entry's code (E_INVALID for a null table: nothing queued)."""
        di = DecodeIn(_ptr(stream), stream_bytes, _ptr(frame_bytes), nframes, 0, -1)
        do = DecodeOut(_ptr(pcm), pcm_cap, _ptr(records), _ptr(summary), _ptr(nsamples))
        sg = DecodeSegments(_ptr(seg_first), nsegs, _ptr(seg_number), _ptr(seg_variable), _ptr(seg_start),
                            _ptr(seg_samples), _ptr(seg_failed))
        wn = DecodeWindows(_ptr(seg_skip), _ptr(seg_take))
        return int(self.lib.fhip_decode_frames_windows_dev(self._h, C.byref(di), C.byref(sg), C.byref(wn), C.byref(do)))

    # -- K10: windows as rows on the device --------------------------------
    def rows_from_segments_dev(self, pcm, pcm_cap: int, nsegs: int, seg_start, seg_samples, seg_failed, seg_row, seg_col,
                               rows, nrows: int, row_len: int, fmt: int) -> int:
        """fhip_rows_from_segments_dev (K10 alone): everything is device memory (torch tensors or raw addresses) -- pcm
        int32 [pcm_cap][channels], seg_start / seg_samples / seg_col int64, seg_failed / seg_row int32, rows
        [nrows][channels][row_len] of the format fmt (ROWS_*).  Async on the handle's stream.  Returns the code:
        E_INVALID means nothing was queued."""
        ro = RowsOut(_ptr(rows), int(nrows), int(fmt), int(row_len))
        return int(self.lib.fhip_rows_from_segments_dev(self._h, _ptr(pcm), int(pcm_cap), int(nsegs), _ptr(seg_start),
                                                        _ptr(seg_samples), _ptr(seg_failed), _ptr(seg_row), _ptr(seg_col),
                                                        C.byref(ro)))

    def rows_zero_dev(self, rows, nrows: int, row_len: int, fmt: int, first_row: int, count: int) -> int:
        """fhip_rows_zero_dev: zero rows first_row .. first_row + count of the destination; async.  Returns the code."""
        ro = RowsOut(_ptr(rows), int(nrows), int(fmt), int(row_len))
        return int(self.lib.fhip_rows_zero_dev(self._h, C.byref(ro), int(first_row), int(count)))

    def decode_frames_windows_rows(self, stream, frame_bytes, pcm_cap: int, seg_first, seg_skip, seg_take, seg_row, seg_col,
                                   rows, nrows: int, row_len: int, fmt: int, seg_number=None, seg_variable=None):
        """fhip_decode_frames_windows_rows: decode_frames_windows' host arguments, host tables seg_row (int32) and
        seg_col (int64) and a device destination rows [nrows][channels][row_len] of the format fmt.  Returns
        decode_frames_windows' tuple with None where the samples were."""
        di, fb, _st = self._decode_in(stream, frame_bytes)
        ro = RowsOut(_ptr(rows), int(nrows), int(fmt), int(row_len))

        def call(sg, do, t):
            wn = DecodeWindows(t["seg_skip"].ctypes.data, t["seg_take"].ctypes.data)
            return self.lib.fhip_decode_frames_windows_rows(self._h, C.byref(di), sg, C.byref(wn), t["seg_row"].ctypes.data,
                                                            t["seg_col"].ctypes.data, C.byref(ro), do)
        return self._segments_call(call, len(fb), None, pcm_cap, seg_first, seg_number, seg_variable,
                                   ("seg_skip, seg_take, seg_row and seg_col",
                                    {"seg_skip": (seg_skip, np.int64), "seg_take": (seg_take, np.int64),
                                     "seg_row": (seg_row, np.int32), "seg_col": (seg_col, np.int64)}))

    # -- K13: spans as hop-spaced rows on the device -------------------------
    def span_rows_from_segments_dev(self, pcm, pcm_cap: int, nsegs: int, seg_start, seg_samples, seg_failed, seg_row0,
                                    seg_nrows, seg_pos, tile_first, ntiles: int, hop: int, rows, nrows: int, row_len: int,
                                    fmt: int) -> int:
        """fhip_span_rows_from_segments_dev (K13 alone): everything is device memory (torch tensors or raw addresses) --
        pcm int32 [pcm_cap][channels], seg_start / seg_samples / seg_pos int64, seg_failed / seg_row0 / seg_nrows int32,
        tile_first int32 [nsegs + 1] (the CSR of the 512-sample tiles each segment gets, ntiles in all), rows
        [nrows][channels][row_len] of the format fmt (ROWS_*).  Async on the handle's stream.  Returns the code:
        E_INVALID means nothing was queued."""
        sp = SpanRows(_ptr(seg_row0), _ptr(seg_nrows), _ptr(seg_pos), int(hop), _ptr(tile_first), int(ntiles))
        ro = RowsOut(_ptr(rows), int(nrows), int(fmt), int(row_len))
        return int(self.lib.fhip_span_rows_from_segments_dev(self._h, _ptr(pcm), int(pcm_cap), int(nsegs), _ptr(seg_start),
                                                             _ptr(seg_samples), _ptr(seg_failed), C.byref(sp), C.byref(ro)))

    # -- K11: held streams -------------------------------------------------
    def frame_heads_dev(self, stream, stream_bytes: int, frame_off, frame_bytes, nframes: int, max_block_size: int,
                        heads) -> int:
        """fhip_frame_heads_dev (k_frame_heads): everything is device memory (torch tensors or raw addresses) --
        frame_off int64, frame_bytes int32, heads nframes records of FRAME_HEAD_DTYPE.  Async.  Returns the code:
        E_INVALID means nothing was queued."""
        return int(self.lib.fhip_frame_heads_dev(self._h, _ptr(stream), int(stream_bytes), _ptr(frame_off),
                                                 _ptr(frame_bytes), int(nframes), int(max_block_size), _ptr(heads)))

    def gather_frames_dev(self, dst, dst_cap: int, dst_frame_bytes, src, src_bytes: int, frame_src, frame_len,
                          nframes: int) -> int:
        """fhip_gather_frames_dev (k_gather_offsets, k_gather_frames): everything is device memory (torch tensors or raw
        addresses) -- frame_src int64, frame_len and dst_frame_bytes int32.  Async.  Returns the code."""
        return int(self.lib.fhip_gather_frames_dev(self._h, _ptr(dst), int(dst_cap), _ptr(dst_frame_bytes), _ptr(src),
                                                   int(src_bytes), _ptr(frame_src), _ptr(frame_len), int(nframes)))

    def _held_call(self, what, sink, sink_tables, src_dev, src_bytes, frame_src, frame_len, pcm_cap, seg_first, seg_skip,
                   seg_take, seg_number, seg_variable, out, null_table):
        """A held entry: lib.<what>(handle, the held source, segs, win, *sink(t), out).  sink_tables: the sink's own group
        of tables (_segments_call), sink(t): its arguments of them."""
        fs = np.ascontiguousarray(frame_src, dtype=np.int64)
        fl = np.ascontiguousarray(frame_len, dtype=np.int32)
        if len(fs) != len(fl):
            raise ValueError("frame_src and frame_len hold one value per frame")

        def call(sg, do, t):
            wn = DecodeWindows(t["seg_skip"].ctypes.data, t["seg_take"].ctypes.data)
            return getattr(self.lib, what)(
                self._h, None if null_table == "src" else _ptr(src_dev), int(src_bytes),
                None if null_table == "frame_src" else (fs.ctypes.data if len(fs) else None),
                None if null_table == "frame_len" else (fl.ctypes.data if len(fl) else None), len(fl),
                None if null_table == "segs" else sg, None if null_table == "win" else C.byref(wn), *sink(t), do)
        return self._segments_call(call, len(fl), out, pcm_cap, seg_first, seg_number, seg_variable,
                                   ("seg_skip and seg_take", {"seg_skip": (seg_skip, np.int64),
                                                              "seg_take": (seg_take, np.int64)}), *sink_tables)

    def decode_frames_windows_held(self, src_dev, src_bytes: int, frame_src, frame_len, pcm_cap: int, seg_first, seg_skip,
                                   seg_take, seg_number=None, seg_variable=None, out=None, null_table=None):
        """fhip_decode_frames_windows_held: decode_frames_windows with the stream taken from device memory -- frame f is
        the frame_len[f] bytes at src_dev + frame_src[f] (src_dev a torch tensor or raw address of src_bytes bytes;
        frame_src int64 and frame_len int32 host tables).  null_table ("src" / "frame_src" / "frame_len" / "segs" /
        "win"): pass a null pointer there (the refusals).  Returns decode_frames_windows' tuple."""
        return self._held_call("fhip_decode_frames_windows_held", lambda t: (), (), src_dev, src_bytes, frame_src, frame_len,
                               pcm_cap, seg_first, seg_skip, seg_take, seg_number, seg_variable, self._decode_out(pcm_cap, out),
                               null_table)

    def decode_frames_windows_rows_held(self, src_dev, src_bytes: int, frame_src, frame_len, pcm_cap: int, seg_first,
                                        seg_skip, seg_take, seg_row, seg_col, rows, nrows: int, row_len: int, fmt: int,
                                        seg_number=None, seg_variable=None, null_table=None):
        """fhip_decode_frames_windows_rows_held: decode_frames_windows_rows with the stream taken from device memory, as
        decode_frames_windows_held takes it.  Returns its tuple with None where the samples were."""
        ro = RowsOut(_ptr(rows), int(nrows), int(fmt), int(row_len))
        return self._held_call("fhip_decode_frames_windows_rows_held",
                               lambda t: (t["seg_row"].ctypes.data, t["seg_col"].ctypes.data, C.byref(ro)),
                               (("seg_row and seg_col", {"seg_row": (seg_row, np.int32), "seg_col": (seg_col, np.int64)}),),
                               src_dev, src_bytes, frame_src, frame_len, pcm_cap, seg_first, seg_skip, seg_take, seg_number,
                               seg_variable, None, null_table)

    def decode_frames_windows_spans_held(self, src_dev, src_bytes: int, frame_src, frame_len, pcm_cap: int, seg_first,
                                         seg_skip, seg_take, seg_row0, seg_nrows, seg_pos, hop: int, rows, nrows: int,
                                         row_len: int, fmt: int, seg_number=None, seg_variable=None, null_table=None):
        """fhip_decode_frames_windows_spans_held: decode_frames_windows_rows_held with K13 behind K7 -- host tables
        seg_row0 / seg_nrows (int32) and seg_pos (int64) and the hop in seg_row's and seg_col's place.  Returns its
        tuple."""
        ro = RowsOut(_ptr(rows), int(nrows), int(fmt), int(row_len))

        def sink(t):
            sp = SpanRows(t["seg_row0"].ctypes.data, t["seg_nrows"].ctypes.data, t["seg_pos"].ctypes.data, int(hop), None, 0)
            return C.byref(sp), C.byref(ro)
        return self._held_call("fhip_decode_frames_windows_spans_held", sink,
                               (("seg_row0, seg_nrows and seg_pos", {"seg_row0": (seg_row0, np.int32),
                                                                     "seg_nrows": (seg_nrows, np.int32),
                                                                     "seg_pos": (seg_pos, np.int64)}),),
                               src_dev, src_bytes, frame_src, frame_len, pcm_cap, seg_first, seg_skip, seg_take, seg_number,
                               seg_variable, None, null_table)

    # -- K8: frame discovery ----------------------------------------------
    def index_ranges(self, stream, range_first, max_block_size: int = 0, frame_cap: int | None = None, sentinel=None):
        """fhip_index_frames on host data: the CPU indexer's answer for the streams stream[range_first[r] :
        range_first[r + 1]] (channels, bits per sample and rate are the handle's).  frame_cap defaults to room for
        every frame there can be.  Returns (rc, frame_bytes int32[frame_cap], range_frames int32[nranges],
        range_consumed int64[nranges], range_variable int32[nranges]); entries of frame_bytes behind the last frame keep
        `sentinel` (default 0).  rc other than OK is returned, not raised (E_INVALID: nothing was queued)."""
        st = _u8(stream)
        rf = np.ascontiguousarray(range_first, dtype=np.int64)
        nr = len(rf) - 1
        if frame_cap is None:
            frame_cap = st.size // 8 + nr + 1           # a frame is no shorter than its header and CRC-16
        fb = np.full(max(frame_cap, 1), 0 if sentinel is None else sentinel, dtype=np.int32)
        k = max(nr, 1)
        r_frames, r_var = np.full(k, -7, np.int32), np.full(k, -7, np.int32)
        r_cons = np.full(k, -7, np.int64)
        ii = IndexIn(st.ctypes.data if st.size else None, st.size, rf.ctypes.data, nr, int(max_block_size), int(frame_cap))
        io = IndexOut(fb.ctypes.data, r_frames.ctypes.data, r_cons.ctypes.data, r_var.ctypes.data)
        rc = self.lib.fhip_index_frames(self._h, C.byref(ii), C.byref(io))
        return rc, fb[:frame_cap], r_frames[:nr], r_cons[:nr], r_var[:nr]

    def index_ranges_dev(self, stream, stream_bytes: int, range_first, nranges: int, max_block_size: int, frame_cap: int,
                         frame_bytes, range_frames, range_consumed, range_variable) -> None:
        """K8 on device-resident data (torch tensors or raw device addresses); async.  range_first, range_consumed:
        int64; the other tables int32."""
        ii = IndexIn(_ptr(stream), stream_bytes, _ptr(range_first), nranges, int(max_block_size), int(frame_cap))
        io = IndexOut(_ptr(frame_bytes), _ptr(range_frames), _ptr(range_consumed), _ptr(range_variable))
        self._check(self.lib.fhip_index_frames_dev(self._h, C.byref(ii), C.byref(io)), "fhip_index_frames_dev")

    # -- K9: gathering spans on the device ---------------------------------
    def gather_spans_dev(self, dst, dst_cap: int, src0, src0_cap: int, src1, src1_cap: int, pieces) -> int:
        """fhip_gather_spans_dev: dst, src0, src1 are int32 device memory (torch tensors or raw addresses; a source may
        be None with capacity 0), capacities in samples per channel; pieces a GATHER_PIECE_DTYPE host table (see
        gather_pieces).  Async on the handle's stream.  Returns the code: E_INVALID means nothing was queued."""
        t = np.ascontiguousarray(pieces, dtype=GATHER_PIECE_DTYPE)
        return self.lib.fhip_gather_spans_dev(self._h, _ptr(dst) if not isinstance(dst, int) else dst, int(dst_cap),
                                              _ptr(src0) if not isinstance(src0, int) else src0, int(src0_cap),
                                              _ptr(src1) if not isinstance(src1, int) else src1, int(src1_cap),
                                              t.ctypes.data if len(t) else None, len(t))

    def frames_packed_gather(self, token: int, nframes: int, block_size: int, src0, src0_cap: int, src1, src1_cap: int,
                             pieces, block_sizes=None) -> int:
        """fhip_frames_packed_gather: the handle's PCM staging filled through a piece table from device sources, in
        place of fhip_frames_packed_upload(_ragged).  token: the value the following _begin's Batch.pcm must carry (it
        names the batch and is never followed).  Returns the code."""
        t = np.ascontiguousarray(pieces, dtype=GATHER_PIECE_DTYPE)
        sz = None if block_sizes is None else np.ascontiguousarray(block_sizes, dtype=np.int32)
        b = Batch(pcm=token, nframes=nframes, block_size=block_size)
        return self.lib.fhip_frames_packed_gather(self._h, C.byref(b), None if sz is None else sz.ctypes.data,
                                                  _ptr(src0) if not isinstance(src0, int) else src0, int(src0_cap),
                                                  _ptr(src1) if not isinstance(src1, int) else src1, int(src1_cap),
                                                  t.ctypes.data if len(t) else None, len(t))

    # -- K12: rows of a planar device batch into interleaved PCM ------------
    def pcm_from_rows_dev(self, dst, dst_cap: int, rows, nrows: int, row_len: int, fmt: int, pieces) -> int:
        """fhip_pcm_from_rows_dev (K12 alone): dst is int32 device memory [dst_cap][channels], rows device memory
        [nrows][channels][row_len] of the format fmt (ROWS_*) (torch tensors or raw addresses); pieces a ROW_PIECE_DTYPE
        host table (see row_pieces).  Async on the handle's stream.  Returns the code: E_INVALID means nothing was
        queued."""
        t = np.ascontiguousarray(pieces, dtype=ROW_PIECE_DTYPE)
        ri = RowsIn(_ptr(rows), int(nrows), int(fmt), int(row_len))
        return int(self.lib.fhip_pcm_from_rows_dev(self._h, _ptr(dst), int(dst_cap), C.byref(ri),
                                                   t.ctypes.data if len(t) else None, len(t)))

    def frames_packed_from_rows(self, token: int, nframes: int, block_size: int, rows, nrows: int, row_len: int, fmt: int,
                                pieces, block_sizes=None) -> int:
        """fhip_frames_packed_from_rows: the handle's PCM staging filled from rows through a piece table, in place of
        fhip_frames_packed_upload(_ragged).  token: the value the following _begin's Batch.pcm must carry (it names the
        batch and is never followed).  Returns the code."""
        t = np.ascontiguousarray(pieces, dtype=ROW_PIECE_DTYPE)
        sz = None if block_sizes is None else np.ascontiguousarray(block_sizes, dtype=np.int32)
        b = Batch(pcm=token, nframes=nframes, block_size=block_size)
        ri = RowsIn(_ptr(rows), int(nrows), int(fmt), int(row_len))
        return int(self.lib.fhip_frames_packed_from_rows(self._h, C.byref(b), None if sz is None else sz.ctypes.data,
                                                         C.byref(ri), t.ctypes.data if len(t) else None, len(t)))

    def kernel_times(self, reset: bool = True) -> dict:
        names = (C.c_char_p * 32)()
        ms = (C.c_double * 32)()
        cnt = (C.c_int * 32)()
        k = self.lib.fhip_get_kernel_times(self._h, names, ms, cnt, 32, int(reset))
        return {names[i].decode(): (ms[i], cnt[i]) for i in range(min(k, 32))}

    def last_launches(self) -> list:
        """The kernel instances the handle's most recent encode call (or prepare_ahead) queued, in
        order: "k_encode_pow2<16,256,0> narrow", ... (fhip_last_launches; host-side, no device work)."""
        k = self.lib.fhip_last_launches(self._h, None, 0)
        if k < 0:
            self._check(k, "fhip_last_launches")
        names = (C.c_char_p * max(k, 1))()
        k = self.lib.fhip_last_launches(self._h, names, k)
        return [names[i].decode() for i in range(k)]

    # -- K6: the MD5 of many streams (device tensors or raw device addresses; async) ------------------
    def md5_init_dev(self, states, nstreams: int) -> None:
        """states: device memory for nstreams fhip_md5_state records (MD5_STATE_BYTES each)."""
        self._check(self.lib.fhip_md5_init_dev(self._h, _ptr(states), nstreams), "fhip_md5_init_dev")

    def md5_update_dev(self, states, nstreams: int, pcm, block_size: int, seg_first, seg_block) -> None:
        """Stream s absorbs blocks seg_block[seg_first[s]:seg_first[s + 1]] of pcm (int32 device tables)."""
        self._check(self.lib.fhip_md5_update_dev(self._h, _ptr(states), nstreams, _ptr(pcm), block_size,
                                                 _ptr(seg_first), _ptr(seg_block)), "fhip_md5_update_dev")

    def md5_update_ranges_dev(self, states, nstreams: int, pcm, seg_first, seg_range, range_start, range_samples) -> None:
        """Stream s absorbs ranges seg_range[seg_first[s]:seg_first[s + 1]] (int32 device tables); range r is
        range_samples[r] samples per channel at sample range_start[r] of pcm (int64 device tables)."""
        self._check(self.lib.fhip_md5_update_ranges_dev(self._h, _ptr(states), nstreams, _ptr(pcm), _ptr(seg_first),
                                                        _ptr(seg_range), _ptr(range_start), _ptr(range_samples)),
                    "fhip_md5_update_ranges_dev")

    def md5_final_dev(self, states, nstreams: int, digests) -> None:
        """digests: device uint8[nstreams][16]; the states stay usable."""
        self._check(self.lib.fhip_md5_final_dev(self._h, _ptr(states), nstreams, _ptr(digests)), "fhip_md5_final_dev")

    # -- hot path ---------------------------------------------------------
    def frame_stride(self, block_size: int) -> int:
        return int(self.lib.fhip_frame_stride(C.byref(self.params), block_size))

    def encode_subframes_dev(self, pcm, nframes: int, block_size: int, info, residual=None,
                             rice_bits=None, slot_bytes: int = 0, samples=None, autoc=None,
                             frames=None, frame_stride: int = 0, frame_bytes=None,
                             first_frame_number: int = 0) -> None:
        """Device-resident batch (torch tensors or raw device addresses); async."""
        b = Batch(_ptr(pcm), nframes, block_size, _ptr(info), _ptr(residual), _ptr(rice_bits),
                  slot_bytes, _ptr(samples), _ptr(autoc), _ptr(frames), frame_stride,
                  _ptr(frame_bytes), first_frame_number, None)
        self._check(self.lib.fhip_encode_subframes_dev(self._h, C.byref(b)),
                    "fhip_encode_subframes_dev")

    def encode_blocks_vbs_dev(self, pcm, nblocks: int, block_size: int, packed, packed_cap: int, totals,
                              frame_bytes=None, block_bytes=None, block_frames=None,
                              first_frame_number: int = 0) -> None:
        """Device-resident variable-block-size batch (vbs.c:85-119 per block); async, no host sync."""
        o = VbsOut(_ptr(packed), packed_cap, _ptr(frame_bytes), _ptr(block_bytes), _ptr(block_frames),
                   _ptr(totals))
        self._check(self.lib.fhip_encode_blocks_vbs_dev(self._h, _ptr(pcm), nblocks, block_size,
                                                        first_frame_number, C.byref(o)),
                    "fhip_encode_blocks_vbs_dev")

    def prepare_ahead(self, pcm, nframes: int, block_size: int) -> None:
        """Hint: start the feeder stage (K0) of the NEXT device-resident batch now, beside the
        batch in flight; the next encode_subframes_dev() call must be for this batch."""
        b = Batch(_ptr(pcm), nframes, block_size, None, None, None, 0, None, None, None, 0,
                  None, 0, None)
        self._check(self.lib.fhip_prepare_ahead(self._h, C.byref(b)), "fhip_prepare_ahead")

    def encode_subframes(self, pcm: np.ndarray, block_size: int, want_residual: bool = True,
                         want_bits: bool = True, want_samples: bool = False,
                         want_autoc: bool = False, want_frames: bool = False,
                         first_frame_number: int = 0) -> dict:
        """Host numpy batch: pcm is [nframes][block_size][channels] int32 (int16 under PCM_S16)."""
        ch = self.params.channels
        pcm = np.ascontiguousarray(pcm, dtype=self.pcm_dtype).reshape(-1, block_size, ch)
        nframes = pcm.shape[0]
        nsub = nframes * ch
        out = {"info": np.zeros(nsub, dtype=INFO_DTYPE)}
        slot = rice_slot_bytes(self.params, block_size)
        if want_residual:
            out["residual"] = np.zeros((nframes, ch, block_size), dtype=np.int32)
        if want_bits:
            out["rice_bits"] = np.zeros((nsub, slot), dtype=np.uint8)
        if want_samples:
            out["samples"] = np.zeros((nframes, ch, block_size), dtype=np.int32)
        if want_autoc:
            out["autoc"] = np.zeros((nsub, MAX_LAGS), dtype=np.float64)
        stride = 0
        if want_frames:
            stride = self.frame_stride(block_size)
            out["frames"] = np.zeros((nframes, stride), dtype=np.uint8)
            out["frame_bytes"] = np.zeros(nframes, dtype=np.int32)
        b = Batch(_ptr(pcm), nframes, block_size, _ptr(out["info"]), _ptr(out.get("residual")),
                  _ptr(out.get("rice_bits")), slot, _ptr(out.get("samples")),
                  _ptr(out.get("autoc")), _ptr(out.get("frames")), stride,
                  _ptr(out.get("frame_bytes")), first_frame_number, None)
        self._check(self.lib.fhip_encode_subframes(self._h, C.byref(b)), "fhip_encode_subframes")
        out["slot_bytes"] = slot
        return out

    # -- stage entry points ----------------------------------------------
    def lpc_calc_coefs(self, samples: np.ndarray, max_order: int, precision: int, omethod: int):
        """lpc_calc_coefs() (lpc.c:224-257) over [nsub][n] blocks."""
        samples = np.ascontiguousarray(samples, dtype=np.int32)
        nsub, n = samples.shape
        coefs = np.zeros((nsub, MAX_ORDER, MAX_ORDER), dtype=np.int32)
        shift = np.zeros((nsub, MAX_ORDER), dtype=np.int32)
        opt = np.zeros(nsub, dtype=np.int32)
        autoc = np.zeros((nsub, MAX_LAGS), dtype=np.float64)
        self._check(self.lib.fhip_lpc_calc_coefs(
            self._h, _ptr(samples), nsub, n, max_order, precision, omethod,
            _ptr(coefs), _ptr(shift), _ptr(opt), _ptr(autoc)), "fhip_lpc_calc_coefs")
        return coefs, shift, opt, autoc

    def encode_residual(self, samples: np.ndarray, obits, want_bits: bool = True) -> dict:
        """encode_residual() (optimize.c:124-276) over prepared [nsub][n] blocks."""
        samples = np.ascontiguousarray(samples, dtype=np.int32)
        nsub, n = samples.shape
        info = np.zeros(nsub, dtype=INFO_DTYPE)
        info["obits"] = obits
        res = np.zeros((nsub, n), dtype=np.int32)
        slot = rice_slot_bytes(self.params, n)
        bits = np.zeros((nsub, slot), dtype=np.uint8) if want_bits else None
        self._check(self.lib.fhip_encode_residual(
            self._h, _ptr(samples), nsub, n, _ptr(info), _ptr(res), _ptr(bits), slot),
            "fhip_encode_residual")
        return {"info": info, "residual": res, "rice_bits": bits, "slot_bytes": slot}

    def order_search_bits(self, samples: np.ndarray, obits, magbits=None) -> np.ndarray:
        """The bits[] table of encode_residual()'s LPC order search (optimize.c:201-261) over prepared
        [nsub][n] blocks: [nsub][32] uint32, 0xFFFFFFFF = order not visited / constant block.
        magbits (|x| < 2^magbits per block, optional) lets 16-bit blocks take the packed FIRs."""
        samples = np.ascontiguousarray(samples, dtype=np.int32)
        nsub, n = samples.shape
        info = np.zeros(nsub, dtype=INFO_DTYPE)
        info["obits"] = obits
        if magbits is not None:
            info["reserved"] = (1 + np.asarray(magbits, dtype=np.int64)) << 8
        bits = np.zeros((nsub, 32), dtype=np.uint32)
        self._check(self.lib.fhip_order_search_bits(self._h, _ptr(samples), nsub, n, _ptr(info), _ptr(bits)),
                    "fhip_order_search_bits")
        return bits

    def calc_rice_params(self, residual: np.ndarray, pred_order: int, lpc: bool, bps: int,
                         pmin: int, pmax: int, slot_bytes: int = 0) -> dict:
        """calc_rice_params_lpc/_fixed (rice.c:173-187) + residual emit on given residuals."""
        residual = np.ascontiguousarray(residual, dtype=np.int32)
        nsub, n = residual.shape
        info = np.zeros(nsub, dtype=INFO_DTYPE)
        bits = np.zeros((nsub, slot_bytes), dtype=np.uint8) if slot_bytes else None
        self._check(self.lib.fhip_calc_rice_params(
            self._h, _ptr(residual), nsub, n, pred_order, int(lpc), bps, pmin, pmax,
            _ptr(info), _ptr(bits), slot_bytes), "fhip_calc_rice_params")
        return {"info": info, "rice_bits": bits}

    def vbs_split(self, pcm: np.ndarray, block_size: int):
        """split_frame_v1 (vbs.c:36-83) over [nblocks][block_size][channels] blocks."""
        ch = self.params.channels
        pcm = np.ascontiguousarray(pcm, dtype=np.int32).reshape(-1, block_size, ch)
        nb = pcm.shape[0]
        frames = np.zeros(nb, dtype=np.int32)
        sizes = np.zeros((nb, 8), dtype=np.int32)
        self._check(self.lib.fhip_vbs_split(self._h, _ptr(pcm), nb, block_size, _ptr(frames),
                                            _ptr(sizes)), "fhip_vbs_split")
        return frames, sizes

    def prepare_frames(self, pcm: np.ndarray, block_size: int):
        """copy_samples + channel_decorrelation + remove_wasted_bits (encode.c:541-694)."""
        ch = self.params.channels
        pcm = np.ascontiguousarray(pcm, dtype=self.pcm_dtype).reshape(-1, block_size, ch)
        nframes = pcm.shape[0]
        smp = np.zeros((nframes, ch, block_size), dtype=np.int32)
        info = np.zeros(nframes * ch, dtype=INFO_DTYPE)
        self._check(self.lib.fhip_prepare_frames(
            self._h, _ptr(pcm), nframes, block_size, _ptr(smp), _ptr(info)),
            "fhip_prepare_frames")
        return smp, info


# ---- host C layer ------------------------------------------------------------

_host = None


def load_host_library() -> C.CDLL:
    global _host
    if _host is not None:
        return _host
    load_library()          # libflake_amd.so links against libflakehip.so
    path = os.path.join(LIB_DIR, "libflake_amd.so")
    if not os.path.exists(path):
        raise ImportError(f"{path} is missing: build it with `python -m flake_amd.build`")
    lib = C.CDLL(path)
    lib.flake_amd_synth_pcm.restype = None
    lib.flake_amd_synth_pcm.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int]
    cp = C.POINTER(HostContext)
    lib.flake_amd_set_defaults.argtypes = [C.POINTER(HostParams)]
    lib.flake_amd_validate_params.argtypes = [cp]
    lib.flake_amd_encode_init.argtypes = [cp]
    lib.flake_amd_get_buffer.argtypes = [cp]
    lib.flake_amd_get_buffer.restype = C.c_void_p
    lib.flake_amd_encode_frame.argtypes = [cp, C.c_void_p, C.c_int]
    lib.flake_amd_encode_frames.argtypes = [cp, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                            C.c_size_t, C.c_void_p]
    lib.flake_amd_encode_frames.restype = C.c_longlong
    lib.flake_amd_encode_frames_s16.argtypes = lib.flake_amd_encode_frames.argtypes
    lib.flake_amd_encode_frames_s16.restype = C.c_longlong
    lib.flake_amd_pin_buffers.argtypes = [cp, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]
    lib.flake_amd_pin_buffers.restype = C.c_int
    lib.flake_amd_encode_close.argtypes = [cp]
    lib.flake_amd_encode_close.restype = None
    lib.flake_amd_get_streaminfo.argtypes = [cp, C.POINTER(HostStreaminfo)]
    lib.flake_amd_write_streaminfo.argtypes = [C.POINTER(HostStreaminfo), C.c_void_p]
    lib.flake_amd_write_streaminfo.restype = None
    lib.flake_amd_get_version.restype = C.c_char_p
    lib.flake_amd_last_error.argtypes = [cp]
    lib.flake_amd_last_error.restype = C.c_char_p
    lib.flake_amd_set_verify.argtypes = [cp, C.c_int]
    lib.flake_amd_set_verify.restype = C.c_int
    lib.flake_amd_set_open.argtypes = [cp, C.c_int, C.c_uint]
    lib.flake_amd_set_open.restype = C.c_void_p
    lib.flake_amd_set_encode.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                         C.c_size_t, C.c_void_p]
    lib.flake_amd_set_encode.restype = C.c_longlong
    lib.flake_amd_set_encode_ragged.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                                C.c_void_p, C.c_size_t, C.c_void_p]
    lib.flake_amd_set_encode_ragged.restype = C.c_longlong
    lib.flake_amd_set_encode_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_longlong, C.c_void_p,
                                              C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    lib.flake_amd_set_encode_rows.restype = C.c_longlong
    lib.flake_amd_set_get_streaminfo.argtypes = [C.c_void_p, C.c_int, C.POINTER(HostStreaminfo)]
    lib.flake_amd_set_get_streaminfo.restype = C.c_int
    lib.flake_amd_set_last_error.argtypes = [C.c_void_p]
    lib.flake_amd_set_last_error.restype = C.c_char_p
    lib.flake_amd_set_enable_verify.argtypes = [C.c_void_p, C.c_int]
    lib.flake_amd_set_enable_verify.restype = C.c_int
    lib.flake_amd_set_last_verify_failure.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_uint),
                                                      C.POINTER(C.c_int)]
    lib.flake_amd_set_last_verify_failure.restype = C.c_int
    lib.flake_amd_set_device_batches.argtypes = [C.c_void_p]
    lib.flake_amd_set_device_batches.restype = C.c_longlong
    lib.flake_amd_set_close.argtypes = [C.c_void_p]
    lib.flake_amd_set_close.restype = None
    lib.flake_amd_read_streaminfo.argtypes = [C.c_void_p, C.POINTER(HostStreaminfo)]
    lib.flake_amd_read_streaminfo.restype = C.c_int
    lib.flake_amd_index_frames.argtypes = [C.POINTER(HostStreaminfo), C.c_void_p, C.c_size_t, C.c_void_p, C.c_int,
                                           C.POINTER(C.c_size_t)]
    lib.flake_amd_index_frames.restype = C.c_longlong
    lib.flake_amd_decode_open.argtypes = [C.POINTER(HostStreaminfo)]
    lib.flake_amd_decode_open.restype = C.c_void_p
    lib.flake_amd_decode_frames.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p,
                                            C.c_int, C.c_size_t]
    lib.flake_amd_decode_frames.restype = C.c_longlong
    lib.flake_amd_decode_index.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.POINTER(C.c_size_t)]
    lib.flake_amd_decode_index.restype = C.c_longlong
    lib.flake_amd_decode_set_index.argtypes = [C.c_void_p, C.c_uint, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                               C.c_void_p, C.c_void_p]
    lib.flake_amd_decode_set_index.restype = C.c_int
    lib.flake_amd_decode_md5.argtypes = [C.c_void_p, C.c_void_p]
    lib.flake_amd_decode_md5.restype = C.c_int
    lib.flake_amd_decode_last_error.argtypes = [C.c_void_p]
    lib.flake_amd_decode_last_error.restype = C.c_char_p
    lib.flake_amd_decode_close.argtypes = [C.c_void_p]
    lib.flake_amd_decode_close.restype = None
    lib.flake_amd_decode_set_open.argtypes = [C.POINTER(HostStreaminfo), C.c_int, C.c_uint]
    lib.flake_amd_decode_set_open.restype = C.c_void_p
    lib.flake_amd_decode_set_frames.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                                C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]
    lib.flake_amd_decode_set_frames.restype = C.c_longlong
    lib.flake_amd_decode_set_windows.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_size_t,
                                                 C.c_void_p, C.c_void_p, C.POINTER(C.c_longlong)]
    lib.flake_amd_decode_set_windows.restype = C.c_longlong
    lib.flake_amd_decode_set_windows_rows.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_longlong,
                                                      C.c_void_p, C.c_void_p, C.POINTER(C.c_longlong)]
    lib.flake_amd_decode_set_windows_rows.restype = C.c_longlong
    lib.flake_amd_decode_set_hold.argtypes = [C.c_void_p, C.c_size_t]
    lib.flake_amd_decode_set_hold.restype = C.c_int
    lib.flake_amd_decode_set_hold_add.argtypes = [C.c_void_p, C.c_uint, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                                  C.c_void_p]
    lib.flake_amd_decode_set_hold_add.restype = C.c_longlong
    lib.flake_amd_decode_set_held_windows.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                      C.c_int, C.c_size_t, C.c_void_p, C.c_void_p,
                                                      C.POINTER(C.c_longlong)]
    lib.flake_amd_decode_set_held_windows.restype = C.c_longlong
    lib.flake_amd_decode_set_held_windows_rows.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                                           C.c_void_p, C.c_int, C.c_longlong, C.c_void_p, C.c_void_p,
                                                           C.POINTER(C.c_longlong)]
    lib.flake_amd_decode_set_held_windows_rows.restype = C.c_longlong
    lib.flake_amd_span_rows_count.argtypes = [C.c_longlong, C.c_longlong, C.c_longlong]
    lib.flake_amd_span_rows_count.restype = C.c_longlong
    lib.flake_amd_decode_set_span_rows.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_int,
                                                   C.c_longlong, C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p,
                                                   C.POINTER(C.c_longlong)]
    lib.flake_amd_decode_set_span_rows.restype = C.c_longlong
    lib.flake_amd_decode_set_held_span_rows.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                                        C.c_longlong, C.c_void_p, C.c_int, C.c_longlong, C.c_longlong,
                                                        C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_longlong)]
    lib.flake_amd_decode_set_held_span_rows.restype = C.c_longlong
    lib.flake_amd_decode_set_held_info.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong),
                                                   C.POINTER(C.c_longlong)]
    lib.flake_amd_decode_set_held_info.restype = C.c_int
    lib.flake_amd_decode_set_held_stats.argtypes = [C.c_void_p, C.c_void_p]
    lib.flake_amd_decode_set_held_stats.restype = C.c_int
    lib.flake_amd_read_seektable.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_int]
    lib.flake_amd_read_seektable.restype = C.c_longlong
    lib.flake_amd_seek_lookup.argtypes = [C.c_void_p, C.c_int, C.c_ulonglong]
    lib.flake_amd_seek_lookup.restype = C.c_longlong
    lib.flake_amd_write_seektable.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t]
    lib.flake_amd_write_seektable.restype = C.c_longlong
    lib.flake_amd_seekpoints_of_frames.argtypes = [C.POINTER(HostStreaminfo), C.c_void_p, C.c_size_t, C.c_void_p, C.c_int,
                                                   C.c_ulonglong, C.c_void_p, C.c_int]
    lib.flake_amd_seekpoints_of_frames.restype = C.c_longlong
    lib.flake_amd_seekpoints.argtypes = [cp, C.c_ulonglong]
    lib.flake_amd_seekpoints.restype = C.c_int
    lib.flake_amd_get_seekpoints.argtypes = [cp, C.c_void_p, C.c_int]
    lib.flake_amd_get_seekpoints.restype = C.c_longlong
    for name in ("flake_amd_set_seekpoints", "flake_amd_recode_set_seekpoints"):
        getattr(lib, name).argtypes = [C.c_void_p, C.c_ulonglong]
        getattr(lib, name).restype = C.c_int
    for name in ("flake_amd_set_get_seekpoints", "flake_amd_recode_set_get_seekpoints"):
        getattr(lib, name).argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
        getattr(lib, name).restype = C.c_longlong
    lib.flake_amd_decode_set_run_offsets.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    lib.flake_amd_decode_set_run_offsets.restype = C.c_int
    lib.flake_amd_decode_set_md5.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    lib.flake_amd_decode_set_md5.restype = C.c_int
    lib.flake_amd_decode_set_failed.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_longlong), C.POINTER(C.c_int)]
    lib.flake_amd_decode_set_failed.restype = C.c_int
    lib.flake_amd_decode_set_device_batches.argtypes = [C.c_void_p]
    lib.flake_amd_decode_set_device_batches.restype = C.c_longlong
    lib.flake_amd_decode_set_last_error.argtypes = [C.c_void_p]
    lib.flake_amd_decode_set_last_error.restype = C.c_char_p
    lib.flake_amd_decode_set_close.argtypes = [C.c_void_p]
    lib.flake_amd_decode_set_close.restype = None
    vp = C.c_void_p
    lib.flake_amd_recode_set_open.argtypes = [C.POINTER(HostStreaminfo), cp, C.c_int, C.c_uint]
    lib.flake_amd_recode_set_open.restype = vp
    lib.flake_amd_recode_set_frames.argtypes = [vp, C.c_int, vp, vp, vp, C.c_size_t, vp, vp, C.c_size_t, vp, vp, C.c_int,
                                                C.POINTER(C.c_int)]
    lib.flake_amd_recode_set_frames.restype = C.c_longlong
    lib.flake_amd_recode_set_out_bound.argtypes = [vp, C.c_longlong, C.POINTER(C.c_size_t), C.POINTER(C.c_longlong)]
    lib.flake_amd_recode_set_out_bound.restype = C.c_int
    lib.flake_amd_recode_set_finish.argtypes = [vp, vp, C.c_size_t, vp, vp, C.c_int, C.POINTER(C.c_int)]
    lib.flake_amd_recode_set_finish.restype = C.c_longlong
    lib.flake_amd_recode_set_get_streaminfo.argtypes = [vp, C.c_int, C.POINTER(HostStreaminfo)]
    lib.flake_amd_recode_set_get_streaminfo.restype = C.c_int
    lib.flake_amd_recode_set_failed.argtypes = [vp, C.c_int, C.POINTER(C.c_longlong), C.POINTER(C.c_int)]
    lib.flake_amd_recode_set_failed.restype = C.c_int
    lib.flake_amd_recode_set_device_batches.argtypes = [vp, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]
    lib.flake_amd_recode_set_device_batches.restype = C.c_int
    lib.flake_amd_recode_set_enable_verify.argtypes = [vp, C.c_int]
    lib.flake_amd_recode_set_enable_verify.restype = C.c_int
    lib.flake_amd_recode_set_last_error.argtypes = [vp]
    lib.flake_amd_recode_set_last_error.restype = C.c_char_p
    lib.flake_amd_recode_set_close.argtypes = [vp]
    lib.flake_amd_recode_set_close.restype = None
    _host = lib
    return lib


class HostParams(C.Structure):
    """``FlakeAmdEncodeParams`` (layout of FlakeEncodeParams, flake.h:59-161)."""
    _fields_ = [(k, C.c_int) for k in (
        "compression", "order_method", "stereo_method", "block_size", "padding_size",
        "min_prediction_order", "max_prediction_order", "prediction_type",
        "min_partition_order", "max_partition_order", "variable_block_size", "allow_vbs")]


class HostContext(C.Structure):
    """``FlakeAmdContext`` (layout of FlakeContext, flake.h:163-215)."""
    _fields_ = [("channels", C.c_int), ("sample_rate", C.c_int), ("bits_per_sample", C.c_int),
                ("samples", C.c_uint), ("params", HostParams), ("header", C.c_void_p),
                ("private_ctx", C.c_void_p)]


class HostStreaminfo(C.Structure):
    _fields_ = [(k, C.c_uint) for k in (
        "min_block_size", "max_block_size", "min_frame_size", "max_frame_size", "sample_rate",
        "channels", "bits_per_sample", "samples")] + [("md5sum", C.c_ubyte * 16)]


class HostEncoder:
    """The host C layer (include/flake_amd.h): libflake's call sequence
    set_defaults -> validate -> encode_init -> encode_frame(s) -> close."""

    def __init__(self, level: int = 5, channels: int = 2, bits_per_sample: int = 16,
                 sample_rate: int = 44100, samples: int = 0, **over):
        self.lib = load_host_library()
        self.ctx = HostContext(channels=channels, sample_rate=sample_rate,
                               bits_per_sample=bits_per_sample, samples=samples)
        self.ctx.params.compression = level
        if self.lib.flake_amd_set_defaults(C.byref(self.ctx.params)) != 0:
            raise ValueError("flake_amd_set_defaults")
        for k, v in over.items():
            if not hasattr(self.ctx.params, k):
                raise AttributeError(k)
            setattr(self.ctx.params, k, v)
        self.subset = self.lib.flake_amd_validate_params(C.byref(self.ctx))
        if self.subset < 0:
            raise ValueError("flake_amd_validate_params rejected the parameters")
        n = self.lib.flake_amd_encode_init(C.byref(self.ctx))
        if n < 0:
            raise FlakeHipError(n, "flake_amd_encode_init")
        self.header = bytes(C.string_at(self.ctx.header, n))
        self.open = True

    def params(self) -> Params:
        hp = self.ctx.params
        return Params(channels=self.ctx.channels, sample_rate=self.ctx.sample_rate,
                      bits_per_sample=self.ctx.bits_per_sample, block_size=hp.block_size,
                      order_method=hp.order_method, stereo_method=hp.stereo_method,
                      prediction_type=hp.prediction_type,
                      min_prediction_order=hp.min_prediction_order,
                      max_prediction_order=hp.max_prediction_order,
                      min_partition_order=hp.min_partition_order,
                      max_partition_order=hp.max_partition_order,
                      variable_block_size=hp.variable_block_size, allow_vbs=hp.allow_vbs,
                      lpc_precision=15)

    def encode_frames(self, pcm: np.ndarray, block_size: int, tail_size: int = 0):
        """pcm: [nblocks*block_size + tail_size][channels] int32.  Returns (bytes, sizes)."""
        return self._encode_frames(pcm, np.int32, block_size, tail_size)

    def encode_frames_s16(self, pcm: np.ndarray, block_size: int, tail_size: int = 0):
        """The same from int16 samples (flake_amd_encode_frames_s16).  For tests and tools."""
        return self._encode_frames(pcm, np.int16, block_size, tail_size)

    def _encode_frames(self, pcm: np.ndarray, dtype, block_size: int, tail_size: int):
        ch = self.ctx.channels
        pcm = np.ascontiguousarray(pcm, dtype=dtype).reshape(-1, ch)
        nblocks = (pcm.shape[0] - tail_size) // block_size
        assert nblocks * block_size + tail_size == pcm.shape[0]
        cap = 64 + pcm.size * 5 + 64 * (nblocks + 1) * 8
        out = np.zeros(cap, dtype=np.uint8)
        sizes = np.zeros(nblocks + (1 if tail_size else 0), dtype=np.int32)
        fn, what = ((self.lib.flake_amd_encode_frames_s16, "flake_amd_encode_frames_s16") if dtype == np.int16
                    else (self.lib.flake_amd_encode_frames, "flake_amd_encode_frames"))
        w = fn(C.byref(self.ctx), pcm.ctypes.data, nblocks, block_size, tail_size, out.ctypes.data, cap,
               sizes.ctypes.data)
        if w < 0:
            raise FlakeHipError(int(w), what, self.lib.flake_amd_last_error(C.byref(self.ctx)).decode())
        return out[:w].copy(), sizes

    def encode_frame(self, pcm: np.ndarray) -> bytes:
        """flake_encode_frame(): one block, result in the library's frame buffer."""
        ch = self.ctx.channels
        pcm = np.ascontiguousarray(pcm, dtype=np.int32).reshape(-1, ch)
        w = self.lib.flake_amd_encode_frame(C.byref(self.ctx), pcm.ctypes.data, pcm.shape[0])
        if w < 0:
            raise FlakeHipError(w, "flake_amd_encode_frame",
                                self.lib.flake_amd_last_error(C.byref(self.ctx)).decode())
        return bytes(C.string_at(self.lib.flake_amd_get_buffer(C.byref(self.ctx)), w))

    def set_verify(self, on: bool) -> None:
        """flake_amd_set_verify: every later encode call verifies its frames on the device."""
        if self.lib.flake_amd_set_verify(C.byref(self.ctx), int(on)) != 0:
            raise RuntimeError("flake_amd_set_verify")

    def seekpoints(self, spacing: int) -> None:
        """flake_amd_seekpoints: record a seek point every `spacing` samples (0: off); before the first block."""
        if self.lib.flake_amd_seekpoints(C.byref(self.ctx), int(spacing)) != 0:
            raise RuntimeError("flake_amd_seekpoints: refused (after the first block?)")

    def get_seekpoints(self):
        """flake_amd_get_seekpoints: the points recorded so far, a SEEK_POINT_DTYPE array."""
        return _seekpoints_from(self.lib.flake_amd_get_seekpoints, "flake_amd_get_seekpoints", C.byref(self.ctx))

    def streaminfo(self) -> HostStreaminfo:
        si = HostStreaminfo()
        if self.lib.flake_amd_get_streaminfo(C.byref(self.ctx), C.byref(si)) != 0:
            raise RuntimeError("flake_amd_get_streaminfo")
        return si

    def close(self) -> None:
        if getattr(self, "open", False):
            self.lib.flake_amd_encode_close(C.byref(self.ctx))
            self.open = False

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def write_streaminfo(si: HostStreaminfo) -> bytes:
    """The 34 STREAMINFO bytes of si (flake_amd_write_streaminfo)."""
    buf = (C.c_ubyte * 34)()
    load_host_library().flake_amd_write_streaminfo(C.byref(si), buf)
    return bytes(buf)


def read_streaminfo(data34: bytes):
    """flake_amd_read_streaminfo: (HostStreaminfo, bits 32..35 of the sample count).  Raises ValueError for a block
    no stream can carry."""
    if len(data34) != 34:
        raise ValueError("a STREAMINFO block is 34 bytes")
    si = HostStreaminfo()
    buf = (C.c_ubyte * 34).from_buffer_copy(bytes(data34))
    hi = load_host_library().flake_amd_read_streaminfo(buf, C.byref(si))
    if hi < 0:
        raise ValueError("invalid STREAMINFO")
    return si, hi


# numpy view of FlakeAmdSeekPoint (24 bytes)
SEEK_POINT_DTYPE = np.dtype([("sample", "<u8"), ("offset", "<u8"), ("frame_samples", "<u4"), ("pad", "<u4")])


def read_seektable(block, cap: int | None = None):
    """flake_amd_read_seektable: the points of a SEEKTABLE block's content that are not placeholders, as a
    SEEK_POINT_DTYPE array -- at most cap of them (default: all) -- and how many the block holds.  Raises ValueError
    for a block that is refused (a length that is no multiple of 18, sample numbers not strictly ascending)."""
    data = np.frombuffer(bytes(block), dtype=np.uint8)
    if cap is None:
        cap = data.size // 18
    pts = np.zeros(max(cap, 1), dtype=SEEK_POINT_DTYPE)
    n = load_host_library().flake_amd_read_seektable(data.ctypes.data if data.size else None, data.size, pts.ctypes.data, cap)
    if n < 0:
        raise ValueError("invalid SEEKTABLE")
    return pts[:min(int(n), cap)].copy(), int(n)


def seek_lookup(points, sample: int) -> int:
    """flake_amd_seek_lookup: the index of the last point at or before `sample`, -1 if there is none."""
    pts = np.ascontiguousarray(points, dtype=SEEK_POINT_DTYPE)
    return int(load_host_library().flake_amd_seek_lookup(pts.ctypes.data if len(pts) else None, len(pts), int(sample)))


def write_seektable(points, placeholders: int = 0) -> bytes:
    """flake_amd_write_seektable: a SEEKTABLE block's content -- the points (a SEEK_POINT_DTYPE array, or rows of
    (sample, offset, frame_samples)) and `placeholders` placeholder points behind them.  Raises ValueError for a table
    that is refused (sample numbers not strictly ascending, too many points)."""
    if not isinstance(points, np.ndarray) or points.dtype != SEEK_POINT_DTYPE:
        rows = [tuple(int(v) for v in p) for p in points]
        points = np.zeros(len(rows), dtype=SEEK_POINT_DTYPE)
        for i, (sample, offset, fs) in enumerate(rows):
            points[i] = (sample, offset, fs, 0)
    pts = np.ascontiguousarray(points)
    buf = np.zeros(max(18 * (len(pts) + max(int(placeholders), 0)), 1), dtype=np.uint8)
    n = load_host_library().flake_amd_write_seektable(pts.ctypes.data if len(pts) else None, len(pts), int(placeholders),
                                                      buf.ctypes.data, buf.size)
    if n < 0:
        raise ValueError("flake_amd_write_seektable refused the table")
    return buf[:n].tobytes()


def _seekpoints_from(fn, what: str, *handle):
    """A getter of recorded seek points (count first, then all of them) as a SEEK_POINT_DTYPE array."""
    n = fn(*handle, None, 0)
    if n < 0:
        raise ValueError(what)
    pts = np.zeros(max(int(n), 1), dtype=SEEK_POINT_DTYPE)
    if fn(*handle, pts.ctypes.data, int(n)) != n:
        raise ValueError(what)
    return pts[:int(n)].copy()


def seekpoints_of_frames(si: HostStreaminfo, stream, sizes, spacing: int):
    """flake_amd_seekpoints_of_frames: the seek points of a finished stream at `spacing` samples, each frame a block
    (sizes from index_frames), as a SEEK_POINT_DTYPE array.  Raises ValueError for a bad argument or a frame whose
    header does not parse."""
    st = _u8(stream)
    fs = np.ascontiguousarray(sizes, dtype=np.int32)
    lib = load_host_library()

    def fn(p, cap):
        return lib.flake_amd_seekpoints_of_frames(C.byref(si), st.ctypes.data if st.size else None, st.size,
                                                  fs.ctypes.data if fs.size else None, len(fs), int(spacing), p, cap)
    return _seekpoints_from(fn, "flake_amd_seekpoints_of_frames")


def span_rows_count(count: int, row_len: int, hop: int) -> int:
    """flake_amd_span_rows_count: the rows of row_len samples, hop apart, that a span of count samples has -- 0 for
    count 0, else min(ceil(count / hop), 1 + ceil(max(count - row_len, 0) / hop)); -1 for a negative count, row_len < 1
    or hop outside 1 .. 2^31 - 1.  Pure: no device, no set."""
    return int(load_host_library().flake_amd_span_rows_count(int(count), int(row_len), int(hop)))


def index_frames(si: HostStreaminfo, stream, cap: int | None = None):
    """flake_amd_index_frames (CPU only): (frame sizes int32[], bytes they cover), or None where the stream does not
    start with a frame."""
    st = _u8(stream)
    if cap is None:
        cap = st.size // 8 + 1            # no frame is shorter than its header and CRC-16
    sizes = np.zeros(max(cap, 1), dtype=np.int32)
    used = C.c_size_t(0)
    n = load_host_library().flake_amd_index_frames(C.byref(si), st.ctypes.data if st.size else None, st.size,
                                                   sizes.ctypes.data, cap, C.byref(used))
    if n < 0:
        return None
    return sizes[:n].copy(), int(used.value)


class HostDecoder:
    """A decoder of the host C layer (flake_amd_decode_*): indexed frames in, PCM out, the MD5 of everything returned
    carried along.  ctypes only; no compute here."""

    def __init__(self, si: HostStreaminfo):
        self.lib = load_host_library()
        self.si = si
        self._d = self.lib.flake_amd_decode_open(C.byref(si))
        if not self._d:
            raise FlakeHipError(-1, "flake_amd_decode_open", self.lib.flake_amd_decode_last_error(None).decode())

    def last_error(self) -> str:
        return self.lib.flake_amd_decode_last_error(self._d).decode()

    def decode_frames(self, stream, frame_sizes, pcm_cap: int, sample_bytes: int = 4) -> np.ndarray:
        """The frames of stream (sizes from index_frames) as [samples][channels] int32, or int16 with sample_bytes 2.
        Raises FlakeHipError naming the frame that failed."""
        st = _u8(stream)
        fs = np.ascontiguousarray(frame_sizes, dtype=np.int32)
        out = np.zeros((pcm_cap, self.si.channels), dtype=np.int16 if sample_bytes == 2 else np.int32)
        n = self.lib.flake_amd_decode_frames(self._d, st.ctypes.data if st.size else None, st.size,
                                             fs.ctypes.data if fs.size else None, len(fs),
                                             out.ctypes.data if out.size else None, sample_bytes, pcm_cap)
        if n < 0:
            raise FlakeHipError(int(n), "flake_amd_decode_frames", self.last_error())
        return out[:n]

    def index(self, stream, cap: int | None = None):
        """flake_amd_decode_index: index_frames' answer, found on the device (K8) -- (frame sizes int32[], bytes they
        cover), or None where the stream does not start with a frame.  Raises FlakeHipError where the device cannot
        answer (2 GiB and more)."""
        st = _u8(stream)
        if cap is None:
            cap = st.size // 8 + 1            # no frame is shorter than its header and CRC-16
        sizes = np.zeros(max(cap, 1), dtype=np.int32)
        used = C.c_size_t(0)
        n = self.lib.flake_amd_decode_index(self._d, st.ctypes.data if st.size else None, st.size, sizes.ctypes.data, cap,
                                            C.byref(used))
        if n < -1:
            raise FlakeHipError(int(n), "flake_amd_decode_index", self.last_error())
        if n < 0:
            return None
        return sizes[:n].copy(), int(used.value)

    def md5(self) -> bytes:
        """flake_amd_decode_md5: of everything decoded so far."""
        buf = (C.c_ubyte * 16)()
        if self.lib.flake_amd_decode_md5(self._d, buf) != 0:
            raise RuntimeError("flake_amd_decode_md5")
        return bytes(buf)

    def close(self) -> None:
        if getattr(self, "_d", None):
            self.lib.flake_amd_decode_close(self._d)
            self._d = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


SET_MD5_HOST, SET_MD5_OFF, SET_VBS = 1, 2, 4      # FLAKE_AMD_SET_*


class StreamSet:
    """A stream set of the host C layer (flake_amd_set_*): many independent streams of one format per batch,
    each stream's MD5 carried on the device.  flags=SET_VBS opens a set with variable block size (levels 9-12: int32
    samples only, a block may become several frames).  ctypes only; no compute here."""

    def __init__(self, nstreams: int, level: int = 5, channels: int = 2, bits_per_sample: int = 16,
                 sample_rate: int = 44100, flags: int = 0, **over):
        self.lib = load_host_library()
        self.ctx = HostContext(channels=channels, sample_rate=sample_rate, bits_per_sample=bits_per_sample)
        self.ctx.params.compression = level
        if self.lib.flake_amd_set_defaults(C.byref(self.ctx.params)) != 0:
            raise ValueError("flake_amd_set_defaults")
        for k, v in over.items():
            if not hasattr(self.ctx.params, k):
                raise AttributeError(k)
            setattr(self.ctx.params, k, v)
        self.nstreams = int(nstreams)
        self.block_size = self.ctx.params.block_size
        self._g = self.lib.flake_amd_set_open(C.byref(self.ctx), self.nstreams, int(flags))
        if not self._g:
            raise FlakeHipError(-1, "flake_amd_set_open", self.lib.flake_amd_set_last_error(None).decode())

    def last_error(self) -> str:
        return self.lib.flake_amd_set_last_error(self._g).decode()

    def encode(self, pcm: np.ndarray, block_size: int, stream_of_block, dtype=np.int32):
        """pcm: [nblocks * block_size][channels] (int32, or int16 with dtype=np.int16), block b of stream
        stream_of_block[b].  Returns (bytes of all frames in batch order, frame sizes [nblocks])."""
        ch = self.ctx.channels
        pcm = np.ascontiguousarray(pcm, dtype=dtype).reshape(-1, ch)
        sob = np.ascontiguousarray(stream_of_block, dtype=np.int32)
        nblocks = len(sob)
        assert nblocks * block_size == pcm.shape[0]
        cap = 64 + pcm.size * 5 + 64 * (nblocks + 1) * 8
        out = np.zeros(cap, dtype=np.uint8)
        sizes = np.zeros(max(nblocks, 1), dtype=np.int32)
        w = self.lib.flake_amd_set_encode(self._g, pcm.ctypes.data, pcm.dtype.itemsize, nblocks, block_size,
                                          sob.ctypes.data, out.ctypes.data, cap, sizes.ctypes.data)
        if w < 0:
            raise FlakeHipError(int(w), "flake_amd_set_encode", self.last_error())
        return out[:w].copy(), sizes[:nblocks]

    def encode_ragged(self, pcm: np.ndarray, block_sizes, stream_of_block, dtype=np.int32):
        """pcm: the blocks back to back, block b block_sizes[b] samples long ([sum(block_sizes)][channels]) and of
        stream stream_of_block[b] (flake_amd_set_encode_ragged).  Returns (bytes of all frames in batch order,
        frame sizes [nblocks])."""
        ch = self.ctx.channels
        pcm = np.ascontiguousarray(pcm, dtype=dtype).reshape(-1, ch)
        sob = np.ascontiguousarray(stream_of_block, dtype=np.int32)
        bsz = np.ascontiguousarray(block_sizes, dtype=np.int32)
        nblocks = len(sob)
        assert len(bsz) == nblocks
        cap = 64 + pcm.size * 5 + 64 * (nblocks + 1) * 8
        out = np.zeros(cap, dtype=np.uint8)
        sizes = np.zeros(max(nblocks, 1), dtype=np.int32)
        w = self.lib.flake_amd_set_encode_ragged(self._g, pcm.ctypes.data, pcm.dtype.itemsize, nblocks, bsz.ctypes.data,
                                                 sob.ctypes.data, out.ctypes.data, cap, sizes.ctypes.data)
        if w < 0:
            raise FlakeHipError(int(w), "flake_amd_set_encode_ragged", self.last_error())
        return out[:w].copy(), sizes[:nblocks]

    def encode_rows(self, rows, lengths, streams=None):
        """flake_amd_set_encode_rows: rows is a contiguous torch tensor [nrows][channels][row_len] of torch.int32,
        torch.int16 or torch.float32 (samples in [-1, 1)) on the set's device; row r is the next lengths[r] samples of
        stream streams[r] (default: row r is of stream r).  Returns a list with each row's bytes: the frames of its whole
        blocks, then of its short block.  Nothing is pending afterwards.  ctypes only; no compute here."""
        import torch
        fmt = {torch.int32: ROWS_I32, torch.int16: ROWS_I16, torch.float32: ROWS_F32}.get(rows.dtype)
        if fmt is None:
            raise ValueError("rows is a tensor of torch.int32, torch.int16 or torch.float32")
        ch = int(self.ctx.channels)
        dev = torch.device("cuda", int(os.environ.get("FLAKE_AMD_DEVICE") or 0))
        if rows.dim() != 3 or rows.shape[1] != ch or not rows.is_contiguous() or rows.device != dev:
            raise ValueError("rows must be a contiguous [nrows, channels, row_len] tensor on the set's device")
        nrows, row_len = int(rows.shape[0]), int(rows.shape[2])
        lens = np.ascontiguousarray(lengths, dtype=np.int64)
        sor = np.ascontiguousarray(np.arange(nrows) if streams is None else streams, dtype=np.int32)
        if len(lens) != nrows or len(sor) != nrows:
            raise ValueError("lengths and streams hold one value per row")
        nblocks = int(sum(-(-int(n) // self.block_size) for n in lens if n > 0))
        cap = 64 + int(np.clip(lens, 0, None).sum()) * ch * 5 + 64 * (nblocks + 1) * 8
        out = np.zeros(cap, dtype=np.uint8)
        whole, tail = np.zeros(max(nrows, 1), dtype=np.int64), np.zeros(max(nrows, 1), dtype=np.int64)
        # the library reads on its handle's stream: whatever torch's own stream still has queued that writes the rows
        # finishes first
        torch.cuda.current_stream(dev).synchronize()
        w = self.lib.flake_amd_set_encode_rows(self._g, rows.data_ptr() if nrows else None, fmt, nrows, row_len,
                                               sor.ctypes.data, lens.ctypes.data, out.ctypes.data, cap,
                                               whole.ctypes.data, tail.ctypes.data)
        if w < 0:
            raise FlakeHipError(int(w), "flake_amd_set_encode_rows", self.last_error())
        wat = np.concatenate([[0], np.cumsum(whole[:nrows])])
        tat = wat[-1] + np.concatenate([[0], np.cumsum(tail[:nrows])])
        return [bytes(out[wat[r]:wat[r + 1]]) + bytes(out[tat[r]:tat[r + 1]]) for r in range(nrows)]

    def device_batches(self) -> int:
        """flake_amd_set_device_batches: chunks handed to an encode entry of the HIP layer since the set was opened."""
        return int(self.lib.flake_amd_set_device_batches(self._g))

    def set_verify(self, on: bool) -> None:
        """flake_amd_set_enable_verify: every later encode call verifies its frames on the device, each against
        its own stream's frame counter."""
        if self.lib.flake_amd_set_enable_verify(self._g, int(on)) != 0:
            raise RuntimeError("flake_amd_set_enable_verify")

    def last_verify_failure(self):
        """(stream, frame number within it, FHIP_VERIFY_* status) of the frame that failed the last encode call's
        verification, or None (flake_amd_set_last_verify_failure)."""
        s, n, st = C.c_int(-1), C.c_uint(0), C.c_int(0)
        if not self.lib.flake_amd_set_last_verify_failure(self._g, C.byref(s), C.byref(n), C.byref(st)):
            return None
        return s.value, n.value, st.value

    def seekpoints(self, spacing: int) -> None:
        """flake_amd_set_seekpoints: record seek points per stream every `spacing` samples (0: off); before the first
        block."""
        if self.lib.flake_amd_set_seekpoints(self._g, int(spacing)) != 0:
            raise RuntimeError("flake_amd_set_seekpoints: refused (after the first block?)")

    def get_seekpoints(self, stream: int):
        """flake_amd_set_get_seekpoints: one stream's points so far, a SEEK_POINT_DTYPE array."""
        return _seekpoints_from(self.lib.flake_amd_set_get_seekpoints, "flake_amd_set_get_seekpoints", self._g, int(stream))

    def streaminfo(self, stream: int) -> HostStreaminfo:
        si = HostStreaminfo()
        if self.lib.flake_amd_set_get_streaminfo(self._g, int(stream), C.byref(si)) != 0:
            raise FlakeHipError(-1, "flake_amd_set_get_streaminfo", self.last_error())
        return si

    def streaminfo_bytes(self, stream: int) -> bytes:
        """The 34 STREAMINFO bytes of one stream (flake_amd_write_streaminfo)."""
        si = self.streaminfo(stream)
        buf = (C.c_ubyte * 34)()
        self.lib.flake_amd_write_streaminfo(C.byref(si), buf)
        return bytes(buf)

    def close(self) -> None:
        if getattr(self, "_g", None):
            self.lib.flake_amd_set_close(self._g)
            self._g = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DecodeSet:
    """A decode set of the host C layer (flake_amd_decode_set_*): runs of frames of many streams of one format per
    call, decoded in shared device batches, each stream's MD5 carried on the device (flags: SET_MD5_HOST, SET_MD5_OFF).
    ctypes only; no compute here."""

    def __init__(self, like: HostStreaminfo, nstreams: int, flags: int = 0):
        self.lib = load_host_library()
        self.si = like
        self.nstreams = int(nstreams)
        self.device = int(os.environ.get("FLAKE_AMD_DEVICE") or 0)      # (what flake_amd_decode_set_open reads)
        self._g = self.lib.flake_amd_decode_set_open(C.byref(like), self.nstreams, int(flags))
        if not self._g:
            raise FlakeHipError(-1, "flake_amd_decode_set_open", self.lib.flake_amd_decode_set_last_error(None).decode())

    def last_error(self) -> str:
        return self.lib.flake_amd_decode_set_last_error(self._g).decode()

    def decode_runs(self, runs, pcm_cap: int, sample_bytes: int = 4):
        """runs: [(stream index, frame bytes, frame sizes)], a run being consecutive frames of one stream.  Returns a
        list with one entry per run: its samples [n][channels] (a view of one buffer), or None for a run of a stream
        that failed (failed(stream) says where).  Raises FlakeHipError when the call is refused: nothing changed then."""
        sor = np.asarray([r[0] for r in runs], dtype=np.int32)
        fs = [np.ascontiguousarray(r[2], dtype=np.int32) for r in runs]
        fof = np.asarray([len(f) for f in fs], dtype=np.int32)
        parts = [_u8(r[1]) for r in runs]
        st = np.ascontiguousarray(np.concatenate(parts)) if parts else np.zeros(0, np.uint8)
        sizes = np.ascontiguousarray(np.concatenate(fs)) if fs else np.zeros(0, np.int32)
        out = np.zeros((pcm_cap, self.si.channels), dtype=np.int16 if sample_bytes == 2 else np.int32)
        rs = np.zeros(max(len(runs), 1), dtype=np.int64)
        n = self.lib.flake_amd_decode_set_frames(self._g, len(runs), sor.ctypes.data if len(runs) else None,
                                                 fof.ctypes.data if len(runs) else None,
                                                 st.ctypes.data if st.size else None, st.size,
                                                 sizes.ctypes.data if sizes.size else None,
                                                 out.ctypes.data if out.size else None, sample_bytes, pcm_cap,
                                                 rs.ctypes.data)
        if n < 0:
            raise FlakeHipError(int(n), "flake_amd_decode_set_frames", self.last_error())
        off = np.zeros(max(len(runs), 1), dtype=np.int64)
        self.lib.flake_amd_decode_set_run_offsets(self._g, off.ctypes.data, len(runs))
        return [None if rs[r] < 0 else out[off[r]:off[r] + rs[r]] if rs[r] else out[:0] for r in range(len(runs))]

    # -- windows: two sources (the call's bytes, the held store) times three sinks (PCM, rows, span rows) ----------------
    @staticmethod
    def _bytes_source(windows):
        """(run bytes, frame sizes, fixed block size, first sample, count) tuples -> (the C arguments nwin, frames_of_win,
        stream, bytes, frame_sizes, fixed_block_size, first_sample, count -- a null pointer for an empty table --, count
        int64[], the arrays the pointers point into: frames_of_win, stream, frame_sizes, fixed, first)."""
        fs = [np.ascontiguousarray(w[1], dtype=np.int32) for w in windows]
        fow = np.asarray([len(f) for f in fs], dtype=np.int32)
        parts = [_u8(w[0]) for w in windows]
        st = np.ascontiguousarray(np.concatenate(parts)) if parts else np.zeros(0, np.uint8)
        sizes = np.ascontiguousarray(np.concatenate(fs)) if fs else np.zeros(0, np.int32)
        fixed = np.asarray([w[2] for w in windows], dtype=np.uint32)
        first = np.asarray([w[3] for w in windows], dtype=np.uint64)
        count = np.asarray([w[4] for w in windows], dtype=np.int64)
        have = len(windows) > 0
        head = (len(windows), fow.ctypes.data if have else None, st.ctypes.data if st.size else None, st.size,
                sizes.ctypes.data if sizes.size else None, fixed.ctypes.data if have else None,
                first.ctypes.data if have else None, count.ctypes.data if have else None)
        return head, count, (fow, st, sizes, fixed, first)

    @staticmethod
    def _held_source(windows):
        """(held id, first sample, count) tuples -> (the C arguments nwin, held_of_win, first_sample, count, count int64[],
        the arrays the pointers point into: ids, first)."""
        ids = np.asarray([w[0] for w in windows], dtype=np.int32)
        first = np.asarray([w[1] for w in windows], dtype=np.uint64)
        count = np.asarray([w[2] for w in windows], dtype=np.int64)
        have = len(windows) > 0
        head = (len(windows), ids.ctypes.data if have else None, first.ctypes.data if have else None,
                count.ctypes.data if have else None)
        return head, count, (ids, first)

    def _windows_call(self, what, head, sink):
        """lib.<what>(set, *head, *sink, win_samples, win_status, frames_decoded) -> (win_samples int64[], win_status
        int32[], the frames handed to the device); raises FlakeHipError when the call is refused."""
        k = max(head[0], 1)
        ws, wst = np.zeros(k, dtype=np.int64), np.zeros(k, dtype=np.int32)
        nfd = C.c_longlong(0)
        n = getattr(self.lib, what)(self._g, *head, *sink, ws.ctypes.data, wst.ctypes.data, C.byref(nfd))
        if n < 0:
            raise FlakeHipError(int(n), what, self.last_error())
        return ws, wst, int(nfd.value)

    def _windows_pcm(self, what, head, count, _arrays, pcm_cap, sample_bytes, out):
        """The PCM sink (head, count, _arrays: a source's answer, the arrays alive until the call is over): pcm_cap
        defaults to the sum of the counts, out to a new array; the call; the result split into one view per window."""
        nwin = head[0]
        if pcm_cap is None:
            pcm_cap = int(np.maximum(count, 0).sum())
        if out is None:
            out = np.zeros((pcm_cap, self.si.channels), dtype=np.int16 if sample_bytes == 2 else np.int32)
        ws, wst, nfd = self._windows_call(what, head, (out.ctypes.data if out.size else None, sample_bytes, pcm_cap))
        res, begins, at = [], [], 0
        for w in range(nwin):
            begins.append(at)
            if ws[w] < 0:
                res.append(None)
                at += int(count[w])
            else:
                res.append(out[at:at + ws[w]])
                at += int(ws[w])
        return res, wst[:nwin], nfd, begins

    def _rows_sink(self, row_len, dtype, out, new_rows, min_rows, first_dim):
        """A rows destination: dtype (default: out's, or float32) to its format; out held to it, to the set's device and
        to [first_dim, channels, row_len] with at least min_rows rows, or made with new_rows() rows.  Returns (out,
        format, row_len) with nothing of torch's own stream pending on out."""
        import torch
        if dtype is None:
            dtype = torch.float32 if out is None else out.dtype
        fmt = {torch.int32: ROWS_I32, torch.int16: ROWS_I16, torch.float32: ROWS_F32}.get(dtype)
        if fmt is None:
            raise ValueError("dtype is torch.int32, torch.int16 or torch.float32")
        ch, row_len = int(self.si.channels), int(row_len)
        dev = torch.device("cuda", self.device)
        if out is None:
            out = torch.empty((new_rows(), ch, max(row_len, 0)), dtype=dtype, device=dev)
        elif (out.dtype != dtype or out.device != dev or not out.is_contiguous() or out.dim() != 3 or out.shape[0] < min_rows
              or tuple(out.shape[1:]) != (ch, row_len)):
            raise ValueError(f"out must be a contiguous [{first_dim}, channels, row_len] tensor of dtype on the set's device")
        # the library writes on its handle's stream: whatever torch's own stream still has queued on this memory (the
        # caching allocator may have handed out a block whose last use is pending there) finishes first
        torch.cuda.current_stream(dev).synchronize()
        return out, fmt, row_len

    def _windows_rows(self, what, head, _count, _arrays, row_len, dtype, out):
        """The rows sink (head, _count, _arrays: a source's answer): window w is row w of out."""
        import torch
        nwin = head[0]
        out, fmt, row_len = self._rows_sink(row_len, dtype, out, lambda: nwin, nwin, ">= nwin")
        ws, wst, nfd = self._windows_call(what, head, (out.data_ptr() if nwin > 0 else None, fmt, row_len))
        return out[:nwin], torch.from_numpy(ws[:nwin].copy()), wst[:nwin], nfd

    def decode_windows(self, windows, pcm_cap: int | None = None, sample_bytes: int = 4, out=None):
        """flake_amd_decode_set_windows.  windows: [(run bytes, frame sizes, fixed block size or 0, first sample,
        count)], a run being consecutive frames of one stream from any frame on.  Returns (one entry per window: its
        samples [n][channels], a view of one buffer, or None for a window that failed; win_status int32[]; the frames
        handed to the device; where each window begins in the buffer).  pcm_cap defaults to the sum of the counts; out
        (optional) is decoded into.  Raises FlakeHipError when the call is refused: nothing was written then."""
        return self._windows_pcm("flake_amd_decode_set_windows", *self._bytes_source(windows), pcm_cap, sample_bytes, out)

    def decode_windows_rows(self, windows, row_len: int, dtype=None, out=None):
        """flake_amd_decode_set_windows_rows: decode_windows' windows as a padded planar batch that stays on the set's
        device.  Returns (tensor [nwin, channels, row_len] of dtype torch.int32, torch.int16 or torch.float32 -- the
        default, samples scaled to [-1, 1) --; lengths, an int64 CPU tensor, -1 for a window that failed; win_status
        int32[]; the frames handed to the device).  Whatever no good window delivered is zero.  out (optional): a
        contiguous tensor on the set's device whose first nwin rows are written; it may hold more rows, which are not
        touched.  Raises FlakeHipError when the call is refused: nothing was written then.  Nothing is pending afterwards.
        ctypes only; no compute here."""
        return self._windows_rows("flake_amd_decode_set_windows_rows", *self._bytes_source(windows), row_len, dtype, out)

    def index(self, streams, max_block_size: int | None = None):
        """flake_amd_decode_set_index: the frames of many files in one device call (K8).  streams: the files' bytes,
        each from its first frame header on; max_block_size: their STREAMINFO value (default: the set's).  Returns one
        entry per stream, each what index_frames returns for it: (frame sizes int32[], bytes they cover) or None."""
        parts = [_u8(x) for x in streams]
        if not parts:
            return []
        st = np.ascontiguousarray(np.concatenate(parts))
        first = np.zeros(len(parts) + 1, dtype=np.uintp)
        first[1:] = np.cumsum([x.size for x in parts])
        cap = st.size // 8 + len(parts) + 1
        sizes = np.zeros(cap, dtype=np.int32)
        frames = np.zeros(len(parts), dtype=np.int64)
        cons = np.zeros(len(parts), dtype=np.uintp)
        rc = self.lib.flake_amd_decode_set_index(self._g, int(self.si.max_block_size if max_block_size is None else max_block_size),
                                                 st.ctypes.data if st.size else None, first.ctypes.data, len(parts),
                                                 sizes.ctypes.data, cap, frames.ctypes.data, cons.ctypes.data)
        if rc != 0:
            raise FlakeHipError(int(rc), "flake_amd_decode_set_index", self.last_error())
        out, at = [], 0
        for r in range(len(parts)):
            if frames[r] < 0:
                out.append(None)
                continue
            out.append((sizes[at:at + frames[r]].copy(), int(cons[r])))
            at += int(frames[r])
        return out

    # -- held streams: a corpus that stays on the device --------------------
    def hold(self, capacity_bytes: int) -> None:
        """flake_amd_decode_set_hold: allocate the set's store on the device, once."""
        if self.lib.flake_amd_decode_set_hold(self._g, int(capacity_bytes)) != 0:
            raise FlakeHipError(-1, "flake_amd_decode_set_hold", self.last_error())

    def hold_add(self, streams, fixed_block_sizes=None, max_block_size: int | None = None):
        """flake_amd_decode_set_hold_add: append files to the store and index them where they lie.  streams: the files'
        bytes, each from its first frame header on; fixed_block_sizes: per file, STREAMINFO's block size where minimum
        and maximum agree, else 0 (default: all 0); max_block_size: their STREAMINFO value (default: the set's).
        Returns the files' ids, in order.  Raises FlakeHipError when the call is refused: nothing changed then."""
        parts = [_u8(x) for x in streams]
        if not parts:
            return []
        st = np.ascontiguousarray(np.concatenate(parts))
        first = np.zeros(len(parts) + 1, dtype=np.uintp)
        first[1:] = np.cumsum([x.size for x in parts])
        fixed = (np.zeros(len(parts), dtype=np.uint32) if fixed_block_sizes is None
                 else np.ascontiguousarray(fixed_block_sizes, dtype=np.uint32))
        if len(fixed) != len(parts):
            raise ValueError("fixed_block_sizes holds one value per stream")
        ids = np.full(len(parts), -1, dtype=np.int32)
        n = self.lib.flake_amd_decode_set_hold_add(self._g, int(self.si.max_block_size if max_block_size is None else max_block_size),
                                                   st.ctypes.data if st.size else None, first.ctypes.data, len(parts),
                                                   fixed.ctypes.data, ids.ctypes.data)
        if n < 0:
            raise FlakeHipError(int(n), "flake_amd_decode_set_hold_add", self.last_error())
        return [int(x) for x in ids]

    def held_windows(self, windows, pcm_cap: int | None = None, sample_bytes: int = 4, out=None):
        """flake_amd_decode_set_held_windows.  windows: [(held id, first sample, count)].  Returns what decode_windows
        returns for the same windows asked of the streams' whole runs."""
        return self._windows_pcm("flake_amd_decode_set_held_windows", *self._held_source(windows), pcm_cap, sample_bytes, out)

    def held_windows_rows(self, windows, row_len: int, dtype=None, out=None):
        """flake_amd_decode_set_held_windows_rows.  windows: [(held id, first sample, count)].  Returns what
        decode_windows_rows returns for the same windows asked of the streams' whole runs; out as there."""
        return self._windows_rows("flake_amd_decode_set_held_windows_rows", *self._held_source(windows), row_len, dtype, out)

    def _span_rows(self, what, head, count, _arrays, row_len, hop, dtype, out):
        """What decode_span_rows and held_span_rows share: the destination, the call (head, count, _arrays: a source's
        answer, the arrays alive until the call is over) and what is returned."""
        import torch
        nspans, hop = len(count), int(hop)

        def new_rows():             # (a call the library will refuse gets no rows: it is the library that says why)
            need = [span_rows_count(int(c), int(row_len), hop) for c in count]
            return max(sum(need) if need and min(need) >= 0 and sum(need) < 2 ** 31 else 0, 1)
        out, fmt, row_len = self._rows_sink(row_len, dtype, out, new_rows, 0, "rows")
        cap = int(out.shape[0])
        first_row = np.zeros(nspans + 1, dtype=np.int32)
        lengths, status = np.zeros(max(cap, 1), dtype=np.int64), np.zeros(max(nspans, 1), dtype=np.int32)
        nfd = C.c_longlong(0)
        n = getattr(self.lib, what)(self._g, *head, hop, out.data_ptr() if nspans > 0 else None, fmt, row_len, cap,
                                    first_row.ctypes.data, lengths.ctypes.data, status.ctypes.data, C.byref(nfd))
        if n < 0:
            raise FlakeHipError(int(n), what, self.last_error())
        return out[:n], torch.from_numpy(lengths[:n].copy()), first_row, status[:nspans], int(nfd.value)

    def decode_span_rows(self, spans, row_len: int, hop: int, dtype=None, out=None):
        """flake_amd_decode_set_span_rows: every window of row_len samples, hop apart, of each span, with every frame
        decoded once.  spans: decode_windows' tuples (bytes, frame sizes, fixed block size, first sample, count), the
        count of any length.  Returns (tensor [R, channels, row_len] on the set's device, dtype as decode_windows_rows';
        lengths, an int64 CPU tensor [R], -1 for the rows of a span that failed; span_first_row int32[nspans + 1];
        span_status int32[nspans]; the frames handed to the device).  Span s owns rows span_first_row[s] ..
        span_first_row[s + 1], span_rows_count(count, row_len, hop) of them; whatever no good span delivered is zero.  out
        (optional): a contiguous [>= R, channels, row_len] tensor on the set's device whose first R rows are written; the
        rest is not touched.  Raises FlakeHipError when the call is refused: nothing was written then.  Nothing is
        pending afterwards.  ctypes only; no compute here."""
        return self._span_rows("flake_amd_decode_set_span_rows", *self._bytes_source(spans), row_len, hop, dtype, out)

    def held_span_rows(self, spans, row_len: int, hop: int, dtype=None, out=None):
        """flake_amd_decode_set_held_span_rows.  spans: [(held id, first sample, count)].  Returns what decode_span_rows
        returns for the same spans asked of the streams' whole runs; out as there."""
        return self._span_rows("flake_amd_decode_set_held_span_rows", *self._held_source(spans), row_len, hop, dtype, out)

    def held_info(self, held_id: int):
        """(frames, samples, bytes) of a held stream."""
        fr, sm, by = C.c_longlong(0), C.c_longlong(0), C.c_longlong(0)
        if self.lib.flake_amd_decode_set_held_info(self._g, int(held_id), C.byref(fr), C.byref(sm), C.byref(by)) != 0:
            raise IndexError(held_id)
        return int(fr.value), int(sm.value), int(by.value)

    def held_stats(self):
        """(bytes resident, frames in the table, bytes uploaded by hold_add, bytes uploaded by held window calls)."""
        out = np.zeros(4, dtype=np.int64)
        if self.lib.flake_amd_decode_set_held_stats(self._g, out.ctypes.data) != 0:
            raise FlakeHipError(-1, "flake_amd_decode_set_held_stats", self.last_error())
        return tuple(int(x) for x in out)

    def md5(self, stream: int):
        """The digest of everything the stream has returned, or None (a failed stream; a set without MD5)."""
        buf = (C.c_ubyte * 16)()
        if self.lib.flake_amd_decode_set_md5(self._g, int(stream), buf) != 0:
            return None
        return bytes(buf)

    def failed(self, stream: int):
        """None while the stream is good, else (frame counted from the stream's first, FHIP_VERIFY_* status)."""
        fr, st = C.c_longlong(-1), C.c_int(0)
        rc = self.lib.flake_amd_decode_set_failed(self._g, int(stream), C.byref(fr), C.byref(st))
        if rc < 0:
            raise IndexError(stream)
        return (fr.value, st.value) if rc else None

    def device_batches(self) -> int:
        return int(self.lib.flake_amd_decode_set_device_batches(self._g))

    def close(self) -> None:
        if getattr(self, "_g", None):
            self.lib.flake_amd_decode_set_close(self._g)
            self._g = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class RecodeSet:
    """A recode set of the host C layer (flake_amd_recode_set_*): FLAC frames of many streams of one format in, FLAC
    frames at other parameters out, the PCM never leaving the device.  like: the sources' STREAMINFO (format and largest
    block); level / over: the encoder's parameters, as StreamSet takes them; flags: SET_VBS (levels 9-12), SET_MD5_OFF.
    ctypes only; no compute here."""

    def __init__(self, like: HostStreaminfo, nstreams: int, level: int = 5, flags: int = 0, channels: int | None = None,
                 bits_per_sample: int | None = None, sample_rate: int | None = None, **over):
        self.lib = load_host_library()
        self.si = like
        self.ctx = HostContext(channels=like.channels if channels is None else channels,
                               sample_rate=like.sample_rate if sample_rate is None else sample_rate,
                               bits_per_sample=like.bits_per_sample if bits_per_sample is None else bits_per_sample)
        self.ctx.params.compression = level
        if self.lib.flake_amd_set_defaults(C.byref(self.ctx.params)) != 0:
            raise ValueError("flake_amd_set_defaults")
        for k, v in over.items():
            if not hasattr(self.ctx.params, k):
                raise AttributeError(k)
            setattr(self.ctx.params, k, v)
        self.nstreams = int(nstreams)
        self.block_size = self.ctx.params.block_size
        self._g = self.lib.flake_amd_recode_set_open(C.byref(like), C.byref(self.ctx), self.nstreams, int(flags))
        if not self._g:
            raise FlakeHipError(-1, "flake_amd_recode_set_open", self.lib.flake_amd_recode_set_last_error(None).decode())

    def last_error(self) -> str:
        return self.lib.flake_amd_recode_set_last_error(self._g).decode()

    def out_bound(self, nframes: int):
        """(bytes, blocks) a recode_runs call of nframes frames may write at most; nframes -1: finish's."""
        nb, nk = C.c_size_t(0), C.c_longlong(0)
        self.lib.flake_amd_recode_set_out_bound(self._g, int(nframes), C.byref(nb), C.byref(nk))
        return nb.value, nk.value

    @staticmethod
    def _split(out, streams, sizes, n):
        res, at = [], 0
        for b in range(n):
            res.append((int(streams[b]), out[at:at + sizes[b]].tobytes()))
            at += int(sizes[b])
        return res

    def recode_runs(self, runs, out_size: int | None = None, block_cap: int | None = None):
        """runs: [(stream index, frame bytes, frame sizes)], as DecodeSet.decode_runs takes them.  Returns the whole
        blocks the call completed as [(stream, bytes)], each stream's in stream order.  out_size / block_cap default
        to the call's bound.  Raises FlakeHipError when the call is refused (nothing changed then) or fails."""
        sor = np.asarray([r[0] for r in runs], dtype=np.int32)
        fs = [np.ascontiguousarray(r[2], dtype=np.int32) for r in runs]
        fof = np.asarray([len(f) for f in fs], dtype=np.int32)
        parts = [_u8(r[1]) for r in runs]
        st = np.ascontiguousarray(np.concatenate(parts)) if parts else np.zeros(0, np.uint8)
        sizes = np.ascontiguousarray(np.concatenate(fs)) if fs else np.zeros(0, np.int32)
        need_bytes, need_blocks = self.out_bound(int(fof.sum()))
        out_size = need_bytes if out_size is None else int(out_size)
        block_cap = need_blocks if block_cap is None else int(block_cap)
        out = np.zeros(max(out_size, 1), dtype=np.uint8)
        bst, bby = np.zeros(max(block_cap, 1), dtype=np.int32), np.zeros(max(block_cap, 1), dtype=np.int32)
        nb = C.c_int(0)
        w = self.lib.flake_amd_recode_set_frames(self._g, len(runs), sor.ctypes.data if len(runs) else None,
                                                 fof.ctypes.data if len(runs) else None,
                                                 st.ctypes.data if st.size else None, st.size,
                                                 sizes.ctypes.data if sizes.size else None, out.ctypes.data, out_size,
                                                 bst.ctypes.data, bby.ctypes.data, block_cap, C.byref(nb))
        if w < 0:
            raise FlakeHipError(int(w), "flake_amd_recode_set_frames", self.last_error())
        assert int(bby[:nb.value].sum()) == w
        return self._split(out, bst, bby, nb.value)

    def finish(self, out_size: int | None = None, block_cap: int | None = None):
        """flake_amd_recode_set_finish: every good stream's tail as [(stream, bytes)]."""
        need_bytes, need_blocks = self.out_bound(-1)
        out_size = need_bytes if out_size is None else int(out_size)
        block_cap = need_blocks if block_cap is None else int(block_cap)
        out = np.zeros(max(out_size, 1), dtype=np.uint8)
        bst, bby = np.zeros(max(block_cap, 1), dtype=np.int32), np.zeros(max(block_cap, 1), dtype=np.int32)
        nb = C.c_int(0)
        w = self.lib.flake_amd_recode_set_finish(self._g, out.ctypes.data, out_size, bst.ctypes.data, bby.ctypes.data,
                                                 block_cap, C.byref(nb))
        if w < 0:
            raise FlakeHipError(int(w), "flake_amd_recode_set_finish", self.last_error())
        return self._split(out, bst, bby, nb.value)

    def streaminfo(self, stream: int):
        """The new STREAMINFO of a good stream (md5sum: the decode side's digest), None for a failed one."""
        si = HostStreaminfo()
        if self.lib.flake_amd_recode_set_get_streaminfo(self._g, int(stream), C.byref(si)) != 0:
            return None
        return si

    def streaminfo_bytes(self, stream: int):
        si = self.streaminfo(stream)
        if si is None:
            return None
        buf = (C.c_ubyte * 34)()
        self.lib.flake_amd_write_streaminfo(C.byref(si), buf)
        return bytes(buf)

    def failed(self, stream: int):
        """None while the stream is good, else (frame counted from the stream's first, FHIP_VERIFY_* status)."""
        fr, st = C.c_longlong(-1), C.c_int(0)
        rc = self.lib.flake_amd_recode_set_failed(self._g, int(stream), C.byref(fr), C.byref(st))
        if rc < 0:
            raise IndexError(stream)
        return (fr.value, st.value) if rc else None

    def device_batches(self):
        """(decode batches, encode batches) so far."""
        d, e = C.c_longlong(0), C.c_longlong(0)
        self.lib.flake_amd_recode_set_device_batches(self._g, C.byref(d), C.byref(e))
        return d.value, e.value

    def set_verify(self, on: bool) -> None:
        if self.lib.flake_amd_recode_set_enable_verify(self._g, int(on)) != 0:
            raise RuntimeError("flake_amd_recode_set_enable_verify")

    def seekpoints(self, spacing: int) -> None:
        """flake_amd_recode_set_seekpoints: record the NEW streams' seek points every `spacing` samples (0: off);
        before the first block."""
        if self.lib.flake_amd_recode_set_seekpoints(self._g, int(spacing)) != 0:
            raise RuntimeError("flake_amd_recode_set_seekpoints: refused (after the first block?)")

    def get_seekpoints(self, stream: int):
        """flake_amd_recode_set_get_seekpoints: a good stream's points so far (a SEEK_POINT_DTYPE array), None for a
        failed one."""
        if self.lib.flake_amd_recode_set_get_seekpoints(self._g, int(stream), None, 0) < 0:
            return None
        return _seekpoints_from(self.lib.flake_amd_recode_set_get_seekpoints, "flake_amd_recode_set_get_seekpoints",
                                self._g, int(stream))

    def close(self) -> None:
        if getattr(self, "_g", None):
            self.lib.flake_amd_recode_set_close(self._g)
            self._g = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def synth_pcm(nframes: int, n: int, channels: int, bps: int, first_frame: int = 0) -> np.ndarray:
    """Deterministic synthetic PCM, [nframes][n][channels] int32."""
    lib = load_host_library()
    out = np.empty((nframes, n, channels), dtype=np.int32)
    lib.flake_amd_synth_pcm(out.ctypes.data, first_frame, nframes, n, channels, bps)
    return out
