"""ctypes binding of libpsk_soft_hip.so (include/psk_soft_hip.h).

The shared library is the product: HIP kernels for gfx950 behind a C ABI.  This module
only marshals arguments.  It never computes anything itself and has no CPU fallback: if
the library is missing, or no MI355X is visible, creation raises.
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libpsk_soft_hip.so")

DEVICE_NONE = -1
OK = 0
NOOP, NORMAL = 0, 1
# Packet.format: interleaved float32 I/Q, interleaved int16 I/Q (sc16), interleaved int8 I/Q (sc8) or interleaved float16 I/Q
# (cf16: torch.complex32 is this layout); n_floats counts the elements of the format
FORMAT_CF32, FORMAT_CS16, FORMAT_CS8, FORMAT_CF16 = 0, 1, 3, 4

STATUS_NAMES = {
    0: "PSK_SOFT_OK",
    1: "PSK_SOFT_ERR_INVALID_ARG",
    2: "PSK_SOFT_ERR_NO_DEVICE",
    3: "PSK_SOFT_ERR_HIP",
    4: "PSK_SOFT_ERR_LIMIT",
    5: "PSK_SOFT_ERR_UNSUPPORTED",
    6: "PSK_SOFT_ERR_CAPACITY",
}

PROP_NAMES = ("samplesPerBaud", "constelationSize", "numAvg", "phaseAvg", "differentialDecoding", "resetState")


class Props(ctypes.Structure):
    _fields_ = [
        ("samplesPerBaud", ctypes.c_uint16),
        ("constelationSize", ctypes.c_uint16),
        ("numAvg", ctypes.c_uint32),
        ("phaseAvg", ctypes.c_uint16),
        ("differentialDecoding", ctypes.c_uint8),
        ("resetState", ctypes.c_uint8),
    ]


class Limits(ctypes.Structure):
    _fields_ = [
        ("max_window_samples", ctypes.c_uint32),
        ("max_phase_avg", ctypes.c_uint32),
        ("max_packet_complex", ctypes.c_uint32),
    ]


class Packet(ctypes.Structure):
    _fields_ = [
        ("data", ctypes.c_void_p),
        ("n_floats", ctypes.c_uint64),
        ("sri_xdelta", ctypes.c_double),
        ("sri_mode", ctypes.c_int32),
        ("sriChanged", ctypes.c_uint8),
        ("inputQueueFlushed", ctypes.c_uint8),
        ("present", ctypes.c_uint8),
        ("format", ctypes.c_uint8),  # FORMAT_CF32 / FORMAT_CS16 / FORMAT_CS8 / FORMAT_CF16
    ]


class Output(ctypes.Structure):
    _fields_ = [
        ("soft", ctypes.c_void_p),
        ("bits", ctypes.c_void_p),
        ("phase", ctypes.c_void_p),
        ("sampleIndex", ctypes.c_void_p),
        ("cap_symbols", ctypes.c_uint64),
        ("ret", ctypes.c_int32),
        ("n_symbols", ctypes.c_uint64),
        ("n_bits", ctypes.c_uint64),
        ("n_sampleIndex", ctypes.c_uint64),
        ("sri_pushed", ctypes.c_int32),
        ("sri_soft_xdelta", ctypes.c_double),
        ("sri_bits_xdelta", ctypes.c_double),
        ("n_warn", ctypes.c_int32),
    ]


class Stats(ctypes.Structure):
    _fields_ = [
        ("channels_fast", ctypes.c_uint64),
        ("channels_exact_timing", ctypes.c_uint64),
        ("channels_sequential", ctypes.c_uint64),
        ("channels_guard", ctypes.c_uint64),
        ("unwrap_extra_passes", ctypes.c_uint64),
        ("unwrap_blocks", ctypes.c_uint64),
        ("timing_exact_blocks", ctypes.c_uint64),
        ("fit_chain_blocks", ctypes.c_uint64),
        ("channels_tiled", ctypes.c_uint64),
        ("channels_parallel_fit", ctypes.c_uint64),
        ("channels_parallel_fit_second_round", ctypes.c_uint64),
        ("parallel_fit_refusals", ctypes.c_uint64),
    ]


# Quality.flags
Q_SOFT, Q_PHASE, Q_INDEX, Q_LOCK, Q_PLANNED = 1, 2, 4, 8, 128


class Quality(ctypes.Structure):
    """psk_soft_quality_t: the record of the last call that covered a channel with OPT_QUALITY on."""

    _fields_ = [
        ("n_symbols", ctypes.c_uint64),
        ("n_finite", ctypes.c_uint64),
        ("n_lock", ctypes.c_uint64),
        ("index_changes", ctypes.c_uint64),
        ("sum_e", ctypes.c_double),
        ("sum_e2", ctypes.c_double),
        ("sum_lock_re", ctypes.c_double),
        ("sum_lock_im", ctypes.c_double),
        ("phase_first", ctypes.c_float),
        ("phase_last", ctypes.c_float),
        ("index_first", ctypes.c_int16),
        ("index_last", ctypes.c_int16),
        ("constelationSize", ctypes.c_uint16),
        ("samplesPerBaud", ctypes.c_uint16),
        ("differentialDecoding", ctypes.c_uint8),
        ("flags", ctypes.c_uint8),
        ("pad", ctypes.c_uint8 * 6),
    ]


class QualityDerived(ctypes.Structure):
    _fields_ = [
        ("lock", ctypes.c_double),
        ("snr_db", ctypes.c_double),
        ("mean_energy", ctypes.c_double),
        ("index_change_rate", ctypes.c_double),
    ]


class Tune(ctypes.Structure):
    """psk_soft_tune_t: phase word of a packet's sample 0 and step per complex sample, both in turns x 2^64."""

    _fields_ = [("phase", ctypes.c_uint64), ("step", ctypes.c_uint64)]


RS_RESTART = 1  # Resample.flags


class Resample(ctypes.Structure):
    """psk_soft_resample_t: position of a packet's first output and step per output, both in input samples x 2^32; step 0
    leaves the packet as it is."""

    _fields_ = [("pos", ctypes.c_uint64), ("step", ctypes.c_uint64), ("flags", ctypes.c_uint32), ("pad", ctypes.c_uint32)]


FIR_RESTART = 1  # Fir.flags
FIR_MAX_TAPS, FIR_SLOTS, FIR_MAX_DECIM = 128, 64, 16
FIR_HISTORY_FLOATS = 2 * (FIR_MAX_TAPS - 1)


class Fir(ctypes.Structure):
    """psk_soft_fir_t: filter = 1 + the slot of the taps (0 leaves the packet as it is), decim input samples per output, pos the
    index of the newest input of the packet's first output (< decim)."""

    _fields_ = [("filter", ctypes.c_uint32), ("decim", ctypes.c_uint32), ("pos", ctypes.c_uint32), ("flags", ctypes.c_uint32)]


# Acquire.flags
A_DATA, A_TUNED, A_PLANNED = 1, 2, 128
ACQUIRE_LAGS = 8  # lags 1, 2, 4 .. 128


class Acquire(ctypes.Structure):
    """psk_soft_acquire_t: the record of the last acquire_device call that covered a channel."""

    _fields_ = [
        ("n_samples", ctypes.c_uint64),
        ("n_valid", ctypes.c_uint64),
        ("n_pairs", ctypes.c_uint64 * ACQUIRE_LAGS),
        ("sum_re", ctypes.c_double * ACQUIRE_LAGS),
        ("sum_im", ctypes.c_double * ACQUIRE_LAGS),
        ("sum_e", ctypes.c_double),
        ("constelationSize", ctypes.c_uint16),
        ("flags", ctypes.c_uint8),
        ("pad", ctypes.c_uint8 * 5),
    ]


class AcquireDerived(ctypes.Structure):
    _fields_ = [
        ("offset_cycles_per_sample", ctypes.c_double),
        ("coherence", ctypes.c_double),
        ("mean_energy", ctypes.c_double),
        ("lags_used", ctypes.c_int32),
        ("pad", ctypes.c_int32),
    ]


# Symrate.flags
SR_DATA, SR_TUNED, SR_PLANNED = 1, 2, 128
SYMRATE_LAGS = 8  # lags of 1, 2, 4 .. 128 blocks


class Symrate(ctypes.Structure):
    """psk_soft_symrate_t: the record of the last symrate_device call that covered a channel (detector 0: e, 1: g)."""

    _fields_ = [
        ("n_samples", ctypes.c_uint64),
        ("n_used", ctypes.c_uint64),
        ("n_blocks", ctypes.c_uint64),
        ("n_valid", ctypes.c_uint64),
        ("n_pairs", ctypes.c_uint64 * SYMRATE_LAGS),
        ("sum_re", (ctypes.c_double * SYMRATE_LAGS) * 2),
        ("sum_im", (ctypes.c_double * SYMRATE_LAGS) * 2),
        ("sum_pow", ctypes.c_double * 2),
        ("sum_lvl", ctypes.c_double * 2),
        ("samplesPerBaud", ctypes.c_uint16),
        ("flags", ctypes.c_uint8),
        ("pad", ctypes.c_uint8 * 5),
    ]


class SymrateDerived(ctypes.Structure):
    _fields_ = [
        ("samples_per_symbol", ctypes.c_double),
        ("step_ratio", ctypes.c_double),
        ("coherence", ctypes.c_double),
        ("mean_level", ctypes.c_double),
        ("detector", ctypes.c_int32),
        ("lags_used", ctypes.c_int32),
    ]


SYNC_RESTART = 1  # SyncIn.flags
SYNC_DATA, SYNC_PLANNED = 1, 128  # SyncRecord.flags
SYNC_MAX_WORD, SYNC_SLOTS, SYNC_HITS = 128, 16, 16
SYNC_HISTORY_FLOATS = 2 * (SYNC_MAX_WORD - 1)


class SyncIn(ctypes.Structure):
    """psk_soft_sync_in_t: one channel of a sync_device call -- a DEVICE pointer to n_symbols (re, im) pairs, word = 1 + the slot
    of the word (0: not searched), flags (SYNC_RESTART), the threshold of a hit."""

    _fields_ = [
        ("soft", ctypes.c_void_p),
        ("n_symbols", ctypes.c_uint64),
        ("word", ctypes.c_uint32),
        ("flags", ctypes.c_uint32),
        ("threshold", ctypes.c_float),
        ("pad", ctypes.c_uint32),
    ]


class SyncHit(ctypes.Structure):
    """psk_soft_sync_hit_t: a window -- its position relative to the row's symbol 0, its sums and its metric."""

    _fields_ = [("pos", ctypes.c_int64), ("cr", ctypes.c_float), ("ci", ctypes.c_float), ("e", ctypes.c_float), ("m", ctypes.c_float)]


class SyncRecord(ctypes.Structure):
    """psk_soft_sync_t: the record of the last sync_device call that covered a channel."""

    _fields_ = [
        ("n_symbols", ctypes.c_uint64),
        ("n_windows", ctypes.c_uint64),
        ("n_valid", ctypes.c_uint64),
        ("n_hits", ctypes.c_uint64),
        ("best", SyncHit),
        ("hits", SyncHit * SYNC_HITS),
        ("word_len", ctypes.c_uint32),
        ("flags", ctypes.c_uint32),
        ("pad", ctypes.c_uint32 * 2),
    ]


class SyncDerived(ctypes.Structure):
    _fields_ = [
        ("angle", ctypes.c_double),
        ("residual", ctypes.c_double),
        ("amplitude", ctypes.c_double),
        ("metric", ctypes.c_double),
        ("rotation", ctypes.c_int32),
        ("pad", ctypes.c_int32),
    ]


DEMAP_I8, DEMAP_FRONT = 1, 2  # DemapIn.flags
DEMAP_DATA, DEMAP_REC_I8, DEMAP_PLANNED = 1, 2, 128  # DemapRecord.flags (REC_I8: the segment's DEMAP_I8 bit shifted left by one)
DEMAP_GAIN_RESIDUAL, DEMAP_GAIN_UNIT = 1, 2  # demap_gain flags
DEMAP_SLOTS, DEMAP_MAX_SEGMENTS, DEMAP_FRONT_SYMBOLS = 16, 1 << 20, 127


class DemapIn(ctypes.Structure):
    """psk_soft_demap_in_t: one segment of a demap_device call -- a DEVICE pointer to the row's symbol 0 and the row's length, the
    segment's first symbol and count, a DEVICE pointer to its output, the channel (with DEMAP_FRONT only), map = 1 + the slot of
    the map (0: skipped), flags (DEMAP_I8, DEMAP_FRONT), the complex gain and the LLR scale."""

    _fields_ = [
        ("soft", ctypes.c_void_p),
        ("n_symbols", ctypes.c_uint64),
        ("pos", ctypes.c_int64),
        ("out", ctypes.c_void_p),
        ("count", ctypes.c_uint32),
        ("channel", ctypes.c_uint32),
        ("map", ctypes.c_uint32),
        ("flags", ctypes.c_uint32),
        ("gain_re", ctypes.c_float),
        ("gain_im", ctypes.c_float),
        ("scale", ctypes.c_float),
        ("pad", ctypes.c_uint32),
    ]


class DemapRecord(ctypes.Structure):
    """psk_soft_demap_t: the record of one segment of the last demap_device call."""

    _fields_ = [
        ("n_symbols", ctypes.c_uint64),
        ("n_finite", ctypes.c_uint64),
        ("n_clip", ctypes.c_uint64),
        ("n_nan", ctypes.c_uint64),
        ("sum_e", ctypes.c_double),
        ("sum_err", ctypes.c_double),
        ("bits", ctypes.c_uint32),
        ("flags", ctypes.c_uint32),
        ("pad", ctypes.c_uint32 * 2),
    ]


VITERBI_PACKED, VITERBI_TERMINATED, VITERBI_ANY_START = 1, 2, 4  # ViterbiIn.flags
# ViterbiRecord.flags: DATA or PLANNED, ORed with the frame's flags shifted left by one
VITERBI_DATA, VITERBI_REC_PACKED, VITERBI_REC_TERMINATED, VITERBI_REC_ANY_START, VITERBI_PLANNED = 1, 2, 4, 8, 128
VITERBI_SLOTS, VITERBI_MAX_FRAMES, VITERBI_MAX_STEPS, VITERBI_SCRATCH_BYTES = 16, 1 << 20, 65536, 256 << 20


class ViterbiIn(ctypes.Structure):
    """psk_soft_viterbi_in_t: one frame of a viterbi_device call -- a DEVICE pointer to its int8 LLRs (any alignment), a DEVICE
    pointer to its output, the trellis steps, code = 1 + the slot of the code (0: skipped) and flags (VITERBI_PACKED,
    VITERBI_TERMINATED, VITERBI_ANY_START)."""

    _fields_ = [
        ("llr", ctypes.c_void_p),
        ("out", ctypes.c_void_p),
        ("n_steps", ctypes.c_uint32),
        ("code", ctypes.c_uint32),
        ("flags", ctypes.c_uint32),
        ("pad", ctypes.c_uint32),
    ]


class ViterbiRecord(ctypes.Structure):
    """psk_soft_viterbi_t: the record of one frame of the last viterbi_device call."""

    _fields_ = [
        ("n_steps", ctypes.c_uint64),
        ("n_llr", ctypes.c_uint64),
        ("metric", ctypes.c_int64),
        ("sum_abs", ctypes.c_int64),
        ("n_flip", ctypes.c_uint32),
        ("n_zero", ctypes.c_uint32),
        ("end_state", ctypes.c_uint32),
        ("start_state", ctypes.c_uint32),
        ("n_bits", ctypes.c_uint32),
        ("flags", ctypes.c_uint32),
        ("pad", ctypes.c_uint32 * 2),
    ]


RS_WITH_PARITY = 1  # RsIn.flags
# RsRecord.flags: DATA or PLANNED, ORed with the frame's flags shifted left by one
RS_DATA, RS_REC_WITH_PARITY, RS_PLANNED = 1, 2, 128
RS_SLOTS, RS_MAX_FRAMES, RS_MAX_DEPTH, RS_MAX_ROOTS, RS_FAILED = 16, 1 << 20, 8, 64, 255
# the usual parameter sets: (gfpoly, fcr, prim, nroots, n)
RS_CCSDS = (0x187, 112, 11, 32, 255)
RS_DVB = (0x11D, 0, 1, 16, 204)


class RsIn(ctypes.Structure):
    """psk_soft_rs_in_t: one frame of an rs_device call -- a DEVICE pointer to its n * depth bytes (any alignment), a DEVICE
    pointer to its output, code = 1 + the slot of the code (0: skipped) and flags (RS_WITH_PARITY)."""

    _fields_ = [
        ("in_", ctypes.c_void_p),
        ("out", ctypes.c_void_p),
        ("code", ctypes.c_uint32),
        ("flags", ctypes.c_uint32),
        ("pad", ctypes.c_uint32 * 2),
    ]


class RsRecord(ctypes.Structure):
    """psk_soft_rs_t: the record of one frame of the last rs_device call.  The C record has no per-frame totals; the properties
    here sum over the frame's codewords."""

    _fields_ = [
        ("flags", ctypes.c_uint32),
        ("n", ctypes.c_uint16),
        ("k", ctypes.c_uint16),
        ("depth", ctypes.c_uint8),
        ("nroots", ctypes.c_uint8),
        ("pad0", ctypes.c_uint8 * 6),
        ("n_err", ctypes.c_uint8 * 8),
        ("n_bit", ctypes.c_uint16 * 8),
        ("pad1", ctypes.c_uint8 * 24),
    ]

    @property
    def failed(self):
        """codewords of the frame that could not be corrected"""
        return sum(1 for j in range(self.depth) if self.n_err[j] == RS_FAILED)

    @property
    def corrected_bytes(self):
        """bytes corrected over the frame's codewords that decoded"""
        return sum(self.n_err[j] for j in range(self.depth) if self.n_err[j] != RS_FAILED)

    @property
    def corrected_bits(self):
        """bits corrected over the frame's codewords that decoded"""
        return sum(self.n_bit[j] for j in range(self.depth))


FRAME_INVERT = 1  # FrameCutIn.flags
# the frame records' flags: DATA or PLANNED; in the cut's ORed with the frame's flags shifted left by one
FRAME_DATA, FRAME_REC_INVERT, FRAME_PLANNED = 1, 2, 128
FRAME_SLOTS, FRAME_MAX_STREAMS, FRAME_MAX_FRAMES, FRAME_MAX_PERIOD, FRAME_MAX_BITS, FRAME_MAX_BYTES = 16, 1 << 20, 1 << 20, 1 << 20, 1 << 31, 1 << 20
FRAME_MAX_DELAY, FRAME_HITS = 1 << 24, 16
# the usual words and formats: (length, word, care) and (branches, cell)
FRAME_CCSDS_ASM = (32, 0x1ACFFC1D, 0xFFFFFFFF)
FRAME_DVB_SYNC = (8, 0x47, 0xFF)
FRAME_DVB_PERIOD = 1632
FRAME_DVB_INTERLEAVER = (12, 17)


class FrameSearchIn(ctypes.Structure):
    """psk_soft_frame_search_in_t: one stream of a frame_search_device call -- a DEVICE pointer to its packed bits (any alignment),
    the bit at which it starts, its length in bits, word = 1 + the slot of the word (0: skipped), max_diff and the period (0: no
    fold)."""

    _fields_ = [
        ("bits", ctypes.c_void_p),
        ("bit0", ctypes.c_uint64),
        ("n_bits", ctypes.c_uint32),
        ("word", ctypes.c_uint32),
        ("max_diff", ctypes.c_uint32),
        ("period", ctypes.c_uint32),
        ("flags", ctypes.c_uint32),
        ("pad", ctypes.c_uint32 * 3),
    ]


class FrameHit(ctypes.Structure):
    """psk_soft_frame_hit_t: a listed hit -- the window's first stream bit, its diff and its polarity (1: inverted)."""

    _fields_ = [("pos", ctypes.c_uint32), ("diff", ctypes.c_uint16), ("pol", ctypes.c_uint8), ("zero", ctypes.c_uint8)]


class FrameSearchRecord(ctypes.Structure):
    """psk_soft_frame_search_t: the record of one stream of the last frame_search_device call."""

    _fields_ = [
        ("flags", ctypes.c_uint32),
        ("length", ctypes.c_uint32),
        ("n_windows", ctypes.c_uint32),
        ("n_hit", ctypes.c_uint32 * 2),
        ("min_diff", ctypes.c_uint32),
        ("min_pos", ctypes.c_uint32),
        ("min_pol", ctypes.c_uint32),
        ("best_phase", ctypes.c_uint32),
        ("best_score", ctypes.c_uint32),
        ("best_inv", ctypes.c_uint32),
        ("n_listed", ctypes.c_uint32),
        ("pad", ctypes.c_uint32 * 4),
        ("hits", FrameHit * 16),
    ]

    @property
    def listed(self):
        """the listed hits as (pos, diff, pol) tuples"""
        return [(int(k.pos), int(k.diff), int(k.pol)) for k in self.hits[: self.n_listed]]


class FrameCutIn(ctypes.Structure):
    """psk_soft_frame_cut_in_t: one frame of a frame_cut_device call -- a DEVICE pointer to the stream's packed bits, the bit at
    which the frame starts, a DEVICE pointer to its n_bytes output bytes, format = 1 + the slot of the format (0: plain), the
    branch of its first byte and flags (FRAME_INVERT)."""

    _fields_ = [
        ("bits", ctypes.c_void_p),
        ("bit", ctypes.c_uint64),
        ("out", ctypes.c_void_p),
        ("n_bytes", ctypes.c_uint32),
        ("format", ctypes.c_uint32),
        ("branch0", ctypes.c_uint32),
        ("flags", ctypes.c_uint32),
        ("pad", ctypes.c_uint32 * 2),
    ]


class FrameCutRecord(ctypes.Structure):
    """psk_soft_frame_cut_t: the record of one frame of the last frame_cut_device call."""

    _fields_ = [
        ("flags", ctypes.c_uint32),
        ("n_bytes", ctypes.c_uint32),
        ("span", ctypes.c_uint32),
        ("n_ones", ctypes.c_uint32),
        ("pad", ctypes.c_uint32 * 4),
    ]


QUALITY_FIELDS = tuple(k for k, _ in Quality._fields_ if k != "pad")

# every symbol include/psk_soft_rs.h declares (the psk_soft_rs_ family; psk_soft_hip.h includes that header)
RS_EXPORTS = (
    "psk_soft_rs_define",
    "psk_soft_rs_device",
    "psk_soft_get_rs",
    "psk_soft_rs_host",
    "psk_soft_rs_encode_host",
    "psk_soft_rs_bytes",
    "psk_soft_rs_in_bytes",
)

# every symbol include/psk_soft_frame.h declares (the psk_soft_frame_ family; psk_soft_hip.h includes that header)
FRAME_EXPORTS = (
    "psk_soft_frame_word_define",
    "psk_soft_frame_search_device",
    "psk_soft_get_frame_search",
    "psk_soft_frame_search_host",
    "psk_soft_frame_tile",
    "psk_soft_frame_format_define",
    "psk_soft_frame_cut_device",
    "psk_soft_get_frame_cut",
    "psk_soft_frame_cut_host",
    "psk_soft_frame_span",
    "psk_soft_frame_search_bytes",
    "psk_soft_frame_search_in_bytes",
    "psk_soft_frame_cut_bytes",
    "psk_soft_frame_cut_in_bytes",
)

# every symbol include/psk_soft_hip.h declares
EXPORTS = (
    "psk_soft_quality_bytes",
    "psk_soft_get_quality",
    "psk_soft_quality_derive",
    "psk_soft_device_alloc",
    "psk_soft_device_free",
    "psk_soft_device_upload",
    "psk_soft_device_download",
    "psk_soft_get_channel_stats",
    "psk_soft_probe_read_ms",
    "psk_soft_set_option",
    "psk_soft_host_alloc",
    "psk_soft_host_free",
    "psk_soft_abi_version",
    "psk_soft_last_error",
    "psk_soft_create",
    "psk_soft_destroy",
    "psk_soft_configure",
    "psk_soft_query",
    "psk_soft_fire_listener",
    "psk_soft_output_capacity",
    "psk_soft_process_device",
    "psk_soft_process_device_strided",
    "psk_soft_process_device_tuned",
    "psk_soft_tune_step",
    "psk_soft_tune_advance",
    "psk_soft_tune_apply",
    "psk_soft_process_device_resampled",
    "psk_soft_resample_get_history",
    "psk_soft_resample_set_history",
    "psk_soft_resample_step",
    "psk_soft_resample_count",
    "psk_soft_resample_advance",
    "psk_soft_resample_apply",
    "psk_soft_resample_piece",
    "psk_soft_fir_define",
    "psk_soft_process_device_filtered",
    "psk_soft_fir_get_history",
    "psk_soft_fir_set_history",
    "psk_soft_fir_count",
    "psk_soft_fir_advance",
    "psk_soft_fir_apply",
    "psk_soft_fir_piece",
    "psk_soft_acquire_device",
    "psk_soft_get_acquire",
    "psk_soft_acquire_derive",
    "psk_soft_acquire_host",
    "psk_soft_acquire_bytes",
    "psk_soft_acquire_piece",
    "psk_soft_symrate_device",
    "psk_soft_get_symrate",
    "psk_soft_symrate_derive",
    "psk_soft_symrate_host",
    "psk_soft_symrate_bytes",
    "psk_soft_symrate_piece",
    "psk_soft_sync_define",
    "psk_soft_sync_device",
    "psk_soft_get_sync",
    "psk_soft_sync_get_history",
    "psk_soft_sync_set_history",
    "psk_soft_sync_derive",
    "psk_soft_sync_host",
    "psk_soft_sync_bytes",
    "psk_soft_sync_in_bytes",
    "psk_soft_sync_piece",
    "psk_soft_demap_define",
    "psk_soft_demap_device",
    "psk_soft_get_demap",
    "psk_soft_demap_host",
    "psk_soft_demap_gain",
    "psk_soft_demap_bytes",
    "psk_soft_demap_in_bytes",
    "psk_soft_demap_piece",
    "psk_soft_viterbi_define",
    "psk_soft_viterbi_device",
    "psk_soft_get_viterbi",
    "psk_soft_viterbi_host",
    "psk_soft_viterbi_encode_host",
    "psk_soft_viterbi_count",
    "psk_soft_viterbi_bytes",
    "psk_soft_viterbi_in_bytes",
    "psk_soft_process_host",
    "psk_soft_synchronize",
    "psk_soft_join",
    "psk_soft_get_stats",
    "psk_soft_set_force_sequential",
    "psk_soft_state_bytes",
    "psk_soft_export_state",
    "psk_soft_import_state",
    "psk_soft_peek",
)


class PskSoftError(RuntimeError):
    def __init__(self, status, text):
        super().__init__("%s: %s" % (STATUS_NAMES.get(status, status), text))
        self.status = status


_lib = None


def load():
    """Load the shared library; raises if it has not been built (no fallback).

    The library links the system's HIP runtime, and torch carries one of its own.  A process that uses both (the test suite
    does) imports torch in front of the first load(): the library then binds to the runtime torch has brought.  The other way
    round the process maps two runtimes, and torch finds no device."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "libpsk_soft_hip.so is not built (run `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C psk_soft_amd/csrc`); there is no CPU fallback"
        )
    L = ctypes.CDLL(LIB_PATH)
    vp, u32, u64, i32 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int
    L.psk_soft_abi_version.restype = u32
    L.psk_soft_last_error.restype = ctypes.c_char_p
    L.psk_soft_create.argtypes = [i32, u32, ctypes.POINTER(Limits), ctypes.POINTER(vp)]
    L.psk_soft_destroy.argtypes = [vp]
    L.psk_soft_configure.argtypes = [vp, u32, u32, ctypes.POINTER(Props)]
    L.psk_soft_query.argtypes = [vp, u32, ctypes.POINTER(Props)]
    L.psk_soft_fire_listener.argtypes = [vp, u32, i32]
    L.psk_soft_output_capacity.argtypes = [vp, u32, u64]
    L.psk_soft_output_capacity.restype = u64
    L.psk_soft_process_device.argtypes = [vp, u32, u32, ctypes.POINTER(Packet), ctypes.POINTER(Output), vp]
    L.psk_soft_process_device_strided.argtypes = [vp, u32, u32, ctypes.POINTER(Packet), ctypes.POINTER(u64), ctypes.POINTER(Output), vp]
    L.psk_soft_process_device_tuned.argtypes = [
        vp, u32, u32, ctypes.POINTER(Packet), ctypes.POINTER(u64), ctypes.POINTER(Tune), ctypes.POINTER(Output), vp
    ]
    L.psk_soft_tune_step.argtypes = [ctypes.c_double]
    L.psk_soft_tune_step.restype = u64
    L.psk_soft_tune_advance.argtypes = [u64, u64, u64]
    L.psk_soft_tune_advance.restype = u64
    L.psk_soft_tune_apply.argtypes = [ctypes.POINTER(Tune), vp, u64, vp]
    L.psk_soft_process_device_resampled.argtypes = [
        vp, u32, u32, ctypes.POINTER(Packet), ctypes.POINTER(u64), ctypes.POINTER(Tune), ctypes.POINTER(Resample), ctypes.POINTER(Output), vp
    ]
    L.psk_soft_resample_get_history.argtypes = [vp, u32, vp]
    L.psk_soft_resample_set_history.argtypes = [vp, u32, vp]
    L.psk_soft_resample_step.argtypes = [ctypes.c_double]
    L.psk_soft_resample_step.restype = u64
    L.psk_soft_resample_count.argtypes = [ctypes.POINTER(Resample), u64]
    L.psk_soft_resample_count.restype = u64
    L.psk_soft_resample_advance.argtypes = [ctypes.POINTER(Resample), u64]
    L.psk_soft_resample_advance.restype = u64
    L.psk_soft_resample_apply.argtypes = [ctypes.POINTER(Resample), vp, vp, u64, vp, vp]
    L.psk_soft_resample_piece.argtypes = []
    L.psk_soft_resample_piece.restype = u32
    L.psk_soft_fir_define.argtypes = [vp, u32, vp, u32]
    L.psk_soft_process_device_filtered.argtypes = [
        vp, u32, u32, ctypes.POINTER(Packet), ctypes.POINTER(u64), ctypes.POINTER(Tune), ctypes.POINTER(Fir), ctypes.POINTER(Resample),
        ctypes.POINTER(Output), vp
    ]
    L.psk_soft_fir_get_history.argtypes = [vp, u32, vp]
    L.psk_soft_fir_set_history.argtypes = [vp, u32, vp]
    L.psk_soft_fir_count.argtypes = [ctypes.POINTER(Fir), u64]
    L.psk_soft_fir_count.restype = u64
    L.psk_soft_fir_advance.argtypes = [ctypes.POINTER(Fir), u64]
    L.psk_soft_fir_advance.restype = u32
    L.psk_soft_fir_apply.argtypes = [ctypes.POINTER(Fir), vp, u32, vp, vp, u64, vp, vp]
    L.psk_soft_fir_piece.argtypes = [u32]
    L.psk_soft_fir_piece.restype = u32
    L.psk_soft_process_host.argtypes = [vp, u32, u32, ctypes.POINTER(Packet), ctypes.POINTER(Output)]
    L.psk_soft_synchronize.argtypes = [vp]
    L.psk_soft_join.argtypes = [vp, vp]
    L.psk_soft_get_stats.argtypes = [vp, ctypes.POINTER(Stats)]
    L.psk_soft_get_channel_stats.argtypes = [vp, u32, u32, ctypes.POINTER(Stats)]
    L.psk_soft_set_force_sequential.argtypes = [vp, i32]
    L.psk_soft_set_option.argtypes = [vp, i32, i32]
    L.psk_soft_state_bytes.argtypes = [vp]
    L.psk_soft_state_bytes.restype = u64
    L.psk_soft_export_state.argtypes = [vp, u32, vp, u64]
    L.psk_soft_import_state.argtypes = [vp, u32, vp, u64]
    L.psk_soft_peek.argtypes = [vp, u32, ctypes.POINTER(u64), ctypes.POINTER(u64), ctypes.POINTER(u64)]
    L.psk_soft_host_alloc.argtypes = [ctypes.c_size_t]
    L.psk_soft_host_alloc.restype = vp
    L.psk_soft_host_free.argtypes = [vp]
    L.psk_soft_device_alloc.argtypes = [vp, ctypes.c_size_t]
    L.psk_soft_device_alloc.restype = vp
    L.psk_soft_device_free.argtypes = [vp, vp]
    L.psk_soft_device_upload.argtypes = [vp, vp, vp, ctypes.c_size_t]
    L.psk_soft_device_download.argtypes = [vp, vp, vp, ctypes.c_size_t]
    L.psk_soft_probe_read_ms.argtypes = [vp, vp, u64, i32, ctypes.POINTER(ctypes.c_double)]
    L.psk_soft_quality_bytes.argtypes = []
    L.psk_soft_quality_bytes.restype = u64
    L.psk_soft_get_quality.argtypes = [vp, u32, u32, ctypes.POINTER(Quality)]
    L.psk_soft_quality_derive.argtypes = [ctypes.POINTER(Quality), ctypes.POINTER(QualityDerived)]
    L.psk_soft_acquire_device.argtypes = [vp, u32, u32, ctypes.POINTER(Packet), ctypes.POINTER(u64), ctypes.POINTER(Tune), vp]
    L.psk_soft_get_acquire.argtypes = [vp, u32, u32, ctypes.POINTER(Acquire)]
    L.psk_soft_acquire_derive.argtypes = [ctypes.POINTER(Acquire), ctypes.POINTER(AcquireDerived)]
    L.psk_soft_acquire_host.argtypes = [ctypes.c_uint16, ctypes.POINTER(Tune), vp, u64, ctypes.POINTER(Acquire)]
    L.psk_soft_acquire_bytes.argtypes = []
    L.psk_soft_acquire_bytes.restype = u64
    L.psk_soft_acquire_piece.argtypes = []
    L.psk_soft_acquire_piece.restype = u32
    L.psk_soft_symrate_device.argtypes = [vp, u32, u32, ctypes.POINTER(Packet), ctypes.POINTER(u64), ctypes.POINTER(Tune), vp]
    L.psk_soft_get_symrate.argtypes = [vp, u32, u32, ctypes.POINTER(Symrate)]
    L.psk_soft_symrate_derive.argtypes = [ctypes.POINTER(Symrate), ctypes.POINTER(SymrateDerived)]
    L.psk_soft_symrate_host.argtypes = [ctypes.c_uint16, ctypes.POINTER(Tune), vp, u64, ctypes.POINTER(Symrate)]
    L.psk_soft_symrate_bytes.argtypes = []
    L.psk_soft_symrate_bytes.restype = u64
    L.psk_soft_symrate_piece.argtypes = []
    L.psk_soft_symrate_piece.restype = u32
    L.psk_soft_sync_define.argtypes = [vp, u32, vp, u32]
    L.psk_soft_sync_device.argtypes = [vp, u32, u32, ctypes.POINTER(SyncIn), vp]
    L.psk_soft_get_sync.argtypes = [vp, u32, u32, ctypes.POINTER(SyncRecord)]
    L.psk_soft_sync_get_history.argtypes = [vp, u32, vp]
    L.psk_soft_sync_set_history.argtypes = [vp, u32, vp]
    L.psk_soft_sync_derive.argtypes = [ctypes.POINTER(SyncHit), ctypes.c_uint16, u32, ctypes.c_float, ctypes.POINTER(SyncDerived)]
    L.psk_soft_sync_host.argtypes = [vp, u32, ctypes.c_float, u32, vp, vp, u64, ctypes.POINTER(SyncRecord), vp]
    L.psk_soft_sync_bytes.argtypes = []
    L.psk_soft_sync_bytes.restype = u64
    L.psk_soft_sync_in_bytes.argtypes = []
    L.psk_soft_sync_in_bytes.restype = u64
    L.psk_soft_sync_piece.argtypes = []
    L.psk_soft_sync_piece.restype = u32
    L.psk_soft_demap_define.argtypes = [vp, u32, u32, vp, vp]
    L.psk_soft_demap_device.argtypes = [vp, u32, ctypes.POINTER(DemapIn), vp]
    L.psk_soft_get_demap.argtypes = [vp, u32, u32, ctypes.POINTER(DemapRecord)]
    L.psk_soft_demap_host.argtypes = [vp, vp, u32, ctypes.POINTER(DemapIn), vp, ctypes.POINTER(DemapRecord)]
    L.psk_soft_demap_gain.argtypes = [ctypes.POINTER(SyncDerived), u32, u32, ctypes.POINTER(ctypes.c_float)]
    L.psk_soft_demap_bytes.argtypes = []
    L.psk_soft_demap_bytes.restype = u64
    L.psk_soft_demap_in_bytes.argtypes = []
    L.psk_soft_demap_in_bytes.restype = u64
    L.psk_soft_demap_piece.argtypes = []
    L.psk_soft_demap_piece.restype = u32
    L.psk_soft_viterbi_define.argtypes = [vp, u32, u32, u32, vp, u32, u32]
    L.psk_soft_viterbi_device.argtypes = [vp, u32, ctypes.POINTER(ViterbiIn), vp]
    L.psk_soft_get_viterbi.argtypes = [vp, u32, u32, ctypes.POINTER(ViterbiRecord)]
    L.psk_soft_viterbi_host.argtypes = [u32, u32, vp, u32, u32, ctypes.POINTER(ViterbiIn), ctypes.POINTER(ViterbiRecord)]
    L.psk_soft_viterbi_encode_host.argtypes = [u32, u32, vp, u32, u32, vp, u32, vp]
    L.psk_soft_viterbi_count.argtypes = [u32, u32, u32, u32, u64]
    L.psk_soft_viterbi_count.restype = u64
    L.psk_soft_viterbi_bytes.argtypes = []
    L.psk_soft_viterbi_bytes.restype = u64
    L.psk_soft_viterbi_in_bytes.argtypes = []
    L.psk_soft_viterbi_in_bytes.restype = u64
    L.psk_soft_rs_define.argtypes = [vp, u32, u32, u32, u32, u32, u32, u32, vp, u32]
    L.psk_soft_rs_device.argtypes = [vp, u32, ctypes.POINTER(RsIn), vp]
    L.psk_soft_get_rs.argtypes = [vp, u32, u32, ctypes.POINTER(RsRecord)]
    L.psk_soft_rs_host.argtypes = [u32, u32, u32, u32, u32, u32, vp, u32, ctypes.POINTER(RsIn), ctypes.POINTER(RsRecord)]
    L.psk_soft_rs_encode_host.argtypes = [u32, u32, u32, u32, u32, u32, vp, u32, vp, vp]
    L.psk_soft_rs_bytes.argtypes = []
    L.psk_soft_rs_bytes.restype = u64
    L.psk_soft_rs_in_bytes.argtypes = []
    L.psk_soft_rs_in_bytes.restype = u64
    L.psk_soft_frame_word_define.argtypes = [vp, u32, u32, u64, u64]
    L.psk_soft_frame_search_device.argtypes = [vp, u32, ctypes.POINTER(FrameSearchIn), vp]
    L.psk_soft_get_frame_search.argtypes = [vp, u32, u32, ctypes.POINTER(FrameSearchRecord)]
    L.psk_soft_frame_search_host.argtypes = [u32, u64, u64, ctypes.POINTER(FrameSearchIn), ctypes.POINTER(FrameSearchRecord)]
    L.psk_soft_frame_tile.argtypes = []
    L.psk_soft_frame_tile.restype = u32
    L.psk_soft_frame_format_define.argtypes = [vp, u32, u32, u32, vp]
    L.psk_soft_frame_cut_device.argtypes = [vp, u32, ctypes.POINTER(FrameCutIn), vp]
    L.psk_soft_get_frame_cut.argtypes = [vp, u32, u32, ctypes.POINTER(FrameCutRecord)]
    L.psk_soft_frame_cut_host.argtypes = [u32, u32, vp, ctypes.POINTER(FrameCutIn), ctypes.POINTER(FrameCutRecord)]
    L.psk_soft_frame_span.argtypes = [u32, u32, u32, u32]
    L.psk_soft_frame_span.restype = u64
    for _n in ("search", "search_in", "cut", "cut_in"):
        _f = getattr(L, "psk_soft_frame_%s_bytes" % _n)
        _f.argtypes = []
        _f.restype = u64
    _lib = L
    return L


def host_alloc(n, dtype):
    """A numpy array of `n` elements in pinned host memory (psk_soft_host_alloc): hand its
    .ctypes.data to Handle.process_device.  Keep the returned array alive; free with host_free."""
    import numpy as np

    dt = np.dtype(dtype)
    p = load().psk_soft_host_alloc(int(n) * dt.itemsize)
    if not p:
        raise MemoryError("psk_soft_host_alloc failed: " + load().psk_soft_last_error().decode())
    buf = (ctypes.c_char * (int(n) * dt.itemsize)).from_address(p)
    arr = np.frombuffer(buf, dtype=dt)
    return arr


def host_free(arr):
    load().psk_soft_host_free(ctypes.c_void_p(arr.ctypes.data))


FORMAT_SAMPLE_BYTES = {FORMAT_CF32: 8, FORMAT_CS16: 4, FORMAT_CS8: 2, FORMAT_CF16: 4}


def frame_major_packets(base, frames, width, first_column, n_channels, fmt=FORMAT_CF32, xdelta=1.0, sriChanged=False):
    """Packets and strides of `n_channels` adjacent channels of a frame-major matrix (a channelizer's output: `frames` rows
    of `width` complex samples of format `fmt`, one sample of every channel per row) at the device address `base`: channel i
    is column first_column + i.  `frames` is a count for all channels or one count per channel (ragged lengths).  Returns
    (Packet array, uint64 stride array) for Handle.process_device_strided; set the remaining packet fields as needed."""
    if first_column < 0 or first_column + n_channels > width:
        raise ValueError("columns %d .. %d are outside a matrix %d wide" % (first_column, first_column + n_channels, width))
    sb = FORMAT_SAMPLE_BYTES[fmt]
    pk = (Packet * n_channels)()
    strides = (ctypes.c_uint64 * n_channels)()
    for i in range(n_channels):
        n = int(frames if np.isscalar(frames) else frames[i])
        pk[i].data = int(base) + sb * (first_column + i)
        pk[i].n_floats = 2 * n
        pk[i].sri_xdelta = float(xdelta)
        pk[i].sri_mode = 1
        pk[i].sriChanged = int(bool(sriChanged))
        pk[i].present = 1
        pk[i].format = fmt
        strides[i] = width
    return pk, strides


def _check(status):
    if status != OK:
        raise PskSoftError(status, load().psk_soft_last_error().decode("utf-8", "replace"))


def quality_derive(q):
    """psk_soft_quality_derive of one Quality record: dict of lock, snr_db, mean_energy, index_change_rate (NaN where undefined)."""
    d = QualityDerived()
    _check(load().psk_soft_quality_derive(ctypes.byref(q), ctypes.byref(d)))
    return {k: getattr(d, k) for k, _ in QualityDerived._fields_}


def tune_step(cycles_per_sample):
    """psk_soft_tune_step: the step word (turns x 2^64) of a shift by `cycles_per_sample`; negate a channel's offset to remove it."""
    return int(load().psk_soft_tune_step(float(cycles_per_sample)))


def tune_advance(phase, step, n_complex):
    """psk_soft_tune_advance: the phase word of the next packet of a continuous stream."""
    return int(load().psk_soft_tune_advance(int(phase), int(step), int(n_complex)))


def tune_apply(phase, step, iq):
    """psk_soft_tune_apply on the host: interleaved float32 I/Q in, the shifted interleaved float32 I/Q out (a new array;
    an odd last element is dropped)."""
    x = np.ascontiguousarray(iq, np.float32)
    n = x.size // 2
    y = np.empty(2 * n, np.float32)
    t = Tune(int(phase), int(step))
    _check(load().psk_soft_tune_apply(ctypes.byref(t), x.ctypes.data, n, y.ctypes.data))
    return y


def _resample(rs):
    """a Resample from a Resample or a (pos, step[, flags]) tuple"""
    return rs if isinstance(rs, Resample) else Resample(int(rs[0]), int(rs[1]), int(rs[2]) if len(rs) > 2 else 0, 0)


def resample_step(in_per_out):
    """psk_soft_resample_step: the step word (input samples per output sample x 2^32); 0 outside [0.5, 2] or non-finite.  For a
    signal at sps samples per symbol demodulated with samplesPerBaud S: resample_step(sps / S)."""
    return int(load().psk_soft_resample_step(float(in_per_out)))


def resample_count(rs, n_complex):
    """psk_soft_resample_count: the outputs of a packet of n_complex samples.  rs: a Resample or (pos, step[, flags])."""
    r = _resample(rs)
    return int(load().psk_soft_resample_count(ctypes.byref(r), int(n_complex)))


def resample_advance(rs, n_complex):
    """psk_soft_resample_advance: pos of the next packet of a continuous stream."""
    r = _resample(rs)
    return int(load().psk_soft_resample_advance(ctypes.byref(r), int(n_complex)))


def resample_apply(rs, iq, history=None):
    """psk_soft_resample_apply on the host: interleaved float32 I/Q in (an odd last element is dropped), history None (zeros)
    or six floats.  Returns (the resampled interleaved float32 I/Q, the history behind the packet as six float32)."""
    r = _resample(rs)
    x = np.ascontiguousarray(iq, np.float32)
    n = x.size // 2
    y = np.empty(2 * resample_count(r, n), np.float32)
    hi = None if history is None else np.ascontiguousarray(history, np.float32)
    if hi is not None and hi.size != 6:
        raise ValueError("a history is three complex samples: six floats")
    ho = np.empty(6, np.float32)
    _check(load().psk_soft_resample_apply(ctypes.byref(r), None if hi is None else hi.ctypes.data, x.ctypes.data, n, y.ctypes.data, ho.ctypes.data))
    return y, ho


def resample_piece():
    """Outputs of one workgroup's piece of the device's resample pass (psk_soft_resample_piece)."""
    return int(load().psk_soft_resample_piece())


def _fir(f):
    """a Fir from a Fir or a (filter, decim, pos[, flags]) tuple"""
    return f if isinstance(f, Fir) else Fir(int(f[0]), int(f[1]), int(f[2]), int(f[3]) if len(f) > 3 else 0)


def fir_count(f, n_complex):
    """psk_soft_fir_count: the outputs of a packet of n_complex samples.  f: a Fir or (filter, decim, pos[, flags])."""
    r = _fir(f)
    return int(load().psk_soft_fir_count(ctypes.byref(r), int(n_complex)))


def fir_advance(f, n_complex):
    """psk_soft_fir_advance: pos of the next packet of a continuous stream."""
    r = _fir(f)
    return int(load().psk_soft_fir_advance(ctypes.byref(r), int(n_complex)))


def fir_apply(f, taps, iq, history=None):
    """psk_soft_fir_apply on the host: the taps (1 .. 128 floats), interleaved float32 I/Q in (an odd last element is dropped),
    history None (zeros) or 254 floats.  f.filter is not looked at.  Returns (the filtered interleaved float32 I/Q, the history
    behind the packet as 254 float32)."""
    r = _fir(f)
    h = np.ascontiguousarray(taps, np.float32)
    x = np.ascontiguousarray(iq, np.float32)
    n = x.size // 2
    n_out = 0 if r.pos >= n or not r.decim else (n - r.pos + r.decim - 1) // r.decim
    y = np.empty(2 * n_out, np.float32)
    hi = None if history is None else np.ascontiguousarray(history, np.float32)
    if hi is not None and hi.size != FIR_HISTORY_FLOATS:
        raise ValueError("a history is 127 complex samples: 254 floats")
    ho = np.empty(FIR_HISTORY_FLOATS, np.float32)
    _check(load().psk_soft_fir_apply(ctypes.byref(r), h.ctypes.data, h.size, None if hi is None else hi.ctypes.data, x.ctypes.data, n,
                                     y.ctypes.data, ho.ctypes.data))
    return y, ho


def fir_piece(decim):
    """Outputs of one workgroup's piece of the device's filter pass at that decimation (psk_soft_fir_piece)."""
    return int(load().psk_soft_fir_piece(int(decim)))


def acquire_derive(rec):
    """psk_soft_acquire_derive of one Acquire record: dict of offset_cycles_per_sample, coherence, mean_energy (NaN where
    undefined) and lags_used.  To take the offset out: tune step += tune_step(-offset_cycles_per_sample)."""
    d = AcquireDerived()
    _check(load().psk_soft_acquire_derive(ctypes.byref(rec), ctypes.byref(d)))
    return {k: getattr(d, k) for k, _ in AcquireDerived._fields_ if k != "pad"}


def acquire_host(M, iq, tune=None):
    """psk_soft_acquire_host: the Acquire record of interleaved float32 I/Q on the host (an odd last element is dropped).
    tune: None or a (phase, step) pair."""
    x = np.ascontiguousarray(iq, np.float32)
    rec = Acquire()
    t = Tune(int(tune[0]), int(tune[1])) if tune is not None else None
    _check(load().psk_soft_acquire_host(int(M), ctypes.byref(t) if t is not None else None, x.ctypes.data, x.size // 2, ctypes.byref(rec)))
    return rec


def acquire_piece():
    """Samples of one piece of the device's fold (psk_soft_acquire_piece)."""
    return int(load().psk_soft_acquire_piece())


def symrate_derive(rec):
    """psk_soft_symrate_derive of one Symrate record: dict of samples_per_symbol, step_ratio, coherence, mean_level (NaN where
    undefined), detector (0: e, 1: g, -1: none) and lags_used.  To bring the signal to samplesPerBaud samples a symbol:
    resample step = resample_step(step_ratio)."""
    d = SymrateDerived()
    _check(load().psk_soft_symrate_derive(ctypes.byref(rec), ctypes.byref(d)))
    return {k: getattr(d, k) for k, _ in SymrateDerived._fields_}


def symrate_host(S, iq, tune=None):
    """psk_soft_symrate_host: the Symrate record of interleaved float32 I/Q on the host (an odd last element is dropped) for
    samplesPerBaud S.  tune: None or a (phase, step) pair."""
    x = np.ascontiguousarray(iq, np.float32)
    rec = Symrate()
    t = Tune(int(tune[0]), int(tune[1])) if tune is not None else None
    _check(load().psk_soft_symrate_host(int(S), ctypes.byref(t) if t is not None else None, x.ctypes.data, x.size // 2, ctypes.byref(rec)))
    return rec


def symrate_piece():
    """Blocks of one piece of the device's fold (psk_soft_symrate_piece)."""
    return int(load().psk_soft_symrate_piece())


def sync_host(word, threshold, soft, flags=0, hist_in=None):
    """psk_soft_sync_host: the search of one row on the host.  word and soft are interleaved float32 (re, im) (an odd last element
    is dropped), hist_in None (zeros) or 254 floats.  Returns (SyncRecord, the history behind the row: 254 float32)."""
    w = np.ascontiguousarray(word, np.float32)
    x = np.ascontiguousarray(soft, np.float32)
    hin = None
    if hist_in is not None:
        hin = np.ascontiguousarray(hist_in, np.float32)
        if hin.size != SYNC_HISTORY_FLOATS:
            raise ValueError("a history is 127 complex symbols: 254 floats")
    rec = SyncRecord()
    hout = np.zeros(SYNC_HISTORY_FLOATS, np.float32)
    _check(load().psk_soft_sync_host(w.ctypes.data if w.size else None, w.size // 2, float(threshold), int(flags),
                                     hin.ctypes.data if hin is not None else None, x.ctypes.data if x.size else None, x.size // 2,
                                     ctypes.byref(rec), hout.ctypes.data))
    return rec, hout


def sync_word_energy(word):
    """Ew of a word: the float32 sum, in index order, of re*re + im*im (what sync_derive takes)."""
    w = np.ascontiguousarray(word, np.float32).reshape(-1, 2)
    s = np.float32(0)
    for j, (a, b) in enumerate(w):
        t = np.float32(np.float32(a * a) + np.float32(b * b))
        s = t if j == 0 else np.float32(s + t)
    return float(s)


def sync_derive(hit, M, L, Ew):
    """psk_soft_sync_derive of one SyncHit: dict of angle, residual, amplitude, metric (NaN for an all-zero hit) and rotation
    (0 .. M-1; -1 for an all-zero hit)."""
    d = SyncDerived()
    _check(load().psk_soft_sync_derive(ctypes.byref(hit), int(M), int(L), float(Ew), ctypes.byref(d)))
    return {k: getattr(d, k) for k, _ in SyncDerived._fields_ if k != "pad"}


def sync_piece():
    """Windows of one piece of the device's fold (psk_soft_sync_piece)."""
    return int(load().psk_soft_sync_piece())


def _sync_in(s):
    return s if isinstance(s, SyncIn) else SyncIn(*s)


def _demap_map(points, labels):
    p = np.ascontiguousarray(points, np.float32).reshape(-1)
    lab = np.ascontiguousarray(labels, np.uint8).reshape(-1)
    if p.size != 2 * lab.size:
        raise ValueError("a map is M points (2 M floats) and M labels")
    return p, lab


def demap_host(points, labels, soft, pos, count, gain, scale, flags=0, front=None):
    """psk_soft_demap_host: one segment on the host.  points: M interleaved float32 (re, im); labels: M labels; soft: the row,
    interleaved float32 (an odd last element is dropped); the segment is its symbols [pos, pos + count); gain: (re, im);
    flags: DEMAP_I8, DEMAP_FRONT; front: None (zeros) or the 254 floats in front of the row (read with DEMAP_FRONT where pos < 0).
    Returns (the count * B values: int8 with DEMAP_I8, float32 without, the DemapRecord)."""
    p, lab = _demap_map(points, labels)
    x = np.ascontiguousarray(soft, np.float32)
    fr = None
    if front is not None:
        fr = np.ascontiguousarray(front, np.float32)
        if fr.size != 2 * DEMAP_FRONT_SYMBOLS:
            raise ValueError("the symbols in front of a row are 127 complex symbols: 254 floats")
    B = max(int(lab.size).bit_length() - 1, 0)
    out = np.zeros(max(int(count) * B, 1), np.int8 if flags & DEMAP_I8 else np.float32)
    k = DemapIn(x.ctypes.data if x.size else None, x.size // 2, int(pos), out.ctypes.data, int(count), 0, 1, int(flags),
                float(gain[0]), float(gain[1]), float(scale), 0)
    rec = DemapRecord()
    _check(load().psk_soft_demap_host(p.ctypes.data if p.size else None, lab.ctypes.data if lab.size else None, lab.size, ctypes.byref(k),
                                      fr.ctypes.data if fr is not None else None, ctypes.byref(rec)))
    return out[: int(count) * B], rec


def demap_gain(derived, M, flags=0):
    """psk_soft_demap_gain: the (re, im) gain, two float32, that undoes a derived hit -- a SyncDerived or the dict sync_derive
    returns -- for constellation size M.  flags: DEMAP_GAIN_RESIDUAL, DEMAP_GAIN_UNIT."""
    d = derived
    if not isinstance(d, SyncDerived):
        d = SyncDerived(derived["angle"], derived["residual"], derived["amplitude"], derived["metric"], derived["rotation"], 0)
    g = (ctypes.c_float * 2)()
    _check(load().psk_soft_demap_gain(ctypes.byref(d), int(M), int(flags), g))
    return np.array([g[0], g[1]], np.float32)


def demap_piece():
    """Symbols of one piece of the device's fold (psk_soft_demap_piece): the unit of the records' summation order."""
    return int(load().psk_soft_demap_piece())


def _demap_in(s):
    return s if isinstance(s, DemapIn) else DemapIn(*s)


def _viterbi_polys(g):
    return np.ascontiguousarray(g, np.uint32).reshape(-1)


def viterbi_count(K, g, P, keep, n_steps):
    """psk_soft_viterbi_count: the LLRs (kept code bits) of a frame of n_steps steps of the code (K, polynomials g, puncture
    period P, keep mask); 0 for a puncture pattern psk_soft_viterbi_define refuses."""
    return int(load().psk_soft_viterbi_count(int(K), int(_viterbi_polys(g).size), int(P), int(keep), int(n_steps)))


def viterbi_encode(K, g, P, keep, bits):
    """psk_soft_viterbi_encode_host: the code bits (uint8 0 / 1, punctured, in order of (t, j)) of the input bits, from state 0;
    a terminated frame's K-1 zeros are the caller's to append."""
    pol = _viterbi_polys(g)
    u = np.ascontiguousarray(bits, np.uint8).reshape(-1)
    out = np.zeros(max(viterbi_count(K, pol, P, keep, u.size), 1), np.uint8)
    _check(load().psk_soft_viterbi_encode_host(int(K), int(pol.size), pol.ctypes.data if pol.size else None, int(P), int(keep),
                                               u.ctypes.data if u.size else None, int(u.size), out.ctypes.data))
    return out[: viterbi_count(K, pol, P, keep, u.size)]


def viterbi_host(K, g, P, keep, llr, n_steps, flags=0):
    """psk_soft_viterbi_host: one frame on the host.  llr: the frame's int8 LLRs (at least viterbi_count of them).  Returns (the
    output bytes: n_bits uint8, or ceil(n_bits / 8) with VITERBI_PACKED, the ViterbiRecord)."""
    pol = _viterbi_polys(g)
    x = np.ascontiguousarray(llr, np.int8).reshape(-1)
    if x.size < viterbi_count(K, pol, P, keep, n_steps):
        raise ValueError("fewer LLRs than the frame's steps hold")
    out = np.zeros(int(n_steps) + 8, np.uint8)
    k = ViterbiIn(x.ctypes.data if x.size else out.ctypes.data, out.ctypes.data, int(n_steps), 1, int(flags), 0)
    rec = ViterbiRecord()
    _check(load().psk_soft_viterbi_host(int(K), int(pol.size), pol.ctypes.data if pol.size else None, int(P), int(keep), ctypes.byref(k),
                                        ctypes.byref(rec)))
    n = int(rec.n_bits)
    return out[: (n + 7) // 8 if flags & VITERBI_PACKED else n].copy(), rec


def _viterbi_in(s):
    return s if isinstance(s, ViterbiIn) else ViterbiIn(*s)


def _rs_mask(mask):
    m = np.zeros(0, np.uint8) if mask is None else np.ascontiguousarray(mask, np.uint8).reshape(-1)
    return m, (m.ctypes.data if m.size else None)


def rs_encode_host(gfpoly, fcr, prim, nroots, n, depth, data, mask=None):
    """psk_soft_rs_encode_host: the frame (n * depth uint8) of the (n - nroots) * depth data bytes -- data[i * depth + j] is byte i
    of codeword j --, systematic, interleaved, the mask (None: none) applied."""
    m, mp = _rs_mask(mask)
    k = int(n) - int(nroots)
    d = np.ascontiguousarray(data, np.uint8).reshape(-1)
    if k > 0 and 1 <= int(depth) <= RS_MAX_DEPTH and d.size != k * int(depth):
        raise ValueError("data must hold (n - nroots) * depth bytes")
    out = np.zeros(255 * RS_MAX_DEPTH, np.uint8)
    _check(load().psk_soft_rs_encode_host(int(gfpoly), int(fcr), int(prim), int(nroots), int(n), int(depth), mp, int(m.size),
                                          d.ctypes.data if d.size else None, out.ctypes.data))
    return out[: int(n) * int(depth)].copy()


def rs_host(gfpoly, fcr, prim, nroots, n, depth, frame, mask=None, flags=0):
    """psk_soft_rs_host: one frame on the host.  frame: its n * depth bytes.  Returns (the output bytes: (n - nroots) * depth
    uint8, or n * depth with RS_WITH_PARITY, the RsRecord)."""
    m, mp = _rs_mask(mask)
    x = np.ascontiguousarray(frame, np.uint8).reshape(-1)
    if 1 <= int(n) <= 255 and 1 <= int(depth) <= RS_MAX_DEPTH and x.size < int(n) * int(depth):
        raise ValueError("fewer bytes than the frame holds")
    out = np.zeros(255 * RS_MAX_DEPTH, np.uint8)
    k = RsIn(x.ctypes.data if x.size else out.ctypes.data, out.ctypes.data, 1, int(flags), (ctypes.c_uint32 * 2)(0, 0))
    rec = RsRecord()
    _check(load().psk_soft_rs_host(int(gfpoly), int(fcr), int(prim), int(nroots), int(n), int(depth), mp, int(m.size), ctypes.byref(k),
                                   ctypes.byref(rec)))
    nb = int(rec.n if flags & RS_WITH_PARITY else rec.k) * int(rec.depth)
    return out[:nb].copy(), rec


def _rs_in(s):
    if isinstance(s, RsIn):
        return s
    s = tuple(s)
    return RsIn(s[0], s[1], s[2], s[3] if len(s) > 3 else 0, (ctypes.c_uint32 * 2)(0, 0))


def _frame_table(table):
    if table is None:
        return None, None
    t = np.ascontiguousarray(table, np.uint8).reshape(-1)
    if t.size != 256:
        raise ValueError("a table is 256 bytes")
    return t, t.ctypes.data


def _u32x(n):
    return (ctypes.c_uint32 * n)(*([0] * n))


def frame_search_host(length, word, care, bits, n_bits, bit0=0, max_diff=0, period=0):
    """psk_soft_frame_search_host: one stream on the host.  bits: the packed bytes that hold the stream bits bit0 .. bit0 + n_bits - 1.
    Returns the FrameSearchRecord."""
    x = np.ascontiguousarray(bits, np.uint8).reshape(-1)
    if 8 * x.size < int(bit0) + int(n_bits):
        raise ValueError("fewer bytes than the stream's bits")
    k = FrameSearchIn(x.ctypes.data if x.size else None, int(bit0), int(n_bits), 1, int(max_diff), int(period), 0, _u32x(3))
    rec = FrameSearchRecord()
    _check(load().psk_soft_frame_search_host(int(length), int(word), int(care), ctypes.byref(k), ctypes.byref(rec)))
    return rec


def frame_span(branches, cell, branch0, n_bytes):
    """psk_soft_frame_span: the stream bytes from `bit` that a frame of n_bytes bytes touches (0: refused arguments)."""
    return int(load().psk_soft_frame_span(int(branches), int(cell), int(branch0), int(n_bytes)))


def frame_cut_host(branches, cell, bits, bit, n_bytes, branch0=0, table=None, flags=0):
    """psk_soft_frame_cut_host: one frame on the host.  bits: the packed bytes of the stream, which must hold frame_span(...) bytes
    from `bit`.  Returns (the n_bytes output bytes, the FrameCutRecord)."""
    x = np.ascontiguousarray(bits, np.uint8).reshape(-1)
    span = frame_span(branches, cell, branch0, n_bytes)
    if span and 8 * x.size < int(bit) + 8 * span:
        raise ValueError("fewer bytes than the frame's span")
    t, tp = _frame_table(table)
    out = np.zeros(max(int(n_bytes), 1) if span else 1, np.uint8)
    k = FrameCutIn(x.ctypes.data if x.size else None, int(bit), out.ctypes.data, int(n_bytes), 0, int(branch0), int(flags), _u32x(2))
    rec = FrameCutRecord()
    _check(load().psk_soft_frame_cut_host(int(branches), int(cell), tp, ctypes.byref(k), ctypes.byref(rec)))
    return out[: int(rec.n_bytes)].copy(), rec


def _frame_search_in(s):
    if isinstance(s, FrameSearchIn):
        return s
    s = tuple(s) + (0, 0)
    return FrameSearchIn(s[0], s[1], s[2], s[3], s[4], s[5], 0, _u32x(3))


def _frame_cut_in(s):
    if isinstance(s, FrameCutIn):
        return s
    s = tuple(s) + (0, 0, 0)
    return FrameCutIn(s[0], s[1], s[2], s[3], s[4], s[5], s[6], _u32x(2))


class Handle:
    """A batch of channels on one GPU (psk_soft_handle_t)."""

    def __init__(self, n_channels, device=0, max_window_samples=16384, max_phase_avg=512, max_packet_complex=1 << 20):
        L = load()
        self._L = L
        self.n_channels = int(n_channels)
        self.device = device
        lim = Limits(max_window_samples, max_phase_avg, max_packet_complex)
        h = ctypes.c_void_p()
        _check(L.psk_soft_create(int(device), self.n_channels, ctypes.byref(lim), ctypes.byref(h)))
        self._h = h
        self._owned = True

    @classmethod
    def borrow(cls, pointer, n_channels, device=None):
        """A Handle around a psk_soft_handle_t that somebody else owns (the component of psk_soft_amd/sandbox.py): every method
        works on it, close() only lets go of the pointer.  Valid for as long as the owner keeps the handle."""
        h = cls.__new__(cls)
        h._L = load()
        h.n_channels = int(n_channels)
        h.device = device
        h._h = ctypes.c_void_p(pointer)
        h._owned = False
        return h

    def close(self):
        if getattr(self, "_h", None):
            if self._owned:
                self._L.psk_soft_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- properties -------------------------------------------------------------------
    def query(self, ch):
        p = Props()
        _check(self._L.psk_soft_query(self._h, ch, ctypes.byref(p)))
        return p

    def configure(self, ch0, props):
        """props: one Props or dict for every channel in [ch0, ch0+len(props))."""
        arr = (Props * len(props))()
        for i, p in enumerate(props):
            if isinstance(p, dict):
                cur = self.query(ch0 + i)
                for k in PROP_NAMES:
                    setattr(arr[i], k, int(p.get(k, getattr(cur, k))))
            else:
                arr[i] = p
        _check(self._L.psk_soft_configure(self._h, ch0, len(props), arr))

    def configure_all(self, **kw):
        cur = self.query(0)
        p = Props()
        for k in PROP_NAMES:
            setattr(p, k, int(kw.get(k, getattr(cur, k))))
        arr = (Props * self.n_channels)(*([p] * self.n_channels))
        _check(self._L.psk_soft_configure(self._h, 0, self.n_channels, arr))

    def fire_listener(self, ch, which):
        _check(self._L.psk_soft_fire_listener(self._h, ch, which))

    OPT_QPSK_SIGN_BITMAP = 1
    OPT_CONCURRENT_CLASSES = 2
    OPT_TIME_TILED = 3  # 0 never, 1 where it pays (default), 2 wherever the kernels exist
    OPT_DEFERRED_JOIN = 5  # mixed window classes: the side streams are joined by join() / synchronize(), not by every call
    OPT_PARALLEL_FIT = 4  # tiled calls: 0 fit block by block, 1 parallel fit with the second round on demand (default), 2 always

    OPT_QUALITY = 6  # 1: every process call ends with the per-channel reduction pass, see quality()
    OPT_FAR_FIT = 7  # 1: phaseAvg above 32640 on the fast path, the fit window in device memory (default 0: reference-order kernel)

    def set_option(self, option, value):
        _check(self._L.psk_soft_set_option(self._h, int(option), int(value)))

    def set_force_sequential(self, on):
        _check(self._L.psk_soft_set_force_sequential(self._h, int(bool(on))))

    def output_capacity(self, ch, n_complex):
        return int(self._L.psk_soft_output_capacity(self._h, ch, int(n_complex)))

    def peek(self, ch):
        a, b, c = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        _check(self._L.psk_soft_peek(self._h, ch, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
        return {"ring_len": a.value, "index": b.value, "fit_len": c.value}

    # -- processing -------------------------------------------------------------------
    def process_device(self, ch0, pkts, outs, stream=None):
        """pkts / outs: ctypes arrays of Packet / Output holding DEVICE pointers."""
        _check(self._L.psk_soft_process_device(self._h, ch0, len(pkts), pkts, outs, ctypes.c_void_p(stream or 0)))

    def process_device_strided(self, ch0, pkts, strides, outs, stream=None):
        """process_device for packets whose complex samples lie strides[i] samples apart (frame-major channelizer output, see
        frame_major_packets): gathered on the GPU, then the ordinary call.  strides: None (all contiguous), a ctypes uint64
        array or a sequence of ints, one per packet."""
        if strides is not None and not isinstance(strides, ctypes.Array):
            strides = (ctypes.c_uint64 * len(pkts))(*[int(s) for s in strides])
        if strides is not None and len(strides) != len(pkts):
            raise ValueError("one stride per packet")
        _check(self._L.psk_soft_process_device_strided(self._h, ch0, len(pkts), pkts, strides, outs, ctypes.c_void_p(stream or 0)))

    def process_device_tuned(self, ch0, pkts, strides, tunes, outs, stream=None):
        """process_device_strided with a frequency shift per packet, applied on the GPU in front of the demodulator.  tunes:
        None (nothing tuned), a ctypes Tune array or a sequence of (phase, step) pairs, one per packet; (0, 0) leaves a packet
        untuned.  strides as for process_device_strided."""
        if strides is not None and not isinstance(strides, ctypes.Array):
            strides = (ctypes.c_uint64 * len(strides))(*[int(s) for s in strides])
        if tunes is not None and not isinstance(tunes, ctypes.Array):
            tunes = (Tune * len(tunes))(*[Tune(int(p), int(s)) for p, s in tunes])
        if (strides is not None and len(strides) != len(pkts)) or (tunes is not None and len(tunes) != len(pkts)):
            raise ValueError("one stride and one tune per packet")
        _check(self._L.psk_soft_process_device_tuned(self._h, ch0, len(pkts), pkts, strides, tunes, outs, ctypes.c_void_p(stream or 0)))

    def process_device_resampled(self, ch0, pkts, strides, tunes, resamples, outs, stream=None):
        """process_device_tuned with a fractional resampler per packet, applied on the GPU in front of the demodulator (and
        behind the frequency shift, in the same pass).  resamples: None (nothing resampled), a ctypes Resample array or a sequence
        of Resample / (pos, step[, flags]), one per packet; step 0 leaves a packet as it is.  Size the output rows with
        output_capacity(ch, resample_count(rs, n)).  strides and tunes as for process_device_tuned."""
        if strides is not None and not isinstance(strides, ctypes.Array):
            strides = (ctypes.c_uint64 * len(strides))(*[int(s) for s in strides])
        if tunes is not None and not isinstance(tunes, ctypes.Array):
            tunes = (Tune * len(tunes))(*[Tune(int(p), int(s)) for p, s in tunes])
        if resamples is not None and not isinstance(resamples, ctypes.Array):
            resamples = (Resample * len(resamples))(*[_resample(r) for r in resamples])
        if any(a is not None and len(a) != len(pkts) for a in (strides, tunes, resamples)):
            raise ValueError("one stride, one tune and one resample per packet")
        _check(self._L.psk_soft_process_device_resampled(self._h, ch0, len(pkts), pkts, strides, tunes, resamples, outs,
                                                         ctypes.c_void_p(stream or 0)))

    def resample_history(self, ch):
        """The resampler's history of channel ch (psk_soft_resample_get_history): six float32, three (re, im) pairs, oldest first."""
        out = np.zeros(6, np.float32)
        _check(self._L.psk_soft_resample_get_history(self._h, int(ch), out.ctypes.data))
        return out

    def set_resample_history(self, ch, six):
        """psk_soft_resample_set_history: replace the resampler's history of channel ch."""
        x = np.ascontiguousarray(six, np.float32)
        if x.size != 6:
            raise ValueError("a history is three complex samples: six floats")
        _check(self._L.psk_soft_resample_set_history(self._h, int(ch), x.ctypes.data))

    def fir_define(self, slot, taps):
        """psk_soft_fir_define: the taps (1 .. 128 floats, copied) of filter slot `slot` (0 .. 63); a packet names it as
        Fir.filter = slot + 1."""
        h = np.ascontiguousarray(taps, np.float32)
        _check(self._L.psk_soft_fir_define(self._h, int(slot), h.ctypes.data if h.size else None, h.size))

    def process_device_filtered(self, ch0, pkts, strides, tunes, firs, resamples, outs, stream=None):
        """process_device_resampled with a decimating real-tap FIR per packet, applied on the GPU behind the frequency shift and
        in front of the resampler.  firs: None (nothing filtered), a ctypes Fir array or a sequence of Fir / (filter, decim,
        pos[, flags]), one per packet; filter 0 leaves a packet as it is.  Size the output rows with output_capacity(ch,
        resample_count(rs, fir_count(f, n))).  strides, tunes and resamples as for process_device_resampled."""
        if strides is not None and not isinstance(strides, ctypes.Array):
            strides = (ctypes.c_uint64 * len(strides))(*[int(s) for s in strides])
        if tunes is not None and not isinstance(tunes, ctypes.Array):
            tunes = (Tune * len(tunes))(*[Tune(int(p), int(s)) for p, s in tunes])
        if firs is not None and not isinstance(firs, ctypes.Array):
            firs = (Fir * len(firs))(*[_fir(f) for f in firs])
        if resamples is not None and not isinstance(resamples, ctypes.Array):
            resamples = (Resample * len(resamples))(*[_resample(r) for r in resamples])
        if any(a is not None and len(a) != len(pkts) for a in (strides, tunes, firs, resamples)):
            raise ValueError("one stride, one tune, one fir and one resample per packet")
        _check(self._L.psk_soft_process_device_filtered(self._h, ch0, len(pkts), pkts, strides, tunes, firs, resamples, outs,
                                                        ctypes.c_void_p(stream or 0)))

    def fir_history(self, ch):
        """The filter's history of channel ch (psk_soft_fir_get_history): 254 float32, 127 (re, im) pairs, oldest first."""
        out = np.zeros(FIR_HISTORY_FLOATS, np.float32)
        _check(self._L.psk_soft_fir_get_history(self._h, int(ch), out.ctypes.data))
        return out

    def set_fir_history(self, ch, floats):
        """psk_soft_fir_set_history: replace the filter's history of channel ch."""
        x = np.ascontiguousarray(floats, np.float32)
        if x.size != FIR_HISTORY_FLOATS:
            raise ValueError("a history is 127 complex samples: 254 floats")
        _check(self._L.psk_soft_fir_set_history(self._h, int(ch), x.ctypes.data))

    def process_host(self, ch0, packets):
        """packets: list (one per channel from ch0) of None (no packet) or dict with
        data (interleaved I/Q: an int16 array is handed over as it is, FORMAT_CS16, an int8 array too, FORMAT_CS8, a float16
        array too, FORMAT_CF16, anything else as float32), xdelta,
        and optional mode / sriChanged / inputQueueFlushed.  Returns one dict per channel with the four output streams."""
        n = len(packets)
        pk = (Packet * n)()
        out = (Output * n)()
        keep = []
        bufs = []
        for i, p in enumerate(packets):
            if p is None:
                pk[i].present = 0
                bufs.append(None)
                continue
            dt = p["data"].dtype if isinstance(p["data"], np.ndarray) else None
            fmt = FORMAT_CS16 if dt == np.int16 else FORMAT_CS8 if dt == np.int8 else FORMAT_CF16 if dt == np.float16 else FORMAT_CF32
            data = np.ascontiguousarray(
                p["data"], dtype={FORMAT_CS16: np.int16, FORMAT_CS8: np.int8, FORMAT_CF16: np.float16}.get(fmt, np.float32)
            )
            keep.append(data)
            pk[i].data = data.ctypes.data
            pk[i].n_floats = data.size
            pk[i].format = fmt
            pk[i].sri_xdelta = float(p["xdelta"])
            pk[i].sri_mode = int(p.get("mode", 1))
            pk[i].sriChanged = int(bool(p.get("sriChanged", False)))
            pk[i].inputQueueFlushed = int(bool(p.get("inputQueueFlushed", False)))
            pk[i].present = 1
            cap = self.output_capacity(ch0 + i, data.size // 2)
            soft = np.empty(2 * cap, np.float32)
            bits = np.empty(3 * cap, np.int16)
            phase = np.empty(cap, np.float32)
            sidx = np.empty(cap, np.int16)
            bufs.append((soft, bits, phase, sidx))
            out[i].soft = soft.ctypes.data
            out[i].bits = bits.ctypes.data
            out[i].phase = phase.ctypes.data
            out[i].sampleIndex = sidx.ctypes.data
            out[i].cap_symbols = cap
        _check(self._L.psk_soft_process_host(self._h, ch0, n, pk, out))
        res = []
        for i in range(n):
            o = out[i]
            if bufs[i] is None:
                soft = np.zeros(0, np.float32)
                bits = np.zeros(0, np.int16)
                phase = np.zeros(0, np.float32)
                sidx = np.zeros(0, np.int16)
            else:
                soft = bufs[i][0][: 2 * o.n_symbols]
                bits = bufs[i][1][: o.n_bits]
                phase = bufs[i][2][: o.n_symbols]
                sidx = bufs[i][3][: o.n_sampleIndex]
            res.append(
                {
                    "ret": o.ret,
                    "soft": soft,
                    "bits": bits,
                    "phase": phase,
                    "index": sidx,
                    "sri_pushed": bool(o.sri_pushed),
                    "sri_soft_xdelta": o.sri_soft_xdelta,
                    "sri_bits_xdelta": o.sri_bits_xdelta,
                    "n_warn": o.n_warn,
                }
            )
        return res

    def plan_only(self, ch0, packets):
        """Control-plane results (counts, SRI) of one call without data (DEVICE_NONE handles).  packets: None or dict with
        n_floats (elements of the format), xdelta, optional mode / sriChanged / inputQueueFlushed / format."""
        n = len(packets)
        pk = (Packet * n)()
        out = (Output * n)()
        for i, p in enumerate(packets):
            if p is None:
                continue
            pk[i].n_floats = int(p["n_floats"])
            pk[i].sri_xdelta = float(p["xdelta"])
            pk[i].sri_mode = int(p.get("mode", 1))
            pk[i].sriChanged = int(bool(p.get("sriChanged", False)))
            pk[i].inputQueueFlushed = int(bool(p.get("inputQueueFlushed", False)))
            pk[i].format = int(p.get("format", FORMAT_CF32))
            pk[i].present = 1
            out[i].cap_symbols = 1 << 62
        _check(self._L.psk_soft_process_device(self._h, ch0, n, pk, out, None))
        return [
            {
                "ret": o.ret,
                "n_symbols": o.n_symbols,
                "n_bits": o.n_bits,
                "n_sampleIndex": o.n_sampleIndex,
                "sri_pushed": bool(o.sri_pushed),
                "sri_soft_xdelta": o.sri_soft_xdelta,
                "sri_bits_xdelta": o.sri_bits_xdelta,
                "n_warn": o.n_warn,
            }
            for o in out
        ]

    def synchronize(self):
        _check(self._L.psk_soft_synchronize(self._h))

    def join(self, stream=None):
        """OPT_DEFERRED_JOIN: `stream` (a raw hipStream_t; None = the handle's own) waits for the handle's side streams."""
        _check(self._L.psk_soft_join(self._h, ctypes.c_void_p(stream) if stream else None))

    def probe_read_ms(self, dev_ptr, nbytes, reps=5):
        """Mean duration (ms) of one pure 16-byte-load pass over a device buffer (empirical read ceiling)."""
        ms = ctypes.c_double()
        _check(self._L.psk_soft_probe_read_ms(self._h, ctypes.c_void_p(dev_ptr), int(nbytes), int(reps), ctypes.byref(ms)))
        return ms.value

    def stats(self):
        s = Stats()
        _check(self._L.psk_soft_get_stats(self._h, ctypes.byref(s)))
        return {k: getattr(s, k) for k, _ in Stats._fields_}

    # -- device buffers for callers without a HIP runtime of their own (tests) --------------
    def device_alloc(self, nbytes):
        p = self._L.psk_soft_device_alloc(self._h, int(nbytes))
        if not p:
            raise PskSoftError(3, self._L.psk_soft_last_error().decode("utf-8", "replace"))
        return p

    def device_free(self, p):
        self._L.psk_soft_device_free(self._h, ctypes.c_void_p(p))

    def upload(self, dev_ptr, arr):
        arr = np.ascontiguousarray(arr)
        _check(self._L.psk_soft_device_upload(self._h, ctypes.c_void_p(dev_ptr), arr.ctypes.data, arr.nbytes))

    def download(self, dev_ptr, shape, dtype):
        out = np.empty(shape, dtype)
        _check(self._L.psk_soft_device_download(self._h, out.ctypes.data, ctypes.c_void_p(dev_ptr), out.nbytes))
        return out

    def channel_stats(self, ch0=0, nch=None):
        nch = self.n_channels - ch0 if nch is None else nch
        arr = (Stats * nch)()
        _check(self._L.psk_soft_get_channel_stats(self._h, ch0, nch, arr))
        return [{k: getattr(s, k) for k, _ in Stats._fields_} for s in arr]

    def quality_records(self, ch0=0, nch=None):
        """The raw Quality records of [ch0, ch0+nch) (psk_soft_get_quality), a ctypes array."""
        nch = self.n_channels - ch0 if nch is None else nch
        arr = (Quality * nch)()
        _check(self._L.psk_soft_get_quality(self._h, ch0, nch, arr))
        return arr

    def quality(self, ch0=0, nch=None):
        """One dict per channel: the fields of its Quality record and the derived values (quality_derive)."""
        res = []
        for q in self.quality_records(ch0, nch):
            d = {k: getattr(q, k) for k in QUALITY_FIELDS}
            d.update(quality_derive(q))
            res.append(d)
        return res

    def acquire_device(self, ch0, pkts, strides, tunes, stream=None):
        """One look at a packet per channel (psk_soft_acquire_device): leaves an Acquire record per covered channel, emits
        nothing and touches no demodulator state.  pkts, strides and tunes as for process_device_tuned."""
        if strides is not None and not isinstance(strides, ctypes.Array):
            strides = (ctypes.c_uint64 * len(strides))(*[int(s) for s in strides])
        if tunes is not None and not isinstance(tunes, ctypes.Array):
            tunes = (Tune * len(tunes))(*[Tune(int(p), int(s)) for p, s in tunes])
        if (strides is not None and len(strides) != len(pkts)) or (tunes is not None and len(tunes) != len(pkts)):
            raise ValueError("one stride and one tune per packet")
        _check(self._L.psk_soft_acquire_device(self._h, ch0, len(pkts), pkts, strides, tunes, ctypes.c_void_p(stream or 0)))

    def acquire_records(self, ch0=0, nch=None):
        """The raw Acquire records of [ch0, ch0+nch) (psk_soft_get_acquire), a ctypes array."""
        nch = self.n_channels - ch0 if nch is None else nch
        arr = (Acquire * nch)()
        _check(self._L.psk_soft_get_acquire(self._h, ch0, nch, arr))
        return arr

    def acquire(self, ch0, pkts, strides=None, tunes=None, stream=None):
        """acquire_device, then one dict per covered channel: the derived values (acquire_derive) of its record."""
        self.acquire_device(ch0, pkts, strides, tunes, stream)
        return [acquire_derive(r) for r in self.acquire_records(ch0, len(pkts))]

    def symrate_device(self, ch0, pkts, strides, tunes, stream=None):
        """One look at a packet per channel (psk_soft_symrate_device): leaves a Symrate record per covered channel, emits
        nothing and touches no demodulator state.  pkts, strides and tunes as for acquire_device."""
        if strides is not None and not isinstance(strides, ctypes.Array):
            strides = (ctypes.c_uint64 * len(strides))(*[int(s) for s in strides])
        if tunes is not None and not isinstance(tunes, ctypes.Array):
            tunes = (Tune * len(tunes))(*[Tune(int(p), int(s)) for p, s in tunes])
        if (strides is not None and len(strides) != len(pkts)) or (tunes is not None and len(tunes) != len(pkts)):
            raise ValueError("one stride and one tune per packet")
        _check(self._L.psk_soft_symrate_device(self._h, ch0, len(pkts), pkts, strides, tunes, ctypes.c_void_p(stream or 0)))

    def symrate_records(self, ch0=0, nch=None):
        """The raw Symrate records of [ch0, ch0+nch) (psk_soft_get_symrate), a ctypes array."""
        nch = self.n_channels - ch0 if nch is None else nch
        arr = (Symrate * nch)()
        _check(self._L.psk_soft_get_symrate(self._h, ch0, nch, arr))
        return arr

    def symrate(self, ch0, pkts, strides=None, tunes=None, stream=None):
        """symrate_device, then one dict per covered channel: the derived values (symrate_derive) of its record."""
        self.symrate_device(ch0, pkts, strides, tunes, stream)
        return [symrate_derive(r) for r in self.symrate_records(ch0, len(pkts))]

    def sync_define(self, slot, word):
        """psk_soft_sync_define: the word (1 .. 128 points, interleaved float32 (re, im), copied) of slot `slot` (0 .. 15); a
        channel names it as SyncIn.word = slot + 1."""
        w = np.ascontiguousarray(word, np.float32)
        if w.size % 2:
            raise ValueError("a word is (re, im) pairs")
        _check(self._L.psk_soft_sync_define(self._h, int(slot), w.ctypes.data if w.size else None, w.size // 2))

    def sync_device(self, ch0, ins, stream=None):
        """The search of a known word in the soft rows of [ch0, ch0 + len(ins)) (psk_soft_sync_device): leaves a SyncRecord per
        covered channel and moves the searched channels' histories; touches no demodulator state.  ins: a ctypes SyncIn array
        or a sequence of SyncIn / (soft, n_symbols, word, flags, threshold).  The rows are DEVICE memory, complete on `stream`
        -- the soft rows of a process_device call enqueued there just before are."""
        if not isinstance(ins, ctypes.Array):
            ins = (SyncIn * len(ins))(*[_sync_in(s) for s in ins])
        _check(self._L.psk_soft_sync_device(self._h, ch0, len(ins), ins, ctypes.c_void_p(stream or 0)))

    def sync_records(self, ch0=0, nch=None):
        """The raw SyncRecord records of [ch0, ch0+nch) (psk_soft_get_sync), a ctypes array."""
        nch = self.n_channels - ch0 if nch is None else nch
        arr = (SyncRecord * nch)()
        _check(self._L.psk_soft_get_sync(self._h, ch0, nch, arr))
        return arr

    def demap_define(self, slot, points, labels):
        """psk_soft_demap_define: the map of slot `slot` (0 .. 15) -- M = 2, 4 or 8 points, interleaved float32 (re, im), and their
        M labels (a permutation of 0 .. M-1), copied; a segment names it as DemapIn.map = slot + 1."""
        p, lab = _demap_map(points, labels)
        _check(self._L.psk_soft_demap_define(self._h, int(slot), lab.size, p.ctypes.data if p.size else None,
                                             lab.ctypes.data if lab.size else None))

    def demap_device(self, ins, stream=None):
        """Segments of soft rows as per-bit LLRs (psk_soft_demap_device): writes count * B values per segment to its `out` and
        leaves a DemapRecord per segment; touches no demodulator state.  ins: a ctypes DemapIn array or a sequence of DemapIn /
        field tuples.  Rows and outputs are DEVICE memory, the rows complete on `stream` (None: the handle's)."""
        if not isinstance(ins, ctypes.Array):
            ins = (DemapIn * len(ins))(*[_demap_in(s) for s in ins])
        _check(self._L.psk_soft_demap_device(self._h, len(ins), ins, ctypes.c_void_p(stream or 0)))

    def demap_records(self, first=0, n=1):
        """The DemapRecord records of the segments [first, first + n) of the last demap_device call (psk_soft_get_demap), a ctypes
        array.  The handle does not tell how many segments that call had: a range beyond them is refused."""
        n = int(n)
        arr = (DemapRecord * n)()
        _check(self._L.psk_soft_get_demap(self._h, int(first), n, arr))
        return arr

    def viterbi_define(self, slot, K, g, P=1, keep=None):
        """psk_soft_viterbi_define: the code of slot `slot` (0 .. 15) -- constraint length K, the polynomials g, the puncture period
        P and keep mask (None: every bit kept), copied; a frame names it as ViterbiIn.code = slot + 1."""
        pol = _viterbi_polys(g)
        if keep is None:
            keep = (1 << (int(pol.size) * int(P))) - 1
        _check(self._L.psk_soft_viterbi_define(self._h, int(slot), int(K), int(pol.size), pol.ctypes.data if pol.size else None, int(P),
                                               int(keep) & 0xFFFFFFFF))

    def viterbi_device(self, ins, stream=None):
        """Frames of int8 LLRs as payload bits (psk_soft_viterbi_device): writes n_bits bytes (or ceil(n_bits / 8) with
        VITERBI_PACKED) per frame to its `out` and leaves a ViterbiRecord per frame; touches no demodulator state.  ins: a ctypes
        ViterbiIn array or a sequence of ViterbiIn / tuples in field order."""
        if not isinstance(ins, ctypes.Array):
            ins = (ViterbiIn * len(ins))(*[_viterbi_in(s) for s in ins])
        _check(self._L.psk_soft_viterbi_device(self._h, len(ins), ins, ctypes.c_void_p(stream or 0)))

    def viterbi_records(self, first=0, n=1):
        """The ViterbiRecord records of the frames [first, first + n) of the last viterbi_device call (psk_soft_get_viterbi), a
        ctypes array; waits for that call."""
        arr = (ViterbiRecord * n)()
        _check(self._L.psk_soft_get_viterbi(self._h, int(first), n, arr))
        return arr

    def rs_define(self, slot, gfpoly, fcr, prim, nroots, n=255, depth=1, mask=None):
        """psk_soft_rs_define: the Reed-Solomon code of slot `slot` (0 .. 15) -- the field polynomial, first consecutive root, the
        primitive element's power, the number of roots, the codeword length n (below 255: shortened), the interleave depth and
        the derandomiser mask (None: none), copied; a frame names it as RsIn.code = slot + 1."""
        m, mp = _rs_mask(mask)
        _check(self._L.psk_soft_rs_define(self._h, int(slot), int(gfpoly), int(fcr), int(prim), int(nroots), int(n), int(depth), mp,
                                          int(m.size)))

    def rs_device(self, ins, stream=None):
        """Frames of bytes as corrected bytes (psk_soft_rs_device): writes (n - nroots) * depth bytes (or n * depth with
        RS_WITH_PARITY) per frame to its `out` and leaves an RsRecord per frame; touches no demodulator state.  ins: a ctypes
        RsIn array or a sequence of RsIn / tuples (in, out, code[, flags])."""
        if not isinstance(ins, ctypes.Array):
            ins = (RsIn * len(ins))(*[_rs_in(s) for s in ins])
        _check(self._L.psk_soft_rs_device(self._h, len(ins), ins, ctypes.c_void_p(stream or 0)))

    def get_rs(self, first=0, n=1):
        """The RsRecord records of the frames [first, first + n) of the last rs_device call (psk_soft_get_rs), a ctypes array;
        waits for that call."""
        arr = (RsRecord * n)()
        _check(self._L.psk_soft_get_rs(self._h, int(first), n, arr))
        return arr

    def frame_word_define(self, slot, length, word, care=None):
        """psk_soft_frame_word_define: the word of slot `slot` (0 .. 15) -- its length in bits (1 .. 64), the word (its first bit in
        stream order the most significant of the `length`) and the care mask (None: every bit); a stream names it as
        FrameSearchIn.word = slot + 1."""
        if care is None:
            care = (1 << int(length)) - 1 if 1 <= int(length) <= 64 else 0
        _check(self._L.psk_soft_frame_word_define(self._h, int(slot), int(length), int(word), int(care)))

    def frame_search_device(self, ins, stream=None):
        """A known word searched in streams of packed bits (psk_soft_frame_search_device): leaves a FrameSearchRecord per stream;
        touches no demodulator state.  ins: a ctypes FrameSearchIn array or a sequence of FrameSearchIn / tuples (bits, bit0,
        n_bits, word[, max_diff[, period]])."""
        if not isinstance(ins, ctypes.Array):
            ins = (FrameSearchIn * len(ins))(*[_frame_search_in(s) for s in ins])
        _check(self._L.psk_soft_frame_search_device(self._h, len(ins), ins, ctypes.c_void_p(stream or 0)))

    def frame_search_records(self, first=0, n=1):
        """The FrameSearchRecord records of the streams [first, first + n) of the last frame_search_device call
        (psk_soft_get_frame_search), a ctypes array; waits for that call."""
        arr = (FrameSearchRecord * n)()
        _check(self._L.psk_soft_get_frame_search(self._h, int(first), n, arr))
        return arr

    def frame_format_define(self, slot, branches=1, cell=0, table=None):
        """psk_soft_frame_format_define: the format of slot `slot` (0 .. 15) -- the branches and the cell of the convolutional byte
        deinterleaver (1 or 0: none) and the 256-byte table every byte goes through (None: the identity), copied; a frame names
        it as FrameCutIn.format = slot + 1."""
        t, tp = _frame_table(table)
        _check(self._L.psk_soft_frame_format_define(self._h, int(slot), int(branches), int(cell), tp))

    def frame_cut_device(self, ins, stream=None):
        """Byte frames cut from streams of packed bits (psk_soft_frame_cut_device): writes n_bytes bytes per frame to its `out` and
        leaves a FrameCutRecord per frame; touches no demodulator state.  ins: a ctypes FrameCutIn array or a sequence of
        FrameCutIn / tuples (bits, bit, out, n_bytes[, format[, branch0[, flags]]])."""
        if not isinstance(ins, ctypes.Array):
            ins = (FrameCutIn * len(ins))(*[_frame_cut_in(s) for s in ins])
        _check(self._L.psk_soft_frame_cut_device(self._h, len(ins), ins, ctypes.c_void_p(stream or 0)))

    def frame_cut_records(self, first=0, n=1):
        """The FrameCutRecord records of the frames [first, first + n) of the last frame_cut_device call (psk_soft_get_frame_cut),
        a ctypes array; waits for that call."""
        arr = (FrameCutRecord * n)()
        _check(self._L.psk_soft_get_frame_cut(self._h, int(first), n, arr))
        return arr

    def sync_history(self, ch):
        """The sync history of channel ch (psk_soft_sync_get_history): 254 float32, 127 (re, im) pairs, oldest first."""
        out = np.zeros(SYNC_HISTORY_FLOATS, np.float32)
        _check(self._L.psk_soft_sync_get_history(self._h, int(ch), out.ctypes.data))
        return out

    def set_sync_history(self, ch, floats):
        """psk_soft_sync_set_history: replace the sync history of channel ch."""
        x = np.ascontiguousarray(floats, np.float32)
        if x.size != SYNC_HISTORY_FLOATS:
            raise ValueError("a history is 127 complex symbols: 254 floats")
        _check(self._L.psk_soft_sync_set_history(self._h, int(ch), x.ctypes.data))

    def export_state(self, ch):
        n = int(self._L.psk_soft_state_bytes(self._h))
        buf = (ctypes.c_uint8 * n)()
        _check(self._L.psk_soft_export_state(self._h, ch, buf, n))
        return bytes(buf)

    def import_state(self, ch, blob):
        buf = (ctypes.c_uint8 * len(blob)).from_buffer_copy(blob)
        _check(self._L.psk_soft_import_state(self._h, ch, buf, len(blob)))
