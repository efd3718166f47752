"""ctypes binding of the C ABI in include/dusp_hip.h (dusp_amd/libdusp_hip.so).

There is deliberately no CPU fallback here: if the HIP library is missing or no
GPU is usable, every entry point raises.
"""
import ctypes
import operator
import threading
import os

import numpy as np

from .mix import check_limiter, check_limiter_release, LIMITER_RELEASE_MAX, LIMITER_RELEASE_SAMPLES, check_loudness, check_meters, check_stems, check_true_peak, meter_blocks, meter_hop, METER_RATE_LOW, METER_RATE_MIN, LIMITER_THRESHOLD_BAD, LIMITER_WINDOW_MAX, LIMITER_WINDOW_SAMPLES, BUSES_WITHOUT_SENDS, SENDS_WITHOUT_BUSES, TRACKS_FADERS_SHAPE, TRACKS_SENDS_SHAPE, check_tracks, SPACE_ALONE, STEREO_NO_PLACES, Placement, check_sends, refuse_sends_placement, _gains_table, _whole, check_stereo_kinds, frac_arrays, pan_arrays, pan_comp, stereo_pan_arrays, tap_arrays  # noqa: F401
from .wavetables import N_TABLES, make_table

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DUSP_HIP_LIB") or os.path.join(_HERE, "libdusp_hip.so")  # (DUSP_HIP_LIB: another build of the library, for A/B runs)

ENGINE_AUTO, ENGINE_CHUNK, ENGINE_FUSED, ENGINE_WAVE, ENGINE_LOOP = 0, 1, 2, 3, 4
ENGINE_RESUMABLE = 0x100  # OR into the engine: the program will be continued (Program.continue_with)
ENGINE_NAMES = {ENGINE_CHUNK: "chunk", ENGINE_FUSED: "fused", ENGINE_WAVE: "wave"}  # (ENGINE_LOOP: accepted by the library, means AUTO since ABI v7)

EXPORTS = [
    "dusp_version", "dusp_abi_version", "dusp_last_error", "dusp_ctx_create", "dusp_ctx_destroy",
    "dusp_table_upload", "dusp_program_build", "dusp_program_destroy", "dusp_program_continue", "dusp_program_info_get",
    "dusp_render_device", "dusp_render_host", "dusp_render_host_interleaved", "dusp_interleave_device", "dusp_state_download",
    "dusp_last_kernel_ms", "dusp_fill_device", "dusp_render_device_inputs", "dusp_render_host_inputs",
    "dusp_host_alloc", "dusp_host_free", "dusp_circuit_kernel_source", "dusp_jit_cache_dir", "dusp_render_chain_window", "dusp_device_count",
    "dusp_peak_device", "dusp_encode_device", "dusp_render_host_pcm", "dusp_mix_device", "dusp_render_host_mix",
    "dusp_score_device", "dusp_render_host_score", "dusp_score_last_ms",
    "dusp_score_rows_device", "dusp_render_host_score_parts", "dusp_descriptor_channels",
    "dusp_score_rows_pan_device", "dusp_render_host_score_parts_pan",
    "dusp_score_rows_frac_device", "dusp_render_host_score_parts_frac",
    "dusp_score_rows_space_device", "dusp_render_host_score_parts_space",
    "dusp_score_rows_stereo_device", "dusp_render_host_score_parts_stereo",
    "dusp_render_host_score_piece",
    "dusp_render_host_score_piece_buses", "dusp_score_rows_send_device", "dusp_score_return_device",
    "dusp_render_host_score_piece_tracks", "dusp_score_tracks_mix_device",
    "dusp_render_host_score_piece_stems", "dusp_score_stems_mix_device", "dusp_score_stems_return_device", "dusp_peak_common_device",
    "dusp_meter_blocks", "dusp_meter_device", "dusp_meter_last_ms", "dusp_meter_host", "dusp_render_host_score_piece_meters",
    "dusp_true_peak_taps", "dusp_true_peak_tile", "dusp_true_peak_device", "dusp_true_peak_host", "dusp_render_host_score_piece_loudness",
    "dusp_limiter_threshold", "dusp_limit_tile", "dusp_limit_device", "dusp_limit_last_ms", "dusp_limit_host", "dusp_render_host_score_piece_limiter",
    "dusp_limit_release_tile", "dusp_limit_release_device", "dusp_limit_release_last_ms", "dusp_limit_release_host", "dusp_render_host_score_piece_limiter_release",
]

PCM_S16, PCM_S24, PCM_F32 = 1, 2, 3  # dusp_pcm_format
PCM_FORMATS = {"s16": PCM_S16, "s24": PCM_S24, "f32": PCM_F32}
PCM_BYTES = {PCM_S16: 2, PCM_S24: 3, PCM_F32: 4}
NORMALISE_NONE, NORMALISE_CLIP, NORMALISE_FULL = 0, 1, 2  # dusp_normalise
# dusp_render_chain_window: windows start on whole blocks of 2048 samples up to sample 2^40 and hold at most 65535 blocks
CHAIN_BLOCK, CHAIN_FIRST_MAX, CHAIN_SAMPLES_MAX = 2048, 1 << 40, 65535 * 2048


class DuspHipError(RuntimeError):
    def __init__(self, status, message):
        super().__init__("%s (status %d)" % (message, status))
        self.status = status
        self.message = message


class ProgramInfo(ctypes.Structure):
    _fields_ = [("sample_rate", ctypes.c_uint32), ("chunk_size", ctypes.c_uint32), ("n_units", ctypes.c_uint32),
                ("n_out_channels", ctypes.c_uint32), ("n_params", ctypes.c_uint32), ("engine", ctypes.c_uint32),
                ("n_device_ops", ctypes.c_uint32), ("n_inputs", ctypes.c_uint32), ("shape", ctypes.c_char * 64)]


_lib = None


def load():
    """Load libdusp_hip.so (built by dusp_amd/csrc/Makefile).  Raises if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise DuspHipError(-3, "HIP extension %s is missing: build it with `make -C dusp_amd/csrc` "
                               "(there is no CPU fallback)" % LIB_PATH)
    try:
        # PyTorch-ROCm ships its own libamdhip64; whichever HIP runtime initialises first owns the GPU
        # in this process, so let torch's copy load first and have this library bind to the same one.
        import torch  # noqa: F401
    except ImportError:
        pass
    L = ctypes.CDLL(LIB_PATH)
    vp, sz, ci = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
    L.dusp_version.restype = ctypes.c_char_p
    L.dusp_abi_version.restype = ci
    L.dusp_device_count.restype = ci
    L.dusp_last_error.restype = ctypes.c_char_p
    L.dusp_last_error.argtypes = [vp]
    L.dusp_ctx_create.argtypes = [ci, ctypes.POINTER(vp)]
    L.dusp_ctx_destroy.argtypes = [vp]
    L.dusp_ctx_destroy.restype = None
    L.dusp_table_upload.argtypes = [vp, ci, vp, sz]
    L.dusp_program_build.argtypes = [vp, vp, sz, ci, ctypes.POINTER(vp)]
    L.dusp_program_destroy.argtypes = [vp]
    L.dusp_program_destroy.restype = None
    L.dusp_program_continue.argtypes = [vp, vp, sz]
    L.dusp_program_info_get.argtypes = [vp, ctypes.POINTER(ProgramInfo)]
    L.dusp_render_device.argtypes = [vp, sz, sz, vp, vp, vp]
    L.dusp_render_host.argtypes = [vp, sz, sz, vp, vp]
    L.dusp_render_host_interleaved.argtypes = [vp, sz, sz, vp, vp]
    L.dusp_interleave_device.argtypes = [vp, vp, sz, sz, sz, vp, vp]
    L.dusp_peak_device.argtypes = [vp, vp, sz, sz, sz, vp, vp]
    L.dusp_encode_device.argtypes = [vp, vp, sz, sz, sz, ci, ci, vp, vp, vp]
    L.dusp_render_host_pcm.argtypes = [vp, sz, sz, vp, vp, ci, ci, vp, vp]
    L.dusp_mix_device.argtypes = [vp, vp, sz, sz, sz, vp, vp, ci, vp, vp]
    L.dusp_render_host_mix.argtypes = [vp, sz, sz, vp, vp, sz, ci, ci, vp, vp]
    L.dusp_score_device.argtypes = [vp, vp, sz, sz, sz, vp, vp, vp, sz, vp, ci, vp, vp]
    L.dusp_score_last_ms.argtypes = [vp, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float)]
    L.dusp_render_host_score.argtypes = [vp, sz, sz, sz, vp, vp, vp, vp, sz, ci, ci, vp, vp]
    L.dusp_score_rows_device.argtypes = [vp, vp, vp, sz, sz, vp, vp, vp, sz, vp, ci, vp, vp]
    L.dusp_render_host_score_parts.argtypes = [vp, sz, sz, vp, vp, vp, vp, sz, sz, ci, ci, vp, vp]
    L.dusp_descriptor_channels.argtypes = [vp, sz]
    L.dusp_score_rows_pan_device.argtypes = [vp, vp, vp, sz, vp, vp, vp, vp, vp, sz, vp, ci, vp, vp]
    L.dusp_render_host_score_parts_pan.argtypes = [vp, sz, sz, vp, vp, vp, vp, vp, vp, sz, sz, ci, ci, vp, vp]
    L.dusp_score_rows_frac_device.argtypes = [vp, vp, vp, sz, sz, vp, vp, vp, vp, vp, vp, sz, vp, ci, vp, vp]
    L.dusp_render_host_score_parts_frac.argtypes = [vp, sz, sz, vp, vp, vp, vp, vp, vp, vp, sz, sz, ci, ci, vp, vp]
    L.dusp_score_rows_space_device.argtypes = [vp, vp, vp, sz, sz, vp, vp, vp, vp, vp, sz, vp, ci, vp, vp]
    L.dusp_render_host_score_parts_space.argtypes = [vp, sz, sz, vp, vp, vp, vp, sz, vp, vp, sz, sz, ci, ci, vp, vp]
    L.dusp_score_rows_stereo_device.argtypes = [vp, vp, vp, vp, sz, vp, vp, vp, vp, vp, vp, sz, vp, ci, vp, vp]
    L.dusp_render_host_score_parts_stereo.argtypes = [vp, sz, sz, vp, vp, vp, vp, vp, vp, vp, sz, sz, ci, ci, vp, vp]
    L.dusp_render_host_score_piece.argtypes = [vp, sz, sz, vp, vp, vp, vp, vp, vp, sz, sz, ci, ci, vp, vp]
    L.dusp_render_host_score_piece_buses.argtypes = [vp, sz, sz, vp, vp, vp, vp, vp, vp, vp, sz, sz, ci, ci, vp, vp]
    L.dusp_score_rows_send_device.argtypes = [vp, vp, vp, sz, sz, vp, vp, vp, vp, vp, sz, vp, sz, vp, ci, vp, vp, vp, vp]
    L.dusp_score_return_device.argtypes = [vp, vp, vp, sz, sz, ci, vp, vp]
    if hasattr(L, "dusp_render_host_score_piece_tracks"):  # (detected by symbol: DUSP_HIP_LIB may name a build from before tracks, for A/B runs)
        L.dusp_render_host_score_piece_tracks.argtypes = [vp, sz, sz, vp, vp, vp, vp, vp, vp, vp, vp, sz, sz, ci, ci, vp, vp]
        L.dusp_score_tracks_mix_device.argtypes = [vp, vp, vp, sz, vp, sz, vp, sz, ci, vp, vp, vp, vp]
    if hasattr(L, "dusp_render_host_score_piece_stems"):  # (detected by symbol, as the tracks are)
        L.dusp_render_host_score_piece_stems.argtypes = [vp, sz, sz, vp, vp, vp, vp, vp, vp, vp, vp, vp, sz, sz, ci, ci, vp, vp]
        L.dusp_score_stems_mix_device.argtypes = [vp, vp, vp, sz, vp, sz, vp, sz, ci, vp, vp, vp, vp, vp]
        L.dusp_score_stems_return_device.argtypes = [vp, vp, vp, sz, sz, ci, vp, vp, vp, vp]
        L.dusp_peak_common_device.argtypes = [vp, vp, sz, vp, vp]
    if hasattr(L, "dusp_render_host_score_piece_meters"):  # (detected by symbol, as the stems are)
        L.dusp_meter_blocks.argtypes, L.dusp_meter_blocks.restype = [sz, ctypes.c_uint32], sz
        L.dusp_meter_device.argtypes = [vp, vp, sz, sz, sz, ctypes.c_uint32, vp, vp, vp]
        L.dusp_meter_last_ms.argtypes = [vp, vp]
        L.dusp_meter_host.argtypes = [vp, vp, sz, sz, sz, ctypes.c_uint32, vp, vp, vp]
        L.dusp_render_host_score_piece_meters.argtypes = [vp, sz, sz, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, sz, sz, ci, ci, vp, vp]
    if hasattr(L, "dusp_render_host_score_piece_loudness"):  # (detected by symbol, as the meters are)
        L.dusp_true_peak_taps.argtypes = [ctypes.c_uint32, ctypes.POINTER(ci), ctypes.POINTER(ctypes.c_double)]
        L.dusp_true_peak_tile.argtypes, L.dusp_true_peak_tile.restype = [vp, sz, sz, sz, ctypes.c_uint32], sz
        L.dusp_true_peak_device.argtypes = [vp, vp, sz, sz, sz, ctypes.c_uint32, vp, vp]
        L.dusp_true_peak_host.argtypes = [vp, vp, sz, sz, sz, ctypes.c_uint32, vp]
        L.dusp_render_host_score_piece_loudness.argtypes = [vp, sz, sz, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, sz, sz, ci, ci, vp, vp]
    if hasattr(L, "dusp_render_host_score_piece_limiter"):  # (detected by symbol, as the loudness delivery is)
        L.dusp_limiter_threshold.argtypes, L.dusp_limiter_threshold.restype = [ctypes.c_double] * 3, ctypes.c_double
        L.dusp_limit_tile.argtypes, L.dusp_limit_tile.restype = [vp, sz, sz], sz
        L.dusp_limit_device.argtypes = [vp, vp, sz, sz, sz, ctypes.c_uint32, ctypes.c_double, sz, vp, vp, vp, vp]
        L.dusp_limit_last_ms.argtypes = [vp, vp]
        L.dusp_limit_host.argtypes = [vp, vp, sz, sz, sz, ctypes.c_uint32, ctypes.c_double, sz, vp, vp, vp]
        L.dusp_render_host_score_piece_limiter.argtypes = [vp, sz, sz, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, sz, sz, ci, ci, vp, vp]
    if hasattr(L, "dusp_render_host_score_piece_limiter_release"):  # (... and the limiter's release)
        L.dusp_limit_release_tile.argtypes, L.dusp_limit_release_tile.restype = [vp, sz, sz, sz], sz
        L.dusp_limit_release_device.argtypes = [vp, vp, sz, sz, sz, ctypes.c_uint32, ctypes.c_double, sz, sz, vp, vp, vp, vp, vp]
        L.dusp_limit_release_last_ms.argtypes = [vp, vp]
        L.dusp_limit_release_host.argtypes = [vp, vp, sz, sz, sz, ctypes.c_uint32, ctypes.c_double, sz, sz, vp, vp, vp]
        L.dusp_render_host_score_piece_limiter_release.argtypes = L.dusp_render_host_score_piece_limiter.argtypes
    L.dusp_state_download.argtypes = [vp, sz, sz, vp, sz]
    L.dusp_last_kernel_ms.argtypes = [vp, ctypes.POINTER(ctypes.c_float)]
    L.dusp_fill_device.argtypes = [vp, vp, sz, ctypes.c_float, vp]
    L.dusp_render_device_inputs.argtypes = [vp, sz, sz, vp, vp, vp, vp]
    L.dusp_render_chain_window.argtypes = [vp, ctypes.c_uint64, sz, vp, ci, vp, vp]
    L.dusp_render_host_inputs.argtypes = [vp, sz, sz, vp, vp, vp, ci]
    L.dusp_host_alloc.argtypes = [vp, sz, ctypes.POINTER(vp)]
    L.dusp_host_free.argtypes = [vp, vp]
    L.dusp_jit_cache_dir.restype = ctypes.c_char_p
    L.dusp_jit_cache_dir.argtypes = []
    L.dusp_circuit_kernel_source.argtypes = [vp, sz, ci, ci, ci, ci, ctypes.c_char_p, sz]
    _lib = L
    return L


class ScorePart(ctypes.Structure):
    """dusp_score_part: one instrument of a piece (dusp_render_host_score_parts)"""
    _fields_ = [("prog", ctypes.c_void_p), ("n_instances", ctypes.c_size_t), ("n_voice_samples", ctypes.c_size_t), ("h_params", ctypes.c_void_p)]


PLACE_ROWS, PLACE_PAN, PLACE_SPACE, PLACE_STEREO = 0, 1, 2, 3  # dusp_score_place_kind
PLACE_KINDS = {"rows": PLACE_ROWS, "pan": PLACE_PAN, "space": PLACE_SPACE, "stereo": PLACE_STEREO}


class ScorePlacement(ctypes.Structure):
    """dusp_score_placement: how the voices of a piece are placed, as one record (dusp_render_host_score_piece)"""
    _fields_ = [("kind", ctypes.c_int), ("h_fracs", ctypes.c_void_p), ("h_pans", ctypes.c_void_p), ("h_comp", ctypes.c_void_p), ("n_speakers", ctypes.c_size_t),
                ("h_delays", ctypes.c_void_p), ("h_tap_gains", ctypes.c_void_p)]


class ScoreMaster(ctypes.Structure):
    """dusp_score_master: the mono circuit a piece's mix goes through, and its parameter table [n_params][timeline channels]"""
    _fields_ = [("prog", ctypes.c_void_p), ("h_params", ctypes.c_void_p)]


class ScoreBuses(ctypes.Structure):
    """dusp_score_buses: the bus circuits of a piece, each given as a master is, and the voices' send levels f32 [n_buses][n_voices]"""
    _fields_ = [("n_buses", ctypes.c_size_t), ("buses", ctypes.c_void_p), ("h_sends", ctypes.c_void_p)]


class ScoreTrackProgram(ctypes.Structure):
    """dusp_score_track_program: the one program of tracks with isomorphic circuits, the tracks it serves, and its parameter table
    [n_params][tracks x timeline channels]"""
    _fields_ = [("prog", ctypes.c_void_p), ("n_tracks", ctypes.c_size_t), ("h_tracks", ctypes.c_void_p), ("h_params", ctypes.c_void_p)]


class ScoreTracks(ctypes.Structure):
    """dusp_score_tracks: where every voice of a piece goes (int32 [n_voices], -1: straight to the mix), the track programs, the faders
    f32 [n_tracks] and the tracks' levels into the buses f32 [n_buses][n_tracks]"""
    _fields_ = [("n_tracks", ctypes.c_size_t), ("h_track_of", ctypes.c_void_p), ("n_programs", ctypes.c_size_t), ("programs", ctypes.c_void_p),
                ("h_faders", ctypes.c_void_p), ("h_track_sends", ctypes.c_void_p)]


class ScoreStems(ctypes.Structure):
    """dusp_score_stems: how many signals the caller has sized h_out and h_peaks for, 1 + tracks + buses + 1"""
    _fields_ = [("n_signals", ctypes.c_size_t)]


class ScoreMeters(ctypes.Structure):
    """dusp_score_meters: how many signals and blocks the caller has sized the three arrays for, and the arrays"""
    _fields_ = [("n_signals", ctypes.c_size_t), ("n_blocks", ctypes.c_size_t), ("h_rms", ctypes.c_void_p), ("h_lufs", ctypes.c_void_p), ("h_momentary", ctypes.c_void_p)]


class ScoreLoudness(ctypes.Structure):
    """dusp_score_loudness: whether the call encodes at a loudness target, the target and the true-peak ceiling, and where the true peaks
    [signals][channels], the gain and the level go"""
    _fields_ = [("deliver", ctypes.c_int), ("target_lufs", ctypes.c_double), ("ceiling_dbtp", ctypes.c_double), ("h_true_peak", ctypes.c_void_p), ("h_gain", ctypes.c_void_p),
                ("h_level", ctypes.c_void_p)]


class ScoreLimiter(ctypes.Structure):
    """dusp_score_limiter: the limiter's window in samples, and where what it did goes: whether it ran, its threshold, min(g), and the
    mix's loudness and the largest true peak in front of it"""
    _fields_ = [("window_samples", ctypes.c_size_t), ("h_engaged", ctypes.c_void_p), ("h_threshold", ctypes.c_void_p), ("h_reduction", ctypes.c_void_p),
                ("h_lufs_in", ctypes.c_void_p), ("h_true_peak_in", ctypes.c_void_p)]


class ScoreLimiterRelease(ctypes.Structure):
    """dusp_score_limiter_release: the limiter's record, and its release in samples (0: none of its own)"""
    _fields_ = [("limiter", ScoreLimiter), ("release_samples", ctypes.c_size_t)]


PINNED_MIN_BYTES = 1 << 20  # results of at least 1 MiB are delivered in pinned memory (dusp_host_alloc): one DMA, no staging
# Page-locked memory is a machine-wide resource: results a caller keeps alive stay pinned, so beyond this many bytes in use per
# context new results are ordinary (pageable) numpy arrays again (the staged download).  `render(..., pinned=False)` opts out per call.
PINNED_MAX_LIVE_BYTES = 8 << 30


class _PinnedBlock:
    """Owner of one dusp_host_alloc buffer: handed back to the context's pool when the last array over it goes."""

    def __init__(self, ctx, ptr, nbytes):
        self.ctx, self.ptr, self.nbytes = ctx, ptr, nbytes

    def __del__(self):  # (whatever thread the garbage collector runs on: _host_release takes the context's lock)
        try:
            self.ctx._host_release(self.ptr, self.nbytes)
        except Exception:
            pass


def circuit_kernel_source(words, waves=16, per_wave=1, lds_table=True, compile=False, continued=False, lean_recurrence=False):
    """HIP text of the kernel the circuit compiler generates for a descriptor (dusp_circuit_kernel_source; needs no GPU).
    Raises DuspHipError(-2) for circuits that stay on the interpreter."""
    L = load()
    words = np.ascontiguousarray(words, dtype=np.float64)
    buf = ctypes.create_string_buffer(1 << 20)
    n = L.dusp_circuit_kernel_source(words.ctypes.data, words.size, waves, per_wave, int(bool(lds_table)) | (2 if continued else 0) | (4 if lean_recurrence else 0), int(compile), buf, len(buf))
    if n < 0:
        raise DuspHipError(n, L.dusp_last_error(None).decode())
    return buf.value.decode()


def descriptor_channels(words):
    """How many output channels the circuit of a descriptor has (dusp_descriptor_channels: host code only, needs no GPU)."""
    L = load()
    words = np.ascontiguousarray(words, dtype=np.float64)
    n = L.dusp_descriptor_channels(words.ctypes.data, words.size)
    if n < 0:
        raise DuspHipError(n, L.dusp_last_error(None).decode())
    return n


def _pcm_format(format):
    """"s16" | "s24" | "f32" (or the DUSP_PCM_* number) -> DUSP_PCM_*"""
    if isinstance(format, str):
        if format not in PCM_FORMATS:
            raise ValueError('dusp-hip: format must be "s16", "s24" or "f32", not %r' % (format,))
        return PCM_FORMATS[format]
    return int(format)


def _whole_samples(values, n, name):
    """onsets / lengths of a score -> contiguous int64 [n]: in samples, whole numbers (a fraction is refused)"""
    return _whole(values, n, name, "n_instances", "dusp-hip: %s are in samples, whole numbers: a fraction (or what is no number) is refused")


def _score_rows(rows, row_samples, onsets, lengths):
    """what the score_rows_* entries take alike -> (pointers uint64 [n], samples uint32 [n], onsets int64 [n], lengths int64 [n] or None)"""
    n = len(rows)
    samples = np.asarray(row_samples) if n else np.zeros(0, dtype=np.uint32)
    if samples.shape != (n,) or samples.dtype.kind not in "iu" or np.any(samples < 0) or np.any(samples > 0xffffffff):
        raise ValueError("dusp-hip: row_samples must be whole numbers 0 .. 2^32 - 1 of shape (voices=%d,)" % n)
    samples = np.ascontiguousarray(samples, dtype=np.uint32)
    pointers = np.array([int(r or 0) for r in rows], dtype=np.uint64)
    onsets = _whole_samples(onsets, n, "onsets")
    if lengths is not None:
        lengths = _whole_samples(lengths, n, "lengths")
    return pointers, samples, onsets, lengths


def _ptr(a, some=True):
    """the address of a host array for the library: NULL for None, and where the caller has nothing to be read (a call without voices)"""
    return a.ctypes.data if a is not None and some else None


def _pcm_out(ctx, format, normalise, frames, pinned, batch=None):
    """What a delivering call hands the library -> (DUSP_PCM_* or 0, normalise, the array for the result, the array for the peaks or
    None).  frames: (samples, channels) of one render; batch: so many of them (Program.render_pcm), each with a peak of its own.
    format None, for one render: planar float32 [channels, samples], nothing normalised and no peak.  Else format and normalise
    are checked, and the frames are int16, uint8 (.., 3) or float32."""
    if format is None and batch is None:
        return 0, 0, ctx.host_empty(frames[::-1], pinned), None
    fmt = _pcm_format(format)
    if fmt not in PCM_BYTES:
        raise ValueError('dusp-hip: format must be "s16", "s24" or "f32", not %r' % (format,))
    if normalise not in (NORMALISE_NONE, NORMALISE_CLIP, NORMALISE_FULL):
        raise ValueError("dusp-hip: normalise must be 0 (none), 1 (shrink only what clips) or 2 (to full scale), not %r" % (normalise,))
    if batch is not None:
        frames = (batch,) + frames
    out = ctx.host_empty_bytes(frames + (3,) if fmt == PCM_S24 else frames, {PCM_S16: np.int16, PCM_S24: np.uint8, PCM_F32: np.float32}[fmt], pinned)
    return fmt, int(normalise), out, np.empty(1 if batch is None else batch, dtype=np.float32)


class Context:
    """One HIP device + stream + the uploaded wave tables."""

    def __init__(self, device=-1, sample_rate=None):
        self._L = load()
        h = ctypes.c_void_p()
        rc = self._L.dusp_ctx_create(device, ctypes.byref(h))
        if rc != 0:
            raise DuspHipError(rc, self._L.dusp_last_error(None).decode())
        self._h = h
        self._host_live = 0       # pinned result buffers some numpy array still looks at
        self._host_live_bytes = 0
        # pool calls may come from a finalizer on another thread — or on THIS one: the cyclic collector can run while the lock is held
        # (allocating Python objects inside host_empty) and collect a cycle that owns a pinned block, whose __del__ takes the lock again.
        # dusp_host_alloc / _free take only the library's own pool mutex, which no Python code runs under, so re-entry is safe.
        self._host_lock = threading.RLock()
        self._close_pending = False
        self.sample_rate = None
        if sample_rate is not None:
            self.upload_tables(sample_rate)

    def host_empty(self, shape, pinned=None):
        """float32 array for a render result (replaces `new TypedArray(lengthInSamples)`, renderChannelData.js:39).  Large
        results live in the context's pinned pool so that the download is a direct DMA; the block returns to the pool when
        the array (and every view of it) has been collected."""
        return self.host_empty_bytes(shape, np.float32, pinned)

    def host_empty_bytes(self, shape, dtype, pinned=None):
        """host_empty for any sample type (int16 / uint8 frames of render_pcm): sized in bytes, same pool, same rules."""
        dtype = np.dtype(dtype)
        nbytes = int(np.prod(shape)) * dtype.itemsize
        if pinned is None:
            with self._host_lock:
                pinned = nbytes >= PINNED_MIN_BYTES and self._host_live_bytes + nbytes <= PINNED_MAX_LIVE_BYTES
        if not pinned or nbytes == 0:
            return np.empty(shape, dtype=dtype)
        p = ctypes.c_void_p()
        with self._host_lock:
            self._check(self._L.dusp_host_alloc(self._h, nbytes, ctypes.byref(p)))
            self._host_live += 1
            self._host_live_bytes += nbytes
        buf = (ctypes.c_ubyte * nbytes).from_address(p.value)
        buf._dusp_owner = _PinnedBlock(self, p.value, nbytes)
        return np.frombuffer(buf, dtype=dtype).reshape(shape)

    def _host_release(self, ptr, nbytes=0):
        with self._host_lock:
            self._host_live -= 1
            self._host_live_bytes -= nbytes
            close_now = False
            if self._h:
                self._L.dusp_host_free(self._h, ptr)
                close_now = self._close_pending and self._host_live == 0
        if close_now:
            self.close()

    def _check(self, rc):
        if rc < 0:
            raise DuspHipError(rc, self._L.dusp_last_error(self._h).decode())
        return rc

    def upload_tables(self, sample_rate, tables=None):
        """Compute (or take) the wave tables (ids 0-4) and Shape tables (ids 5-8) for this sample rate and hand
        them to the device."""
        for tid in range(N_TABLES):
            t = tables[tid] if tables is not None else make_table(tid, sample_rate)  # (every table is defined at every rate, as in the reference)
            t = np.ascontiguousarray(t, dtype=np.float32)
            self._check(self._L.dusp_table_upload(self._h, tid, t.ctypes.data, t.size))
        self.sample_rate = sample_rate

    def build(self, words, engine=ENGINE_AUTO):
        return Program(self, words, engine)

    def interleave(self, d_planar, n_instances, n_channels, n_samples, d_out, stream=None):
        """Device pointers: planar f32 [instance][channel][sample] -> frames f32 [instance][sample][channel]."""
        self._check(self._L.dusp_interleave_device(self._h, d_planar, n_instances, n_channels, n_samples, d_out, stream))

    def peak(self, d_planar, n_instances, n_channels, n_samples, d_peaks, stream=None):
        """Device pointers: planar f32 [instance][channel][sample] -> f32 [instance], each instance's exact max |x| (NaN if it holds one)."""
        self._check(self._L.dusp_peak_device(self._h, d_planar, n_instances, n_channels, n_samples, d_peaks, stream))

    def encode(self, d_planar, n_instances, n_channels, n_samples, d_out, format="s16", normalise=NORMALISE_NONE, d_peaks=None, stream=None):
        """Device pointers: planar f32 -> interleaved s16 / packed s24 / f32 frames [instance][sample][channel], each instance scaled by the
        gain its peak (d_peaks, from Context.peak) gives under `normalise` (include/dusp_hip.h: the sample contract)."""
        self._check(self._L.dusp_encode_device(self._h, d_planar, n_instances, n_channels, n_samples, _pcm_format(format), int(normalise), d_peaks, d_out, stream))

    def mix(self, d_planar, n_instances, n_channels, n_samples, d_out, d_gains=None, d_init=None, raw=False, stream=None):
        """Device pointers: planar f32 [instance][channel][sample] -> f32 [channel][sample], the instances' mix in Sum.many's chain order
        (dusp_mix_device; dusp_amd/mix.py mix_chain is the contract): one f32 rounding per add, in index order, each instance first scaled by
        its f32 gain (d_gains), the chain continued from d_init (which may be d_out); raw: a partial sum, NaN and -0 kept."""
        self._check(self._L.dusp_mix_device(self._h, d_planar, n_instances, n_channels, n_samples, d_gains, d_init, int(bool(raw)), d_out, stream))

    def score_device(self, d_planar, n_instances, n_channels, n_voice_samples, onsets, n_total_samples, d_out, lengths=None, d_gains=None, d_init=None,
                     raw=False, stream=None):
        """Device pointers: planar f32 [instance][channel][voice sample] -> f32 [channel][timeline sample], the instances mixed in Sum.many's
        chain order with instance k at timeline sample onsets[k] (dusp_score_device; dusp_amd/mix.py score_chain is the contract).  onsets
        and lengths are HOST arrays of whole numbers of samples (any sign; lengths in 0 .. n_voice_samples, None: whole voices): the
        launch's plan is made on the host.  d_gains, d_init (which may be d_out) and raw as for mix()."""
        onsets = _whole_samples(onsets, n_instances, "onsets")
        if lengths is not None:
            lengths = _whole_samples(lengths, n_instances, "lengths")
        self._check(self._L.dusp_score_device(self._h, d_planar, n_instances, n_channels, n_voice_samples, _ptr(onsets, n_instances), _ptr(lengths), d_gains,
                                              n_total_samples, d_init, int(bool(raw)), d_out, stream))

    def score_rows_device(self, rows, row_samples, n_channels, onsets, n_total_samples, d_out, lengths=None, d_gains=None, d_init=None, raw=False, stream=None):
        """score_device over voices that each lie in a buffer of their own (dusp_score_rows_device; dusp_amd/mix.py score_chain_rows is the
        contract): rows are the voices' DEVICE pointers (ints; None or 0 for a voice of no samples), voice k planar f32
        [n_channels][row_samples[k]].  onsets and lengths are HOST arrays of whole numbers of samples, lengths in 0 .. row_samples[k].
        Everything else as score_device; score_last_ms() reports the call."""
        self._score_rows_call(rows, row_samples, onsets, lengths, lambda n: (), lambda n, rows, samples, onsets, lengths: self._L.dusp_score_rows_device(
            self._h, rows, samples, n, n_channels, onsets, lengths, d_gains, n_total_samples, d_init, int(bool(raw)), d_out, stream))

    def _score_rows_call(self, rows, row_samples, onsets, lengths, placed, call):
        """What the score_rows_* methods do alike: the rows' arrays, checked (_score_rows); what places the voices, checked — placed(n) ->
        host arrays, alive across the call; and the library's entry, call(n, rows, samples, onsets, lengths as addresses, *those arrays)."""
        n = len(rows)
        pointers, samples, onsets, lengths = _score_rows(rows, row_samples, onsets, lengths)
        arrays = placed(n)
        self._check(call(n, _ptr(pointers, n), _ptr(samples, n), _ptr(onsets, n), _ptr(lengths), *arrays))

    def score_rows_pan(self, rows, row_samples, onsets, pans, n_total_samples, d_out, lengths=None, d_gains=None, d_init=None, raw=False, comp=None, stream=None):
        """score_rows_device over MONO rows, voice k panned to pans[k] where it is added to a timeline of TWO channels
        (dusp_score_rows_pan_device; dusp_amd/mix.py score_chain_rows_panned is the contract): rows are the voices' DEVICE pointers, voice
        k f32 [row_samples[k]]; pans a HOST array of finite f32, not clamped; comp the f64 compensation per voice (None: math.pow's, the
        reference's formula); d_init (which may be d_out) and d_out f32 [2][n_total_samples].  score_last_ms() reports the call."""
        self._score_rows_call(rows, row_samples, onsets, lengths, lambda n: pan_arrays(pans, n, comp), lambda n, rows, samples, onsets, lengths, pans, comp: self._L.dusp_score_rows_pan_device(
            self._h, rows, samples, n, onsets, lengths, d_gains, _ptr(pans, n), _ptr(comp, n), n_total_samples, d_init, int(bool(raw)), d_out, stream))

    def score_rows_frac(self, rows, row_samples, n_channels, onsets, fracs, n_total_samples, d_out, lengths=None, d_gains=None, d_init=None, raw=False, pans=None,
                        comp=None, stream=None):
        """score_rows_device — or, with pans, score_rows_pan (n_channels must be 1, the timeline has two) — with voice k starting at
        onsets[k] + fracs[k] samples (dusp_score_rows_frac_device; dusp_amd/mix.py score_chain_rows / score_chain_rows_panned with fracs is
        the contract): fracs a HOST array of finite f64 in [0, 1), None for all zero.  A voice with a fraction is heard through the
        reference Delay's two taps and covers one more sample; one without is the voice of those calls, and a call without any fraction
        launches their kernels.  score_last_ms() reports the call."""
        def placed(n):
            place = Placement(n, pans, comp, fracs, fracs_first=True)
            if place.kind == "pan" and n == 0:  # (no voices: `|| 0`, or a copy, of both channels of d_init; the pointer only says "two channels")
                return place.fracs, np.zeros(1, dtype=np.float32), np.ones(1, dtype=np.float64)
            return place.fracs, place.pans, place.comp

        self._score_rows_call(rows, row_samples, onsets, lengths, placed, lambda n, rows, samples, onsets, lengths, fracs, pans, comp: self._L.dusp_score_rows_frac_device(
            self._h, rows, samples, n, n_channels, onsets, _ptr(fracs, n), lengths, d_gains, _ptr(pans), _ptr(comp), n_total_samples, d_init, int(bool(raw)), d_out, stream))

    def score_rows_space(self, rows, row_samples, onsets, delays, tap_gains, n_total_samples, d_out, lengths=None, d_gains=None, d_init=None, raw=False, stream=None):
        """score_rows_device over MONO rows, voice k heard by speaker c — channel c of a timeline of C — through the gain tap_gains[k][c]
        and a delay of delays[k][c] samples (dusp_score_rows_space_device; dusp_amd/mix.py score_chain_rows_placed is the contract): rows
        are the voices' DEVICE pointers, voice k f32 [row_samples[k]]; delays and tap_gains HOST arrays of f64 [voices][C], 1 <= C <= 8,
        the delays finite in [0, 2^24] and the gains finite (dusp_amd.space_taps makes both from places and speakers); d_init (which may
        be d_out) and d_out f32 [C][n_total_samples].  score_last_ms() reports the call."""
        self._score_rows_call(rows, row_samples, onsets, lengths, lambda n: tap_arrays((delays, tap_gains), n), lambda n, rows, samples, onsets, lengths, delays, tap_gains: self._L.dusp_score_rows_space_device(
            self._h, rows, samples, n, delays.shape[1], onsets, lengths, d_gains, _ptr(delays, n), _ptr(tap_gains, n), n_total_samples, d_init, int(bool(raw)), d_out, stream))

    def score_rows_stereo(self, rows, row_samples, row_channels, onsets, pans, n_total_samples, d_out, lengths=None, d_gains=None, d_init=None, raw=False, comp=None,
                          fracs=None, stream=None):
        """score_rows_device over rows of ONE OR TWO channels into a timeline of two (dusp_score_rows_stereo_device; dusp_amd/mix.py
        score_chain_rows_stereo is the contract): rows are the voices' DEVICE pointers, voice k planar f32 [row_channels[k]][row_samples[k]];
        pans a HOST array of f32 with NaN (or None) for a voice that is not placed (None: nothing placed) — a mono voice with a finite
        pan is score_rows_pan's voice, one without feeds both channels, a voice of two channels is not placed; fracs as score_rows_frac's
        (None: all zero); d_init (which may be d_out) and d_out f32 [2][n_total_samples].  score_last_ms() reports the call."""
        def placed(n):
            channels = np.asarray(row_channels) if n else np.zeros(0, dtype=np.uint32)
            if channels.shape != (n,) or channels.dtype.kind not in "iu":
                raise ValueError("dusp-hip: row_channels must be whole numbers of shape (voices=%d,)" % n)
            place = stereo_pan_arrays(pans, n, comp)
            check_stereo_kinds(channels.tolist(), place[0])
            return (np.ascontiguousarray(channels, dtype=np.uint32), frac_arrays(fracs, n) if fracs is not None else None) + place

        self._score_rows_call(rows, row_samples, onsets, lengths, placed, lambda n, rows, samples, onsets, lengths, channels, fracs, pans, comp: self._L.dusp_score_rows_stereo_device(
            self._h, rows, samples, _ptr(channels, n), n, onsets, _ptr(fracs, n), lengths, d_gains, _ptr(pans, n), _ptr(comp, n), n_total_samples, d_init, int(bool(raw)), d_out, stream))

    def score_rows_send(self, rows, row_samples, n_channels, onsets, sends, n_total_samples, d_out, d_send_out, lengths=None, d_gains=None, d_init=None, d_send_init=None,
                        raw=False, pans=None, comp=None, stream=None):
        """score_rows_device — or, with pans, score_rows_pan (n_channels must be 1, the timelines have two) — with effect sends
        (dusp_score_rows_send_device; dusp_amd/mix.py score_chain_sends is the contract): sends a HOST array of finite f32
        [buses][voices], 1 .. 4 buses (one bus: [voices] will do); every term the dry chain adds also goes, times the voice's level,
        to bus b's send timeline.  d_send_init (None: +0; may be d_send_out) and d_send_out: f32 [buses][C][n_total_samples], always
        raw.  score_last_ms() reports the call."""
        def placed(n):
            a = np.asarray(sends)
            levels = check_sends(a, n, 1 if a.ndim == 1 else a.shape[0])
            return (levels,) + (pan_arrays(pans, n, comp) if pans is not None else (None, None))

        self._score_rows_call(rows, row_samples, onsets, lengths, placed, lambda n, rows, samples, onsets, lengths, levels, pans, comp: self._L.dusp_score_rows_send_device(
            self._h, rows, samples, n, n_channels, onsets, lengths, d_gains, _ptr(pans), _ptr(comp), levels.shape[0], _ptr(levels), n_total_samples, d_init, int(bool(raw)), d_out,
            d_send_init, d_send_out, stream))

    def score_return(self, d_dry, d_wets, n_floats, d_out, raw=False, stream=None):
        """Device pointers: d_out[j] = d_dry[j] + d_wets[0][j] + ... over n_floats floats, left-deep with one f32 rounding an add, `|| 0`
        unless raw (dusp_score_return_device; dusp_amd/mix.py bus_return is the contract).  d_wets: 1 .. 4 pointers; d_out may be d_dry."""
        wets = (ctypes.c_void_p * max(len(d_wets), 1))(*d_wets)
        self._check(self._L.dusp_score_return_device(self._h, d_dry, ctypes.addressof(wets), len(d_wets), n_floats, int(bool(raw)), d_out, stream))

    def score_tracks_mix(self, d_direct, d_tracks, n_floats, d_out, faders=None, levels=None, d_feed_out=None, d_feed_init=None, raw=False, stream=None):
        """Device pointers: d_out[j] = d_direct[j] + term_0[j] + ... over n_floats floats, term_g = d_tracks[g][j] times faders[g] (None:
        as it stands), left-deep with one f32 rounding an add, `|| 0` unless raw; with levels, HOST f32 [buses][tracks] (0 .. 4 buses),
        d_feed_out[b][j] = (d_feed_init ? d_feed_init[b][j] : +0) + f32(term_0[j] * levels[b][0]) + ..., f32 [buses][n_floats], always raw
        (dusp_score_tracks_mix_device; dusp_amd/mix.py track_mix is the contract).  d_tracks: 1 .. 8 pointers; d_out may be d_direct,
        d_feed_out may be d_feed_init.  score_last_ms() reports the call."""
        tracks = (ctypes.c_void_p * max(len(d_tracks), 1))(*d_tracks)
        if faders is not None:
            faders = np.ascontiguousarray(faders, dtype=np.float32)
            if faders.shape != (len(d_tracks),):
                raise ValueError(TRACKS_FADERS_SHAPE % len(d_tracks))
        n_buses = 0
        if levels is not None:
            levels = np.ascontiguousarray(levels, dtype=np.float32)
            if levels.ndim != 2 or levels.shape[1] != len(d_tracks):
                raise ValueError(TRACKS_SENDS_SHAPE % (levels.shape[0] if levels.ndim == 2 else 0, len(d_tracks)))
            n_buses = levels.shape[0]
        self._check(self._L.dusp_score_tracks_mix_device(self._h, d_direct, ctypes.addressof(tracks), len(d_tracks), _ptr(faders), n_buses, _ptr(levels, n_buses), n_floats,
                                                         int(bool(raw)), d_out, d_feed_init, d_feed_out, stream))

    def score_stems_mix(self, d_direct, d_tracks, n_floats, d_out, d_stems, faders=None, levels=None, d_feed_out=None, d_feed_init=None, raw=False, stream=None):
        """score_tracks_mix with 0 .. 8 tracks, which also writes d_stems, f32 [1 + tracks][n_floats]: slot 0 d_direct || 0, slot 1 + g
        term g || 0 (dusp_score_stems_mix_device; mix.track_terms and mix.stems are the contract).  d_stems aliases no other buffer."""
        tracks = (ctypes.c_void_p * max(len(d_tracks), 1))(*d_tracks)
        if faders is not None:
            faders = np.ascontiguousarray(faders, dtype=np.float32)
            if faders.shape != (len(d_tracks),):
                raise ValueError(TRACKS_FADERS_SHAPE % len(d_tracks))
        n_buses = 0
        if levels is not None:
            levels = np.ascontiguousarray(levels, dtype=np.float32)
            if levels.ndim != 2 or levels.shape[1] != len(d_tracks):
                raise ValueError(TRACKS_SENDS_SHAPE % (levels.shape[0] if levels.ndim == 2 else 0, len(d_tracks)))
            n_buses = levels.shape[0]
        self._check(self._L.dusp_score_stems_mix_device(self._h, d_direct, ctypes.addressof(tracks), len(d_tracks), _ptr(faders, len(d_tracks)), n_buses,
                                                        _ptr(levels, n_buses and len(d_tracks)), n_floats, int(bool(raw)), d_out, d_feed_init, d_feed_out, d_stems, stream))

    def score_stems_return(self, d_dry, d_wets, n_floats, d_out, d_stem_buses, d_stem_direct=None, raw=False, stream=None):
        """score_return which also copies wet b into d_stem_buses + b * n_floats floats and, d_stem_direct given, writes d_dry || 0 there
        (dusp_score_stems_return_device; mix.bus_return and mix.stems are the contract).  The slots alias no other buffer."""
        wets = (ctypes.c_void_p * max(len(d_wets), 1))(*d_wets)
        self._check(self._L.dusp_score_stems_return_device(self._h, d_dry, ctypes.addressof(wets), len(d_wets), n_floats, int(bool(raw)), d_out, d_stem_direct, d_stem_buses, stream))

    def peak_common(self, d_peaks, n_peaks, d_common, stream=None):
        """Device pointers: d_common[i] = the largest of d_peaks[0 .. n_peaks), compared as unsigned words, for every i < n_peaks
        (dusp_peak_common_device; wav.common_peak): what encode() reads as d_peaks to give all instances one gain."""
        self._check(self._L.dusp_peak_common_device(self._h, d_peaks, n_peaks, d_common, stream))

    def meter_device(self, d_planar, n_signals, n_channels, n_samples, sample_rate, d_sumsq, d_hops, stream=None):
        """Device pointers: the meter kernels alone (dusp_meter_device; mix.meters is the contract) over f32 [n_signals][n_channels]
        [n_samples] -> d_sumsq f64 [n_signals][n_channels], the sums of squares, and d_hops f64 [n_signals][ceil(n_samples / hop)], per
        hop of 100 ms the sum over the channels of the K-weighted squares.  Timed by score_last_ms; meter_last_ms has the passes."""
        self._check(self._L.dusp_meter_device(self._h, d_planar, n_signals, n_channels, n_samples, int(sample_rate), d_sumsq, d_hops, stream))

    def meter_last_ms(self):
        """-> the four passes of the most recent meter_device call in ms, by HIP events (dusp_meter_last_ms; waits for that call): the
        segments from rest, the walk over their states, the segments from their true states, the reduction"""
        ms = (ctypes.c_float * 4)()
        self._check(self._L.dusp_meter_last_ms(self._h, ctypes.addressof(ms)))
        return tuple(ms)

    def meter(self, planar, sample_rate):
        """planar float32 [signals, channels, samples] (or [channels, samples]: one signal) in host memory -> what mix.meters returns
        but the energies: dict(rms [S, C], lufs [S], momentary [S, n_blocks], hop, block), float64, metered on the device and gated in
        the library (dusp_meter_host)."""
        planar = np.ascontiguousarray(planar, dtype=np.float32)
        if planar.ndim == 2:
            planar = planar[None]
        if planar.ndim != 3:
            raise ValueError("dusp-hip: the signals to meter are float32 of shape (signals, channels, samples)")
        if not int(sample_rate) >= METER_RATE_MIN:
            raise ValueError(METER_RATE_LOW % sample_rate)
        S, C, n = planar.shape
        rms, lufs, momentary = np.zeros((S, C)), np.full(S, -np.inf), np.zeros((S, meter_blocks(n, sample_rate)))
        if n:
            self._check(self._L.dusp_meter_host(self._h, planar.ctypes.data, S, C, n, int(sample_rate), rms.ctypes.data, lufs.ctypes.data, _ptr(momentary)))
        return dict(rms=rms, lufs=lufs, momentary=momentary, hop=meter_hop(sample_rate), block=4 * meter_hop(sample_rate))

    def true_peak_device(self, d_planar, n_signals, n_channels, n_samples, sample_rate, d_words, stream=None):
        """Device pointers: the true-peak kernel alone (dusp_true_peak_device; mix.true_peak is the contract) over f32 [n_signals]
        [n_channels][n_samples] -> d_words uint64 [n_signals][n_channels], the bits of every row's true peak as a double.  Timed by
        score_last_ms."""
        self._check(self._L.dusp_true_peak_device(self._h, d_planar, n_signals, n_channels, n_samples, int(sample_rate), d_words, stream))

    def true_peak_tile(self, n_signals, n_channels, n_samples, sample_rate):
        """-> the output positions a workgroup of that true-peak call owns on this context's device (dusp_true_peak_tile)"""
        return int(self._L.dusp_true_peak_tile(self._h, n_signals, n_channels, n_samples, int(sample_rate)))

    def true_peak(self, planar, sample_rate):
        """planar float32 [signals, channels, samples] (or [channels, samples]: one signal) in host memory -> what mix.true_peak
        returns: float64 [signals, channels], linear, taken on the device (dusp_true_peak_host)."""
        planar = np.ascontiguousarray(planar, dtype=np.float32)
        if planar.ndim == 2:
            planar = planar[None]
        if planar.ndim != 3:
            raise ValueError("dusp-hip: the signals to take the true peak of are float32 of shape (signals, channels, samples)")
        if not int(sample_rate) > 0:
            raise ValueError("dusp-hip: the true peak needs a sample rate, not %r: it decides the oversampling" % (sample_rate,))
        S, C, n = planar.shape
        got = np.zeros((S, C))
        if n and S and C:
            self._check(self._L.dusp_true_peak_host(self._h, planar.ctypes.data, S, C, n, int(sample_rate), got.ctypes.data))
        return got

    def limit_device(self, d_planar, n_signals, n_channels, n_samples, sample_rate, threshold, window, d_q=None, d_gain=None, d_smallest=None, stream=None):
        """Device pointers: the limiter's two kernels alone (dusp_limit_device; mix.limit is the contract), IN PLACE over f32 [n_signals]
        [n_channels][n_samples].  Optional: d_q uint32 [n_samples], the words q; d_gain float64 [n_samples], the curve; d_smallest, one
        uint64, the smallest window sum (reduction = word / (window x 2^30)).  Timed by score_last_ms; limit_last_ms has the two kernels."""
        self._check(self._L.dusp_limit_device(self._h, d_planar, n_signals, n_channels, n_samples, int(sample_rate), float(threshold), int(window), d_q, d_gain, d_smallest, stream))

    def limit_last_ms(self):
        """-> the two kernels of the most recent limit_device call in ms, by HIP events (dusp_limit_last_ms; waits for that call): the
        envelope kernel, the gain / apply kernel"""
        ms = (ctypes.c_float * 2)()
        self._check(self._L.dusp_limit_last_ms(self._h, ctypes.addressof(ms)))
        return tuple(ms)

    def limit_tile(self, n_samples, window):
        """-> the samples a workgroup of that limiter call owns on this context's device (dusp_limit_tile)"""
        return int(self._L.dusp_limit_tile(self._h, n_samples, int(window)))

    def limit_release_device(self, d_planar, n_signals, n_channels, n_samples, sample_rate, threshold, window, release, d_q=None, d_held=None, d_gain=None, d_smallest=None,
                             stream=None):
        """limit_device with a release of `release` samples, 1 .. 2^22 (dusp_limit_release_device; mix.limit(..., release=) is the
        contract): the envelope kernel, then the hold, release and mean / apply kernels.  d_held: optional, uint32 [n_samples + window
        - 1], the held curve.  Timed by score_last_ms; limit_release_last_ms has the four kernels."""
        self._check(self._L.dusp_limit_release_device(self._h, d_planar, n_signals, n_channels, n_samples, int(sample_rate), float(threshold), int(window), int(release), d_q, d_held,
                                                      d_gain, d_smallest, stream))

    def limit_release_last_ms(self):
        """-> the four kernels of the most recent limit_release_device call in ms, by HIP events (dusp_limit_release_last_ms; waits for
        that call): envelope, hold, release, mean / apply"""
        ms = (ctypes.c_float * 4)()
        self._check(self._L.dusp_limit_release_last_ms(self._h, ctypes.addressof(ms)))
        return tuple(ms)

    def limit_release_tile(self, n_samples, window, release):
        """-> the positions a workgroup of that call owns on this context's device (dusp_limit_release_tile)"""
        return int(self._L.dusp_limit_release_tile(self._h, n_samples, int(window), int(release)))

    def limit(self, planar, sample_rate, threshold, window, release=0):
        """planar float32 [signals, channels, samples] (or [channels, samples]: one signal) in host memory -> what mix.limit returns:
        (limited float32 of planar's shape, g float64 [samples], reduction), limited on the device under ONE curve
        (dusp_limit_host).  threshold: linear, finite, above 0; window: 1 .. 4096 samples; release: 0, or the limiter's release of its
        own, 1 .. 2^22 samples (dusp_limit_release_host)."""
        planar = np.ascontiguousarray(planar, dtype=np.float32)
        shape = planar.shape
        if planar.ndim == 2:
            planar = planar[None]
        if planar.ndim != 3:
            raise ValueError("dusp-hip: the signals to limit are float32 of shape (signals, channels, samples)")
        if not int(sample_rate) > 0:
            raise ValueError("dusp-hip: the limiter needs a sample rate, not %r: it decides the oversampling" % (sample_rate,))
        if not (isinstance(threshold, (int, float, np.integer, np.floating)) and np.isfinite(threshold) and threshold > 0):
            raise ValueError(LIMITER_THRESHOLD_BAD)
        if not (isinstance(window, (int, np.integer)) and 1 <= window <= LIMITER_WINDOW_MAX):
            raise ValueError(LIMITER_WINDOW_SAMPLES)
        if not (isinstance(release, (int, np.integer)) and not isinstance(release, (bool, np.bool_)) and 0 <= release <= LIMITER_RELEASE_MAX):
            raise ValueError(LIMITER_RELEASE_SAMPLES)
        S, C, n = planar.shape
        limited, g, reduction = np.empty_like(planar), np.ones(n), ctypes.c_double(1.0)
        if n and S and C and release:
            if not hasattr(self._L, "dusp_limit_release_host"):
                raise DuspHipError(-3, "dusp-hip: this library's limiter has no release (dusp_limit_release_host is missing)")
            self._check(self._L.dusp_limit_release_host(self._h, planar.ctypes.data, S, C, n, int(sample_rate), float(threshold), int(window), int(release), limited.ctypes.data,
                                                        g.ctypes.data, ctypes.addressof(reduction)))
        elif n and S and C:
            self._check(self._L.dusp_limit_host(self._h, planar.ctypes.data, S, C, n, int(sample_rate), float(threshold), int(window), limited.ctypes.data, g.ctypes.data,
                                                ctypes.addressof(reduction)))
        return limited.reshape(shape), g, float(reduction.value)

    def render_score_parts(self, parts, part_of, onsets, n_total_samples, lengths=None, gains=None, tile_bytes=0, format=None, normalise=NORMALISE_NONE, pinned=None,
                           pans=None, fracs=None, taps=None, stereo=False, master=None, buses=None, sends=None, tracks=None, stems=False, meters=False, true_peak=False,
                           loudness=None, true_peak_max=-1.0, limiter=False, limiter_window=0.005, limiter_release=None):
        """Host round trip that delivers a PIECE of several instruments (dusp_render_host_score_parts).  parts: a list of
        (program, n_voice_samples, n_instances, params) — programs of this context with one number of output channels; voice k of the
        chain is the next unused instance of part part_of[k].  Bit for bit mix.score_chain_rows over what each program's render() gives
        on its compiled kernel, in the caller's voice order, whatever tile_bytes (0: the library's default) cuts the voice list into.
        onsets, lengths, gains: per voice, in chain order; format, normalise and what is returned: as Program.render_score.
        pans (one finite f32 a voice): the parts are MONO and voice k is panned where it is added (dusp_render_host_score_parts_pan;
        mix.score_chain_rows_panned): the result has two channels.
        fracs (one finite f64 in [0, 1) a voice): voice k starts at onsets[k] + fracs[k] samples (dusp_render_host_score_parts_frac; the
        contracts above with fracs), with or without pans.
        taps = (delays, gains), f64 [voices][C] each: the parts are MONO and voice k is heard by speaker c through gains[k][c] and a
        delay of delays[k][c] samples (dusp_render_host_score_parts_space; mix.score_chain_rows_placed): the result has C channels.
        Not together with pans or fracs.
        stereo=True: the parts have ONE OR TWO output channels and the result has two (dusp_render_host_score_parts_stereo;
        mix.score_chain_rows_stereo): pans may be None (nothing placed) or hold None / NaN for a voice that is not placed, and a voice
        of a two-channel part is not placed; fracs as above.  Not together with taps.
        master = (program, params): the mix goes through that program before it is delivered (dusp_render_host_score_piece, the one
        entry that takes every placement above as a record; mix.master_chain is the contract) — a program of this context with ONE
        input stream and ONE output channel, channel c of the timeline instance c of it, params its table [n_params][timeline
        channels] (None without parameters).  The library refuses what is no master, before anything renders.
        buses = [(program, params), ...] with sends, f32 [buses][voices]: effect sends (dusp_render_host_score_piece_buses;
        mix.score_chain_sends, mix.master_chain and mix.bus_return are the contract) — 1 .. 4 programs, each what a master is; voice k
        gives sends[b][k] of what it adds to the mix to bus b, every bus is rendered over its send timeline, and their outputs are
        added to the dry mix in order, in front of the master where there is one.  With plain rows and with pans; fracs, taps and
        stereo are refused together with sends.
        tracks = dict(n_tracks, track_of, programs, faders=None, track_sends=None): sub-mixes (dusp_render_host_score_piece_tracks;
        mix.track_mix is the contract) — voice k goes to track track_of[k], or with -1 straight to the mix; programs is a list of
        (program, [track numbers], params), each what a master is and ONE program for the tracks it lists, params its table
        [n_params][tracks x timeline channels]; a track in no program has no circuit.  faders: one finite f32 a track; track_sends:
        f32 [buses][tracks], with buses, whose sends are then None.  Whatever the placement.
        stems=True: the direct mix, every track and every bus return beside the mix (dusp_render_host_score_piece_stems; mix.stems is
        the contract, mix.stem_names the order) -> (signals, peaks): signals [S + 1, channels, n_total] float32 without a format, else
        [S + 1, n_total, channels(, 3)] frames under ONE gain (wav.encode_stems), the mix last and exactly what the call returns
        without stems; peaks float32 [S + 1], every signal's own, whatever the format.
        meters=True: the RMS and the BS.1770 loudness of every signal the call delivers — its S + 1 signals with stems, else the mix —
        at the parts' sample rate (dusp_render_host_score_piece_meters; mix.meters is the contract) -> (what the call returns without
        meters, dict(rms [signals, channels], lufs [signals], momentary [signals, n_blocks], hop, block)), all float64.
        true_peak=True (implies meters): the dict gains true_peak [signals, channels], linear, the true peak of every signal and
        channel the call delivers (dusp_render_host_score_piece_loudness; mix.true_peak is the contract).
        loudness (a finite number of LUFS; implies true_peak; with a format, normalise 0) and true_peak_max (dBTP, at most 0): the
        frames of every signal are encoded under ONE gain that brings the MIX to that loudness unless the largest true peak of any
        signal would then exceed the ceiling (mix.loudness_gain; wav.encode_at_level has the bytes); the dict gains gain (a float) and
        level (numpy.float32).
        limiter=True (with loudness) and limiter_window (seconds, default 0.005; at most 4096 samples): where the largest true peak
        lies above the ceiling seen from the target, every delivered signal is first limited under ONE look-ahead gain curve
        (dusp_render_host_score_piece_limiter; mix.deliver_limited is the contract), and what the call returns — the meters, the
        peaks, gain and level — then describes the limited signals; the dict gains limiter, a dict of engaged, threshold, window (in
        samples), reduction, lufs_in and true_peak_in.
        limiter_release (seconds, with limiter=True; at most 2^22 samples): the limiter's release of its own
        (dusp_render_host_score_piece_limiter_release; mix.deliver_limited(..., release=) is the contract); the limiter's dict then
        has release, in samples."""
        stems, meters, true_peak = check_stems(stems), check_meters(meters), check_true_peak(true_peak)
        loudness, true_peak_max = check_loudness(loudness, true_peak_max, normalise, format is not None)
        window = check_limiter(limiter, limiter_window, loudness, parts[0][0].sample_rate if parts else 1)
        release = check_limiter_release(limiter_release, limiter, parts[0][0].sample_rate if parts else 1)
        true_peak = true_peak or loudness is not None
        meters = meters or true_peak
        if tracks is not None:
            track_of, faders, track_sends = check_tracks(len(part_of), tracks["n_tracks"], tracks["track_of"], tracks.get("faders"), tracks.get("track_sends"),
                                                         0 if buses is None else len(buses), sends)
        elif buses is None and sends is not None:
            raise ValueError(SENDS_WITHOUT_BUSES)
        if buses is not None and tracks is None:
            if sends is None:
                raise ValueError(BUSES_WITHOUT_SENDS)
            refuse_sends_placement(fracs, taps, stereo)
        Placement.refuse_together(pans, fracs, taps, stereo)
        if not parts:
            raise ValueError("dusp-hip: a piece has at least one part")
        n = len(part_of)
        part_of = np.asarray(part_of)
        if part_of.shape != (n,) or part_of.dtype.kind not in "iu" or np.any(part_of < 0) or np.any(part_of >= len(parts)):
            raise ValueError("dusp-hip: part_of names a part, 0 .. %d, for each voice" % (len(parts) - 1))
        part_of = np.ascontiguousarray(part_of, dtype=np.uint32)
        onsets = _whole_samples(onsets, n, "onsets")
        if lengths is not None:
            lengths = _whole_samples(lengths, n, "lengths")
        gains = _gains_table(gains, n, "voices")
        if int(tile_bytes) < 0:
            raise ValueError("dusp-hip: tile_bytes must be 0 (the default tile) or a number of bytes")
        table = (ScorePart * len(parts))()
        keep = []  # (the parameter tables, alive across the call)
        for p, (prog, n_voice_samples, n_instances, params) in enumerate(parts):
            keep.append(prog._params_table(params, n_instances, "dusp-hip: the params of part %d must have shape" % p))
            table[p] = ScorePart(prog._h, n_instances, n_voice_samples, _ptr(keep[-1]))
        place = Placement(n, pans, None, fracs, taps, stereo, fracs_first=True)
        if place.kind == "stereo":
            check_stereo_kinds([parts[p][0].n_out_channels for p in part_of], place.pans)
        n_ch = place.channels(parts[0][0].n_out_channels)  # (parts that do not fit the placement: the library refuses them)
        voices = (table, len(parts), n, part_of.ctypes.data, onsets.ctypes.data)
        if master is not None or buses is not None or tracks is not None or stems or meters:
            how = ScorePlacement(PLACE_KINDS[place.kind], _ptr(place.fracs), _ptr(place.pans), _ptr(place.comp), n_ch if place.kind == "space" else 0,
                                 _ptr(place.taps[0]) if place.taps else None, _ptr(place.taps[1]) if place.taps else None)
            through = None
            if master is not None:
                prog, params = master
                params = prog._params_table(params, n_ch, "dusp-hip: the params of the master must have shape")  # (n_instances: the timeline's channels)
                through = ScoreMaster(prog._h, _ptr(params))
        if buses is not None:
            buses = list(buses)
            levels = check_sends(sends, n, len(buses)) if tracks is None else None
            circuits = (ScoreMaster * len(buses))()
            for b, (prog, params) in enumerate(buses):
                keep.append(prog._params_table(params, n_ch, "dusp-hip: the params of bus %d must have shape" % b))
                circuits[b] = ScoreMaster(prog._h, _ptr(keep[-1]))
            into = ScoreBuses(len(buses), ctypes.addressof(circuits), _ptr(levels))
        if tracks is not None:
            served = list(tracks["programs"])
            table_t = (ScoreTrackProgram * max(len(served), 1))()
            for p, (prog, which, params) in enumerate(served):
                which = np.ascontiguousarray(which, dtype=np.uint32)
                keep.append(which)
                keep.append(prog._params_table(params, len(which) * n_ch, "dusp-hip: the params of track program %d must have shape" % p))
                table_t[p] = ScoreTrackProgram(prog._h, len(which), which.ctypes.data, _ptr(keep[-1]))
            routed = ScoreTracks(tracks["n_tracks"], track_of.ctypes.data, len(served), ctypes.addressof(table_t), _ptr(faders), _ptr(track_sends))
        if meters:  # (one entry for every call: with or without stems, tracks, buses and a master)
            rate = parts[0][0].sample_rate
            if not rate >= METER_RATE_MIN:
                raise ValueError(METER_RATE_LOW % rate)
            n_signals = 1 + (tracks["n_tracks"] if tracks is not None else 0) + (len(buses) if buses is not None else 0) + 1 if stems else 1
            n_blocks = meter_blocks(n_total_samples, rate)
            got = dict(rms=np.zeros((n_signals, n_ch)), lufs=np.zeros(n_signals), momentary=np.zeros((n_signals, n_blocks)), hop=meter_hop(rate), block=4 * meter_hop(rate))
            want = ScoreMeters(n_signals, n_blocks, got["rms"].ctypes.data, got["lufs"].ctypes.data, _ptr(got["momentary"]))
            entry, loud = self._L.dusp_render_host_score_piece_meters, ()
            if true_peak:  # (the same entry with one more record)
                got["true_peak"] = np.zeros((n_signals, n_ch))
                gain, level = ctypes.c_double(1.0), ctypes.c_float(1.0)
                asked_loud = ScoreLoudness(int(loudness is not None), 0.0 if loudness is None else loudness, true_peak_max, got["true_peak"].ctypes.data, ctypes.addressof(gain),
                                           ctypes.addressof(level))
                entry, loud = self._L.dusp_render_host_score_piece_loudness, (ctypes.addressof(asked_loud),)
                if window:  # (... and one more)
                    if not hasattr(self._L, "dusp_render_host_score_piece_limiter"):
                        raise DuspHipError(-3, "dusp-hip: this library has no limiter (dusp_render_host_score_piece_limiter is missing)")
                    engaged, did = ctypes.c_int(0), (ctypes.c_double * 4)(0.0, 1.0, 0.0, 0.0)
                    at = ctypes.addressof(did)
                    asked_limiter = ScoreLimiter(window, ctypes.addressof(engaged), at, at + 8, at + 16, at + 24)
                    entry, loud = self._L.dusp_render_host_score_piece_limiter, loud + (ctypes.addressof(asked_limiter),)
                    if release:  # (... and the same record with a release behind it)
                        if not hasattr(self._L, "dusp_render_host_score_piece_limiter_release"):
                            raise DuspHipError(-3, "dusp-hip: this library's limiter has no release (dusp_render_host_score_piece_limiter_release is missing)")
                        asked_release = ScoreLimiterRelease(asked_limiter, release)
                        entry, loud = self._L.dusp_render_host_score_piece_limiter_release, loud[:-1] + (ctypes.addressof(asked_release),)
            if stems:
                if format is None:
                    fmt, normalise, out = 0, 0, self.host_empty((n_signals, n_ch, n_total_samples), pinned)
                else:
                    fmt, normalise, out, _ = _pcm_out(self, format, normalise, (n_total_samples, n_ch), pinned, batch=n_signals)
                peak, asked = np.empty(n_signals, dtype=np.float32), ScoreStems(n_signals)
            else:
                fmt, normalise, out, peak = _pcm_out(self, format, normalise, (n_total_samples, n_ch), pinned)
            self._check(entry(*voices, _ptr(lengths), _ptr(gains), ctypes.addressof(how), ctypes.addressof(routed) if tracks is not None else None,
                              ctypes.addressof(into) if buses is not None else None, ctypes.addressof(through) if through is not None else None,
                              ctypes.addressof(asked) if stems else None, ctypes.addressof(want), *loud, n_total_samples, int(tile_bytes), fmt, normalise, out.ctypes.data, _ptr(peak)))
            if loudness is not None:
                got["gain"], got["level"] = float(gain.value), np.float32(level.value)
            if window:
                got["limiter"] = dict(engaged=bool(engaged.value), threshold=float(did[0]), window=window, reduction=float(did[1]), lufs_in=float(did[2]), true_peak_in=float(did[3]), release=release)
            return ((out, peak) if stems else out if peak is None else (out, peak[0])), got
        if stems:
            n_signals = 1 + (tracks["n_tracks"] if tracks is not None else 0) + (len(buses) if buses is not None else 0) + 1
            if format is None:
                fmt, normalise, out = 0, 0, self.host_empty((n_signals, n_ch, n_total_samples), pinned)
            else:
                fmt, normalise, out, _ = _pcm_out(self, format, normalise, (n_total_samples, n_ch), pinned, batch=n_signals)
            peaks, asked = np.empty(n_signals, dtype=np.float32), ScoreStems(n_signals)
            self._check(self._L.dusp_render_host_score_piece_stems(*voices, _ptr(lengths), _ptr(gains), ctypes.addressof(how), ctypes.addressof(routed) if tracks is not None else None,
                                                                   ctypes.addressof(into) if buses is not None else None,
                                                                   ctypes.addressof(through) if through is not None else None, ctypes.addressof(asked), n_total_samples,
                                                                   int(tile_bytes), fmt, normalise, out.ctypes.data, peaks.ctypes.data))
            return out, peaks
        if tracks is not None:
            fmt, normalise, out, peak = _pcm_out(self, format, normalise, (n_total_samples, n_ch), pinned)
            self._check(self._L.dusp_render_host_score_piece_tracks(*voices, _ptr(lengths), _ptr(gains), ctypes.addressof(how), ctypes.addressof(routed),
                                                                    ctypes.addressof(into) if buses is not None else None,
                                                                    ctypes.addressof(through) if through is not None else None, n_total_samples, int(tile_bytes), fmt,
                                                                    normalise, out.ctypes.data, _ptr(peak)))
            return out if peak is None else (out, peak[0])
        if buses is not None:
            fmt, normalise, out, peak = _pcm_out(self, format, normalise, (n_total_samples, n_ch), pinned)
            self._check(self._L.dusp_render_host_score_piece_buses(*voices, _ptr(lengths), _ptr(gains), ctypes.addressof(how), ctypes.addressof(into),
                                                                   ctypes.addressof(through) if through is not None else None, n_total_samples, int(tile_bytes), fmt,
                                                                   normalise, out.ctypes.data, _ptr(peak)))
            return out if peak is None else (out, peak[0])
        if master is not None:
            fmt, normalise, out, peak = _pcm_out(self, format, normalise, (n_total_samples, n_ch), pinned)
            self._check(self._L.dusp_render_host_score_piece(*voices, _ptr(lengths), _ptr(gains), ctypes.addressof(how), ctypes.addressof(through),
                                                             n_total_samples, int(tile_bytes), fmt, normalise, out.ctypes.data, _ptr(peak)))
            return out if peak is None else (out, peak[0])
        scaled, placed, timeline = (_ptr(lengths), _ptr(gains)), (_ptr(place.pans), _ptr(place.comp)), (n_total_samples, int(tile_bytes))
        if place.kind == "space":
            entry, args = self._L.dusp_render_host_score_parts_space, voices + scaled + (n_ch, place.taps[0].ctypes.data, place.taps[1].ctypes.data) + timeline
        elif place.kind == "stereo":
            entry, args = self._L.dusp_render_host_score_parts_stereo, voices + (_ptr(place.fracs),) + scaled + placed + timeline
        elif place.fracs is not None:  # (with the pans and their compensation, or two NULLs)
            entry, args = self._L.dusp_render_host_score_parts_frac, voices + (_ptr(place.fracs),) + scaled + placed + timeline
        elif place.kind == "pan":
            entry, args = self._L.dusp_render_host_score_parts_pan, voices + scaled + placed + timeline
        else:
            entry, args = self._L.dusp_render_host_score_parts, voices + scaled + timeline
        fmt, normalise, out, peak = _pcm_out(self, format, normalise, (n_total_samples, n_ch), pinned)
        self._check(entry(*args, fmt, normalise, out.ctypes.data, _ptr(peak)))
        return out if peak is None else (out, peak[0])

    def score_last_ms(self):
        """-> (kernel_ms, plan_ms, upload_ms) of the most recent score_device call (dusp_score_last_ms; waits for that launch): the kernel
        alone by HIP events, the plan on the host's clock, the plan's upload by events."""
        k, p, u = ctypes.c_float(), ctypes.c_float(), ctypes.c_float()
        self._check(self._L.dusp_score_last_ms(self._h, ctypes.byref(k), ctypes.byref(p), ctypes.byref(u)))
        return k.value, p.value, u.value

    def fill(self, d_ptr, n_floats, value=0.0, stream=None):
        self._check(self._L.dusp_fill_device(self._h, d_ptr, n_floats, value, stream))

    def close(self):
        if self._h and self._host_live > 0:  # arrays over the pinned pool are still alive: the last one closes
            self._close_pending = True
            return
        if self._h:
            self._L.dusp_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Program:
    def __init__(self, ctx, words, engine=ENGINE_AUTO):
        self.ctx = ctx
        self._L = ctx._L
        words = np.ascontiguousarray(words, dtype=np.float64)
        h = ctypes.c_void_p()
        ctx._check(self._L.dusp_program_build(ctx._h, words.ctypes.data, words.size, engine, ctypes.byref(h)))
        self._h = h
        self._read_info()

    def _read_info(self):
        info = ProgramInfo()
        self.ctx._check(self._L.dusp_program_info_get(self._h, ctypes.byref(info)))
        self.sample_rate = info.sample_rate
        self.n_units = info.n_units
        self.n_out_channels = info.n_out_channels
        self.n_params = info.n_params
        self.n_inputs = info.n_inputs
        self.engine = ENGINE_NAMES.get(info.engine, str(info.engine))
        self.shape = info.shape.decode()
        self.n_device_ops = info.n_device_ops

    def read_shape(self):
        """The program's shape string as of now (after a render it names the kernel that ran: "compiled kernel: ..." or not)."""
        self._read_info()
        return self.shape

    def continue_with(self, words):
        """dusp_program_continue: re-arm this rendered program from a later extraction of the same circuit
        (unit state and constants from `words`, delay lines / feedback chunks stay on the device)."""
        words = np.ascontiguousarray(words, dtype=np.float64)
        self.ctx._check(self._L.dusp_program_continue(self._h, words.ctypes.data, words.size))
        self._read_info()

    def _params_table(self, params, n_instances, must="params must have shape"):
        """the parameter table of a call -> contiguous float32 [n_params, n_instances], checked (must: how the refusal begins), or None
        for a program without parameters"""
        if not self.n_params:
            return None
        params = np.ascontiguousarray(params, dtype=np.float32)
        if params.shape != (self.n_params, n_instances):
            raise ValueError("%s (n_params=%d, n_instances=%d)" % (must, self.n_params, n_instances))
        return params

    def render(self, n_samples, n_instances=1, params=None, interleaved=False, inputs=None, pinned=None):
        """Host round trip: float32 [n_instances, n_out_channels, n_samples], or — interleaved — frames
        [n_instances, n_samples, n_out_channels] (the RenderStream / WAV layout, transposed on the device).
        inputs: the host-generated streams of this call, float32 [n_inputs, n_instances, n_samples] (programs with INPUT units)."""
        shape = (n_instances, n_samples, self.n_out_channels) if interleaved else (n_instances, self.n_out_channels, n_samples)
        out = self.ctx.host_empty(shape, pinned)  # pinned=None: by size; False: pageable memory (the staged download)
        params = self._params_table(params, n_instances)
        pp = _ptr(params)
        if self.n_inputs:
            inputs = np.ascontiguousarray(inputs, dtype=np.float32)
            if inputs.shape != (self.n_inputs, n_instances, n_samples):
                raise ValueError("inputs must have shape (n_inputs=%d, n_instances=%d, n_samples=%d)" % (self.n_inputs, n_instances, n_samples))
            self.ctx._check(self._L.dusp_render_host_inputs(self._h, n_instances, n_samples, pp, inputs.ctypes.data, out.ctypes.data, int(interleaved)))
            return out
        call = self._L.dusp_render_host_interleaved if interleaved else self._L.dusp_render_host
        self.ctx._check(call(self._h, n_instances, n_samples, pp, out.ctypes.data))
        return out

    def render_pcm(self, n_samples, n_instances=1, params=None, format="s16", normalise=NORMALISE_NONE, inputs=None, pinned=None):
        """Host round trip that delivers encoded frames (dusp_render_host_pcm): peak, gain, quantisation and interleave run on the device
        and 2 (s16) or 3 (s24) bytes per sample are downloaded.  Returns (data, peaks): data int16 [n_instances, n_samples, n_out_channels]
        for "s16", uint8 [.., .., .., 3] (little-endian 24-bit) for "s24", float32 for "f32"; peaks float32 [n_instances], every instance's
        max |x| before the gain.  normalise: 0 none, 1 shrink only an instance that would clip, 2 every instance to full scale."""
        fmt, normalise, out, peaks = _pcm_out(self.ctx, format, normalise, (n_samples, self.n_out_channels), pinned, batch=n_instances)
        params = self._params_table(params, n_instances)
        ip = None
        if self.n_inputs:
            inputs = np.ascontiguousarray(inputs, dtype=np.float32)
            if inputs.shape != (self.n_inputs, n_instances, n_samples):
                raise ValueError("inputs must have shape (n_inputs=%d, n_instances=%d, n_samples=%d)" % (self.n_inputs, n_instances, n_samples))
            ip = inputs.ctypes.data
        self.ctx._check(self._L.dusp_render_host_pcm(self._h, n_instances, n_samples, _ptr(params), ip, fmt, normalise, out.ctypes.data, peaks.ctypes.data))
        return out, peaks

    def render_mix(self, n_samples, n_instances, params=None, gains=None, tile_instances=0, format=None, normalise=NORMALISE_NONE, pinned=None):
        """Host round trip that delivers the MIX of the instances (dusp_render_host_mix): rendered tile by tile on the device and summed
        there in Sum.many's chain order (bit for bit mix.mix_chain over what render() gives on the circuit's compiled kernel: a mix waits
        for that kernel also where a first short render() under DUSP_WAVE_JIT=1 would not), so that device memory is bounded by the tile
        and one instance's worth of samples is downloaded.  gains: float32 [n_instances], a factor per instance.  tile_instances: 0 lets the
        library size the tile.  format None: float32 [n_out_channels, n_samples]; "s16" | "s24" | "f32": (data, peak) as render_pcm
        delivers one instance — data [n_samples, n_out_channels(, 3)] — with the mix's peak as one float32."""
        params, gains = self._params_table(params, n_instances), _gains_table(gains, n_instances, "n_instances")
        if int(tile_instances) < 0:
            raise ValueError("dusp-hip: tile_instances must be 0 (the default tile) or at least 1")
        fmt, normalise, out, peak = _pcm_out(self.ctx, format, normalise, (n_samples, self.n_out_channels), pinned)
        self.ctx._check(self._L.dusp_render_host_mix(self._h, n_instances, n_samples, _ptr(params), _ptr(gains), int(tile_instances), fmt, normalise, out.ctypes.data, _ptr(peak)))
        return out if peak is None else (out, peak[0])

    def render_score(self, n_voice_samples, n_total_samples, n_instances, onsets, lengths=None, params=None, gains=None, tile_instances=0, format=None,
                     normalise=NORMALISE_NONE, pinned=None):
        """Host round trip that delivers a SCORE (dusp_render_host_score): the instances are rendered for n_voice_samples each, tile by
        tile as render_mix renders them, and mixed on the device into a timeline of n_total_samples with instance k at sample onsets[k]
        — bit for bit mix.score_chain over what render() gives on the circuit's compiled kernel.  onsets, lengths: whole numbers of
        samples (onsets of any sign; lengths in 0 .. n_voice_samples clip a voice, None: whole voices).  gains, tile_instances, format,
        normalise and what is returned: as render_mix, over the timeline."""
        onsets = _whole_samples(onsets, n_instances, "onsets")
        if lengths is not None:
            lengths = _whole_samples(lengths, n_instances, "lengths")
        params, gains = self._params_table(params, n_instances), _gains_table(gains, n_instances, "n_instances")
        if int(tile_instances) < 0:
            raise ValueError("dusp-hip: tile_instances must be 0 (the default tile) or at least 1")
        fmt, normalise, out, peak = _pcm_out(self.ctx, format, normalise, (n_total_samples, self.n_out_channels), pinned)
        self.ctx._check(self._L.dusp_render_host_score(self._h, n_instances, n_voice_samples, n_total_samples, _ptr(params), _ptr(gains), onsets.ctypes.data, _ptr(lengths),
                                                       int(tile_instances), fmt, normalise, out.ctypes.data, _ptr(peak)))
        return out if peak is None else (out, peak[0])

    def render_device(self, n_samples, n_instances, d_params, d_out, stream=None, d_inputs=None):
        """Asynchronous render between device pointers (ints), e.g. torch tensors' data_ptr()."""
        if d_inputs is not None or self.n_inputs:
            self.ctx._check(self._L.dusp_render_device_inputs(self._h, n_instances, n_samples, d_params, d_inputs, d_out, stream))
        else:
            self.ctx._check(self._L.dusp_render_device(self._h, n_instances, n_samples, d_params, d_out, stream))

    def render_chain_window(self, first_sample, n_samples, d_init, raw, d_out, stream=None):
        """dusp_render_chain_window: the window [first_sample, first_sample + n_samples) of a fused sum-chain program's timeline, its sums
        continued from d_init (None: the chain's first voices are this program's); raw: a partial sum for the next rank (shard.chain_mixdown).
        first_sample: a multiple of 2048 up to 2^40; n_samples: up to 65535 blocks of 2048 — every window in that range is exact, anything
        else is refused here, before the library is called."""
        first_sample, n_samples = operator.index(first_sample), operator.index(n_samples)
        if first_sample < 0 or first_sample > CHAIN_FIRST_MAX:  # (whole blocks: the library's check)
            raise ValueError("dusp-hip: first_sample of a chain window must be in 0 .. 2^40, not %d" % first_sample)
        if n_samples < 1 or n_samples > CHAIN_SAMPLES_MAX:
            raise ValueError("dusp-hip: n_samples of a chain window must be in 1 .. %d (65535 blocks of %d samples), not %d" % (CHAIN_SAMPLES_MAX, CHAIN_BLOCK, n_samples))
        self.ctx._check(self._L.dusp_render_chain_window(self._h, first_sample, n_samples, d_init, int(bool(raw)), d_out, stream))

    def state(self, unit, instance=0):
        buf = np.zeros(128, dtype=np.float64)
        n = self.ctx._check(self._L.dusp_state_download(self._h, instance, unit, buf.ctypes.data, buf.size))
        return buf[:n].copy()

    def last_kernel_ms(self):
        ms = ctypes.c_float()
        self.ctx._check(self._L.dusp_last_kernel_ms(self._h, ctypes.byref(ms)))
        return ms.value

    def close(self):
        if self._h and self.ctx._h:  # (a context finalized first — the collector's order at exit — has taken its device with it)
            self._L.dusp_program_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
