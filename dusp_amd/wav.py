"""RIFF/WAVE files of rendered PCM, and the PCM sample contract on the host.

Byte-compatible with dusp_amd/js/lib/wav.js: 32-bit float (WAVE_FORMAT_IEEE_FLOAT, with a fact chunk), 24- and 16-bit
signed PCM.  The quantiser is the numpy restatement of dusp_amd/csrc/pcm_quant.hpp (what the device encoder computes,
include/dusp_hip.h "Device-side PCM delivery"); the tests use it as the reference for the device's bytes.

    encode_wav(channel_data, sample_rate, bit_depth=32)   channel_data: per-channel float arrays ([channels, samples])
    encode_wav(frames, sample_rate, bit_depth, frames=True)   float frames [samples, channels]
    encode_wav(encoded, sample_rate, bit_depth)   what Program.render_pcm returned for one instance: int16 [samples, channels]
                                                  (16), uint8 [samples, channels, 3] (24): only the header is added
    decode_wav(data) -> {"sampleRate", "numberOfChannels", "bitDepth", "format", "channelData": float32 [channels, samples]}
"""
import struct

import numpy as np

SCALE = {16: 32767.0, 24: 8388607.0}
NORMALISE_NONE, NORMALISE_CLIP, NORMALISE_FULL = 0, 1, 2


class WavError(ValueError):
    pass


def peak(x):
    """Exact max |x| as a float32, NaN if any sample is NaN: the maximum of `bits & 0x7fffffff` as unsigned integers
    (monotone over the non-NaN values; every NaN sorts above infinity)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    if x.size == 0:
        return np.float32(0)
    return np.array([np.max(x.view(np.uint32) & np.uint32(0x7fffffff))], dtype=np.uint32).view(np.float32)[0]


def gain(peak_value, normalise):
    """The gain an instance of this peak gets: 1 / (double)peak when normalising applies, else 1 (a double)."""
    p = np.float64(np.float32(peak_value))
    if normalise == NORMALISE_NONE or not np.isfinite(p):
        return np.float64(1.0)
    if normalise not in (NORMALISE_CLIP, NORMALISE_FULL):
        raise WavError("dusp-hip: normalise must be 0 (none), 1 (shrink only what clips) or 2 (to full scale)")
    return np.float64(1.0) / p if p > (1.0 if normalise == NORMALISE_CLIP else 0.0) else np.float64(1.0)


def quantise(x, g=1.0, bit_depth=16):
    """f32 samples -> int32 array of 16- or 24-bit values: (double)x * g, NaN -> 0, clamp to [-1, 1], times 32767 / 8388607,
    rounded half away from zero.  (floor-and-compare: floor(a + 0.5) is wrong for the double just below 0.5.)"""
    if bit_depth not in SCALE:
        raise WavError("dusp-hip: PCM bit depth must be 16 or 24")
    t = np.asarray(x, dtype=np.float32).astype(np.float64) * np.float64(g)
    t = np.where(np.isnan(t), 0.0, t)
    t = np.minimum(np.maximum(t, -1.0), 1.0)
    v = t * SCALE[bit_depth]
    a = np.abs(v)
    r = np.floor(a)
    r = r + (a - r >= 0.5)
    return np.where(v < 0, -r, r).astype(np.int32)


def scale_f32(x, g=1.0):
    """Format f32: (float)((double)x * g), not clamped, NaN left as it is."""
    with np.errstate(over="ignore", invalid="ignore"):
        return (np.asarray(x, dtype=np.float32).astype(np.float64) * np.float64(g)).astype(np.float32)


def pack(q, bit_depth):
    """int32 sample values -> their little-endian bytes: int16 [...] or uint8 [..., 3]."""
    q = np.asarray(q, dtype=np.int32)
    if bit_depth == 16:
        return q.astype("<i2")
    return np.ascontiguousarray(q.astype("<i4")).view(np.uint8).reshape(q.shape + (4,))[..., :3].copy()


def encode_frames(planar, bit_depth=16, normalise=NORMALISE_NONE):
    """One instance, planar f32 [channels, samples] -> (frames, peak): int16 [samples, channels], uint8 [samples, channels, 3]
    or float32 [samples, channels] (bit_depth 32), under ONE gain from the peak over all channels.  The device encoder's bytes."""
    planar = np.ascontiguousarray(planar, dtype=np.float32)
    p = peak(planar)
    g = gain(p, normalise)
    frames = planar.T
    if bit_depth == 32:
        return np.ascontiguousarray(scale_f32(frames, g)), p
    return np.ascontiguousarray(pack(quantise(frames, g, bit_depth), bit_depth)), p


def encode_wav(data, sample_rate, bit_depth=32, frames=False):
    if bit_depth not in (32, 24, 16):
        raise WavError("dusp-hip: WAV bitDepth must be 32 (float), 24 or 16 (PCM)")
    if not sample_rate or not sample_rate > 0:
        raise WavError("dusp-hip: WAV needs a sample rate")
    arr = data if isinstance(data, np.ndarray) else None
    if arr is not None and arr.dtype == np.int16 and bit_depth == 16 and arr.ndim == 2:
        n_channels, body = arr.shape[1], arr.astype("<i2").tobytes()
    elif arr is not None and arr.dtype == np.uint8 and bit_depth == 24 and arr.ndim == 3 and arr.shape[2] == 3:
        n_channels, body = arr.shape[1], arr.tobytes()
    elif arr is not None and arr.dtype.kind in "iu":
        raise WavError("dusp-hip: encoded frames must be int16 [samples, channels] (16 bit) or uint8 [samples, channels, 3] (24 bit)")
    else:
        if frames:
            fr = np.asarray(data, dtype=np.float32)
            if fr.ndim != 2:
                raise WavError("dusp-hip: frames must be [samples, channels]")
        else:
            if len(data) == 0:
                raise WavError("dusp-hip: nothing to encode (no channels)")
            fr = np.stack([np.asarray(ch, dtype=np.float32) for ch in data]).T
        n_channels = fr.shape[1]
        body = fr.astype("<f4").tobytes() if bit_depth == 32 else pack(quantise(fr, 1.0, bit_depth), bit_depth).tobytes()
    if n_channels < 1:
        raise WavError("dusp-hip: nothing to encode (no channels)")
    is_float = bit_depth == 32
    n_bytes = bit_depth // 8
    fmt_bytes = 18 if is_float else 16  # non-PCM formats carry cbSize and need a fact chunk
    header = 12 + 8 + fmt_bytes + (12 if is_float else 0) + 8
    total = header + len(body) + (len(body) & 1)
    out = b"RIFF" + struct.pack("<I", total - 8) + b"WAVE"
    out += b"fmt " + struct.pack("<IHHIIHH", fmt_bytes, 3 if is_float else 1, n_channels, int(sample_rate), int(sample_rate) * n_channels * n_bytes,
                                 n_channels * n_bytes, bit_depth)
    if is_float:
        out += struct.pack("<H", 0) + b"fact" + struct.pack("<II", 4, len(body) // (n_bytes * n_channels))
    out += b"data" + struct.pack("<I", len(body)) + body + (b"\0" if len(body) & 1 else b"")
    return out


def decode_wav(buf):
    buf = bytes(buf)
    if buf[0:4] != b"RIFF" or buf[8:12] != b"WAVE":
        raise WavError("dusp-hip: not a RIFF/WAVE file")
    p, fmt, data = 12, None, None
    while p + 8 <= len(buf):
        cid, size = buf[p:p + 4], struct.unpack_from("<I", buf, p + 4)[0]
        if cid == b"fmt ":
            tag, n_channels, sample_rate, _, _, bit_depth = struct.unpack_from("<HHIIHH", buf, p + 8)
            fmt = {"format": tag, "numberOfChannels": n_channels, "sampleRate": sample_rate, "bitDepth": bit_depth}
        elif cid == b"data":
            data = buf[p + 8:p + 8 + size]
        p += 8 + size + (size & 1)
    if fmt is None or data is None:
        raise WavError("dusp-hip: WAV without fmt / data chunk")
    n_channels, bit_depth = fmt["numberOfChannels"], fmt["bitDepth"]
    if fmt["format"] == 3:
        fr = np.frombuffer(data, dtype="<f4")
    elif bit_depth == 16:
        fr = (np.frombuffer(data, dtype="<i2").astype(np.float64) / 32767.0).astype(np.float32)
    elif bit_depth == 24:
        b = np.frombuffer(data, dtype=np.uint8).reshape(-1, 3).astype(np.int32)
        q = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
        fr = ((q - ((q & 0x800000) << 1)).astype(np.float64) / 8388607.0).astype(np.float32)
    else:
        raise WavError("dusp-hip: unsupported WAV sample format")
    fmt["channelData"] = np.ascontiguousarray(fr.reshape(-1, n_channels).T)
    return fmt


def common_peak(peaks):
    """The one peak of several signals: the largest of their peaks compared as unsigned bit patterns (a NaN wins) -> float32"""
    peaks = np.ascontiguousarray(peaks, dtype=np.float32)
    if peaks.size == 0:
        return np.float32(0)
    return np.array([np.max(peaks.view(np.uint32))], dtype=np.uint32).view(np.float32)[0]


def encode_stems(stack, bit_depth=16, normalise=NORMALISE_NONE):
    """The signals of a call with stems (mix.stems: float32 [S + 1, channels, samples]) -> (frames [S + 1, samples, channels] as
    encode_frames makes them — int16, uint8 [.., 3] or float32 — and peaks float32 [S + 1], every signal's own over all its channels)
    under ONE gain for all of them: gain(common_peak(peaks), normalise).  Delivered stems then still add up to the delivered mix, and
    none clips where the mix does not.  normalise 0 is the quantiser a signal.  The device's bytes (dusp_render_host_score_piece_stems)."""
    stack = np.ascontiguousarray(stack, dtype=np.float32)
    if stack.ndim != 3:
        raise WavError("dusp-hip: the stems are float32 of shape (signals, channels, samples)")
    peaks = np.array([peak(x) for x in stack], dtype=np.float32)
    g = gain(common_peak(peaks), normalise)
    frames = np.transpose(stack, (0, 2, 1))
    if bit_depth == 32:
        return np.ascontiguousarray(scale_f32(frames, g)), peaks
    return np.ascontiguousarray(pack(quantise(frames, g, bit_depth), bit_depth)), peaks


def encode_at_level(stack, bit_depth=16, level=1.0):
    """encode_stems' byte contract with every signal under gain(level, NORMALISE_FULL) — 1 / float64(float32(level)), or 1 for a level
    that is 0, NaN or Inf: `level` is the sample magnitude that is brought to full scale (mix.loudness_gain makes it from a loudness
    target).  At level = the common peak these are the bytes of encode_stems(stack, bit_depth, NORMALISE_FULL).  -> (frames, peaks),
    the peaks every signal's own sample peak.  The device's bytes with deliver = 1 (dusp_render_host_score_piece_loudness)."""
    stack = np.ascontiguousarray(stack, dtype=np.float32)
    if stack.ndim != 3:
        raise WavError("dusp-hip: the stems are float32 of shape (signals, channels, samples)")
    peaks = np.array([peak(x) for x in stack], dtype=np.float32)
    g = gain(level, NORMALISE_FULL)
    frames = np.transpose(stack, (0, 2, 1))
    if bit_depth == 32:
        return np.ascontiguousarray(scale_f32(frames, g)), peaks
    return np.ascontiguousarray(pack(quantise(frames, g, bit_depth), bit_depth)), peaks
