"""Loudness delivery without a device: the contract — mix.true_peak_taps against the structure and the sums the
windowed sinc has, mix.true_peak on signals whose true peak is known, mix.loudness_gain where the loudness limits, where the ceiling
limits and where the gain is unity, wav.encode_at_level against wav.encode_stems at the common peak — the refusal strings and the
routing of true_peak=, loudness= and true_peak_max=, the library's taps against Python's, and the text of the true-peak kernel on the
host under sanitizers (tests/native/truepeak_kernel_check.cpp)."""
import ctypes
import json
import math
import os
import subprocess

import numpy as np
import pytest

import dusp_amd as d
import master_cases as mc
import score_voices as sv
from dusp_amd import mix, render, runtime, wav
from test_piece_host import ROOT, SANITIZE


# ---- the taps ---------------------------------------------------------------------------------------------------------------------------

def test_the_taps_have_the_windowed_sincs_structure_and_sums():
    F, h = mix.true_peak_taps(48000)
    assert F == 4 and h.shape == (49,) and h.dtype == np.float64
    assert h[0] == 0.0 and h[48] == 0.0 and h[24] == 1.0
    assert all(h[j] == 0.0 for j in range(49) if (j - 24) % 4 == 0 and j != 24), "exactly 0 where F divides m"
    assert all(h[j] != 0.0 for j in range(1, 48) if (j - 24) % 4 != 0)
    assert np.allclose([h[p::4].sum() for p in range(4)], (1.0, 1.0004797919518407, 1.0009044839413876, 1.0004797919518404), rtol=0, atol=1e-12)
    assert np.allclose(h, h[::-1], rtol=0, atol=1e-15), "symmetric"
    for j in (1, 7, 23, 25, 30, 47):  # (the formula itself)
        m = j - 24
        assert abs(h[j] - math.sin(m * math.pi / 4) / (m * math.pi / 4) * 0.5 * (1 - math.cos(2 * math.pi * j / 48))) <= 1e-15
    F2, h2 = mix.true_peak_taps(96000)
    assert F2 == 2 and h2.shape == (49,) and h2[24] == 1.0 and h2[0] == h2[48] == 0.0
    assert all(h2[j] == 0.0 for j in range(0, 49, 2) if j != 24) and abs(h2[1::2].sum() - 1.000113462147264) <= 1e-12 and abs(h2[0::2].sum() - 1.0) <= 1e-12
    assert np.allclose(h2, h2[::-1], rtol=0, atol=1e-15)
    F1, h1 = mix.true_peak_taps(192000)
    assert F1 == 1 and h1.tolist() == [1.0]
    assert [mix.true_peak_taps(rate)[0] for rate in (8000, 48000, 95999, 96000, 191999, 192000)] == [4, 4, 4, 2, 2, 1]
    for rate in (0, -1):
        with pytest.raises(ValueError, match="the true peak needs a sample rate"):
            mix.true_peak_taps(rate)


def test_the_librarys_taps_are_pythons():
    L = runtime.load()
    for rate in (8000, 44100, 48000, 95999, 96000, 191999, 192000, 384000):
        factor, h49 = ctypes.c_int(0), (ctypes.c_double * 49)()
        assert L.dusp_true_peak_taps(rate, ctypes.byref(factor), h49) == 0
        F, h = mix.true_peak_taps(rate)
        want = np.zeros(49)
        want[:len(h)] = h
        assert factor.value == F and np.max(np.abs(np.array(h49[:]) - want)) <= 1e-15, rate
        assert all(h49[j] == 0.0 for j in range(49) if want[j] == 0.0) and h49[24 if F > 1 else 0] == 1.0
    assert L.dusp_true_peak_taps(0, ctypes.byref(factor), h49) != 0  # (a rate of 0 is refused)


# ---- known signals ----------------------------------------------------------------------------------------------------------------------

def tp(x, rate, **kw):
    return float(mix.true_peak(np.asarray(x, dtype=np.float32)[None, None], rate, **kw)[0, 0])


def test_signals_whose_true_peak_is_known():
    impulse = np.zeros(40, dtype=np.float32)
    impulse[7] = 1.0
    assert tp(impulse, 48000) == 1.0 and tp(-impulse, 96000) == 1.0 and tp(0.25 * impulse, 192000) == 0.25
    # the classic: a sine at fs / 4 with phase pi / 4 is sampled at 0.7071 on both sides of every crest
    classic = np.sin(2 * np.pi * np.arange(4800) / 4 + np.pi / 4).astype(np.float32)
    assert wav.peak(classic) == np.float32(0.70710677)
    got = tp(classic, 48000)
    assert 1.0 < got < 1.02 and abs(got - 1.01199) < 1e-5, got
    sine = np.sin(2 * np.pi * 997 * np.arange(48000) / 48000).astype(np.float32)
    assert abs(tp(sine, 48000) - 1.00063) < 1e-5
    assert tp(sine, 48000, taps=(1, [1.0])) == float(wav.peak(sine)) == tp(sine, 192000), "F = 1: the sample peak"
    square = (0.9 * np.sign(np.sin(2 * np.pi * 1000 * (np.arange(4800) + 0.5) / 48000))).astype(np.float32)
    got = tp(square, 48000)
    assert got > 1.1 and abs(got - 1.1264) < 1e-4, "overshoot: %r" % got
    # the library's own taps handed in give what the function's own give
    assert tp(classic, 48000, taps=mix.true_peak_taps(48000)) == tp(classic, 48000)


def test_the_tail_the_shapes_and_what_is_not_finite():
    # the largest value last: the peak lies behind the last sample, in the filter's tail
    x = np.full(30, 0.01, dtype=np.float32)
    x[-1] = 0.9
    F, h = mix.true_peak_taps(44100)
    inside = mix.true_peak(x[None, None, :-1], 44100)[0, 0]
    assert h[24] == 1.0  # (phase 0 gives the last sample back at u = n - 1 + 6, behind the row's end)
    assert tp(x, 44100) >= float(np.float32(0.9)) > 0.5 > inside
    # n below K - 1, n = 1, n = 0
    assert tp([0.5], 48000) == 0.5 and tp([0.5], 96000) == 0.5 and tp([-0.5, 0.25, 0.125], 48000) >= 0.5
    assert mix.true_peak(np.zeros((2, 3, 0), dtype=np.float32), 48000).tolist() == [[0.0] * 3] * 2
    # a NaN or an Inf makes its own row NaN and no other
    y = np.random.default_rng(3).standard_normal((2, 2, 57)).astype(np.float32)
    clean = mix.true_peak(y, 48000)
    for bad in (np.nan, np.inf, -np.inf):
        z = y.copy()
        z[1, 0, 56] = bad
        got = mix.true_peak(z, 48000)
        assert math.isnan(got[1, 0]) and np.array_equal(np.delete(got.ravel(), 2), np.delete(clean.ravel(), 2))
    # the operations and their order: the loop written out in Python's own doubles
    row = y[0, 1].astype(np.float64).tolist()
    K, best = 13, 0.0
    for u in range(len(row) + K - 1):
        for p in range(4):
            acc = 0.0
            for k in range(K):
                tap = h[p + 4 * k] if p + 4 * k < 49 else 0.0
                acc = acc + tap * (row[u - k] if 0 <= u - k < len(row) else 0.0)
            best = max(best, abs(acc))
    assert clean[0, 1] == best
    with pytest.raises(ValueError, match=r"shape \(signals, channels, samples\)"):
        mix.true_peak(np.zeros((2, 5), dtype=np.float32), 48000)


# ---- the gain ---------------------------------------------------------------------------------------------------------------------------

def test_the_loudness_gain():
    one = np.float32(1.0)
    # the loudness limits: 3 dB down, far below the ceiling
    gain, level = mix.loudness_gain(-20.0, [[0.5, 0.25]], -23.0, -1.0)
    assert level == np.float32(10 ** (3 / 20)) and level.dtype == np.float32 and gain == 1.0 / float(np.float64(level))
    assert abs(-20.0 + 20 * math.log10(gain) + 23.0) < 1e-6 and 0.5 * gain < 10 ** (-1 / 20)
    # the ceiling limits: the largest true peak of ANY signal lands on it, one f32 step below at the most
    gain, level = mix.loudness_gain(-30.0, [[0.9, 0.2], [1.2, 0.1]], 0.0, -1.0)
    ceiling = 10 ** (-1 / 20)
    assert level == np.float32(1.2 / ceiling) and gain == 1.0 / float(np.float64(level))
    assert ceiling * (1 - 2.0 ** -23) <= 1.2 * gain <= ceiling * (1 + 2.0 ** -24)
    # unity: silence, a loudness or a true peak that is no number to scale by, a level that no f32 holds
    for lufs, tps in ((-math.inf, [0.5]), (math.nan, [0.5]), (-20.0, [0.0]), (-20.0, [0.5, math.nan]), (-20.0, [math.inf]), (-20.0, []), (1e9, [0.5]), (-1e9, [1e-300])):
        assert mix.loudness_gain(lufs, tps, -23.0, -1.0) == (1.0, one), (lufs, tps)
    assert mix.loudness_gain(-1000.0, [1e-40], -23.0, 0.0) == (1.0, one)  # (a level of 1e-40 is subnormal in f32: the samples stay as they are)
    assert mix.loudness_gain(-1000.0, [1e-30], -23.0, 0.0)[1] == np.float32(1e-30)  # (... and 1e-30 is a level like any other)
    # the gain is what the encoders apply to that level word
    for lufs, tps, target in ((-17.3, [0.8], -14.0), (-9.0, [1.4], -16.0), (-40.0, [0.01], -23.0)):
        gain, level = mix.loudness_gain(lufs, tps, target, -1.0)
        assert gain == 1.0 / float(np.float64(level)) == float(wav.gain(level, wav.NORMALISE_FULL))


@pytest.mark.parametrize("bit_depth", [16, 24, 32])
def test_encode_at_level_at_the_common_peak_is_encode_stems_to_full_scale(bit_depth):
    rng = np.random.default_rng(11)
    stack = (rng.standard_normal((4, 2, 301)) * np.array([0.3, 0.05, 1.7, 0.6])[:, None, None]).astype(np.float32)
    frames, peaks = wav.encode_stems(stack, bit_depth, wav.NORMALISE_FULL)
    got, got_peaks = wav.encode_at_level(stack, bit_depth, wav.common_peak(peaks))
    assert got.dtype == frames.dtype and got.tobytes() == frames.tobytes() and np.array_equal(got_peaks, peaks)
    # another level is another gain, and a level that is no magnitude leaves the samples as they are
    half, _ = wav.encode_at_level(stack, bit_depth, 2 * float(wav.common_peak(peaks)))
    assert half.tobytes() != frames.tobytes()
    for level in (0.0, math.nan, math.inf):
        assert wav.encode_at_level(stack, bit_depth, level)[0].tobytes() == wav.encode_stems(stack, bit_depth, wav.NORMALISE_NONE)[0].tobytes()
    with pytest.raises(wav.WavError):
        wav.encode_at_level(stack[0], bit_depth, 1.0)


# ---- the Python surface, without a device -----------------------------------------------------------------------------------------------

CALLS = (d.render_piece, d.render_score, d.render_piece_pcm, d.render_score_pcm, d.render_piece_wav, d.render_score_wav)
PCM_CALLS = CALLS[2:]


def voices(n=3):
    d.configure(sv.SAMPLE_RATE)
    return [sv.voice(k) for k in range(n)]


@pytest.mark.parametrize("call", CALLS, ids=lambda f: f.__name__)
def test_true_peak_that_is_no_bool_is_refused_by_string_next_to_meters(call):
    for value in (1, 0, None, "dBTP", 2.0):
        with pytest.raises(ValueError) as e:
            call(voices(), [0, 1, 2], 0.01, 0.05, true_peak=value, pans=[0])  # (the pans' shape would be refused next)
        assert str(e.value) == mix.TRUE_PEAK_NOT_BOOL
    with pytest.raises(ValueError) as e:
        call(voices(), [0, 1, 2], 0.01, 0.05, true_peak=1, meters=1)
    assert str(e.value) == mix.METERS_NOT_BOOL  # (meters first)
    assert mix.check_true_peak(True) is True and mix.check_true_peak(np.bool_(False)) is False


@pytest.mark.parametrize("call", PCM_CALLS, ids=lambda f: f.__name__)
def test_what_loudness_does_not_go_with_is_refused_by_string(call):
    for value in ("-16", True, math.nan, math.inf, [-16]):
        with pytest.raises(ValueError) as e:
            call(voices(), [0, 1, 2], 0.01, 0.05, 16, 0, loudness=value)
        assert str(e.value) == mix.LOUDNESS_NOT_NUMBER
    for value in (0.5, math.nan, -math.inf, None, "-1"):
        with pytest.raises(ValueError) as e:
            call(voices(), [0, 1, 2], 0.01, 0.05, 16, 0, loudness=-16, true_peak_max=value)
        assert str(e.value) == mix.TRUE_PEAK_MAX_BAD
    for normalise in (1, 2):
        with pytest.raises(ValueError) as e:
            call(voices(), [0, 1, 2], 0.01, 0.05, 24, normalise, loudness=-16)
        assert str(e.value) == mix.LOUDNESS_WITH_NORMALISE % normalise


def test_loudness_on_the_planar_calls_is_refused_by_string():
    for call in (d.render_piece, d.render_score):
        with pytest.raises(ValueError) as e:
            call(voices(), [0, 1, 2], 0.01, 0.05, loudness=-16)
        assert str(e.value) == mix.LOUDNESS_PLANAR
        with pytest.raises(TypeError):
            call(voices(), [0, 1, 2], 0.01, 0.05, true_peak_max=-1)  # (a ceiling belongs to a target)
    assert mix.check_loudness(None) == (None, -1.0) and mix.check_loudness(-16, -2, 0, True) == (-16.0, -2.0) and mix.check_loudness(np.float32(-23), 0)[0] == -23.0


def test_the_new_keywords_travel_with_the_placement_to_the_piece():
    d.configure(sv.SAMPLE_RATE)
    plain = render._placing(None, None, None, None, -3, None, False)
    assert plain["true_peak"] is False and plain["loudness"] is None and plain["true_peak_max"] == -1.0
    placing = render._placing(None, None, None, None, -3, None, False, stems=True, true_peak=True, loudness=-16, true_peak_max=-2)
    *_, place = render._piece(voices(), [0, 1, 2], 0.01, 0.05, None, None, placing)
    assert place.true_peak is True and place.loudness == -16 and place.true_peak_max == -2 and place.stems is True and place.meters is False
    assert not {"true_peak", "loudness", "true_peak_max"} & set(place.keywords())
    # a score with true peaks goes the piece's way, as one part
    with pytest.raises(d.DuspError, match="the voices of a score are isomorphic circuits"):
        d.render_score([sv.voice(0), mc.stereo_voice(1)], [0, 1], 0.01, 0, true_peak=True)
    with pytest.raises(d.DuspError, match="the voices of a score are isomorphic circuits"):
        d.render_score_pcm([sv.voice(0), mc.stereo_voice(1)], [0, 1], 0.01, 0, 16, 0, loudness=-16)


def test_a_timeline_of_no_samples_has_true_peaks_0_gain_1_and_frames_of_no_samples():
    with_tracks = dict(tracks=[mc.echo, None], track_of=[0, 1, -1], faders=[1, 0.5], buses=[mc.comb], track_sends=[[1, 0]])
    got = d.render_score(voices(), [0, 1, 2], 0.01, 0, stems=True, true_peak=True, **with_tracks)
    assert isinstance(got, render.Stems) and got.meters.names == got.names == mix.stem_names(2, 1)
    assert all(np.array_equal(got.meters.true_peak[name], [0.0]) and got.meters.lufs[name] == -math.inf for name in got.names)
    assert not hasattr(got, "level")
    one = d.render_piece_pcm(voices(), [0, 1, 2], 0.01, 0, 24, 0, loudness=-16)
    assert isinstance(one, render.Metered) and one.meters.names == ["mix"] and one.mix.data.shape == (0, 1, 3)
    assert one.gain == 1.0 and one.level == np.float32(1.0) and np.array_equal(one.meters.true_peak["mix"], [0.0]) and one.mix.peak == 0
    stems = d.render_piece_pcm(voices(), [0, 1, 2], 0.01, 0, 16, 0, stems=True, loudness=-23, true_peak_max=-2, **with_tracks)
    assert stems.gain == 1.0 and stems.level == np.float32(1.0) and stems.mix.data.shape == (0, 1) and stems.meters.names == stems.names
    files = d.render_piece_wav(voices(), [0, 1, 2], 0.01, 0, 16, 0, stems=True, loudness=-23, **with_tracks)
    assert files.gain == 1.0 and files.level == np.float32(1.0) and files.mix[:4] == b"RIFF" and files.meters.names == stems.names
    lone = d.render_score_wav(voices(), [0, 1, 2], 0.01, 0, 16, 0, loudness=-14)
    assert lone.mix[:4] == b"RIFF" and lone.gain == 1.0 and lone.level == np.float32(1.0)
    # without the new keywords a call hands back what it did
    assert not hasattr(d.render_score(voices(), [0, 1, 2], 0.01, 0, stems=True, meters=True, **with_tracks).meters, "true_peak")
    assert not hasattr(d.render_piece_pcm(voices(), [0, 1, 2], 0.01, 0, 24, 2, meters=True), "gain")
    # a rate below the meters' is refused in the meters' words
    d.configure(4000)
    try:
        with pytest.raises(ValueError) as e:
            d.render_piece([d.Osc(100 + k) for k in range(2)], [0, 1], 0.01, 0, true_peak=True)
        assert str(e.value) == mix.METER_RATE_LOW % 4000
    finally:
        d.configure(sv.SAMPLE_RATE)
    # render.true_peak of no samples needs no device call either way it is shaped
    assert mix.true_peak(np.zeros((1, 2, 0), np.float32), 8000).shape == (1, 2)


# ---- the kernel's text, under sanitizers ------------------------------------------------------------------------------------------------

def test_true_peak_kernel_text_on_the_host_under_sanitizers(tmp_path):
    """dusp_amd/csrc/truepeak_engine.hip itself, compiled for the host — the lanes of a workgroup as threads, LDS as statics,
    __syncthreads a barrier (tests/native/hip_host_stub_lds; the shuffle and the 64-bit atomicMax in the program itself) — every buffer
    a heap allocation of exactly its size, under AddressSanitizer and UBSan, bit for bit against the contract's loop
    (tests/native/truepeak_kernel_check.cpp lists what it covers).  A stand-alone program, run as a subprocess; nothing is loaded into
    Python under a sanitizer."""
    native = os.path.join(ROOT, "tests", "native")
    exe = str(tmp_path / "truepeak_kernel_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-pthread"] + SANITIZE + ["-w", "-I", os.path.join(native, "hip_host_stub_lds"), "-x", "c++",
                           os.path.join(native, "truepeak_kernel_check.cpp"), "-o", exe])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    out = p.stdout.decode()
    assert p.returncode == 0, out[-4000:]
    rep = json.loads(out.strip().splitlines()[-1])
    assert rep["bad"] == 0 and rep["cases"] > 800 and rep["groups"] > 2000 and rep["per_lane"] == 1 | 2 | 4 | 8, rep
