"""What the Space-placement tests share (tests/test_space_host.py, tests/test_gpu_space.py, tests/test_js_space.py): places and speakers
per voice count, the anchor circuit in the reference — ONE channel at a time — and planted mono rows with edge delays.

Where the reference anchors the contract (dusp_amd/mix.py score_chain_rows_placed), and where the anchor ends.  Channel
c of a placed piece is the oracle's render of the ONE-channel circuit

    Sum.many(k -> MonoDelay(Gain(Delay(Multiply(voice_k, g_k), onset_k, 8192), dB_kc), D_kc))        G_kc = pow(10, dB_kc / 20)

with the voice at onset 0 left without its Delay and a tap with D == 0 left without its MonoDelay (both units turn a 0 argument into
4410).  MonoDelay writes before it reads and wraps with %, so delays in (0, 1) and timelines longer than its ring are covered.  The
anchor ends in three places:
  * D_kc must be an f32: an inlet constant is rounded to f32 (space_taps gives f32 delays; elsewhere the contract is more exact);
  * with a whole delay the reference forms f32(f32(0 + y) + y * 0), which is y for every finite y up to the sign of a zero but NaN for
    +-Inf; the contract keeps y.  Planted rows with Inf are held to the contract, not to the oracle;
  * the reference's ConcatChannels ticks its second inlet one chunk late, so a stereo Space in the reference hears its
    right speaker 256 samples after its left.  That lag is not reproduced: the anchor is taken channel by channel, never through
    ConcatChannels."""
import functools
import math

import numpy as np

import dusp_amd as d
import score_voices as sv
from dusp_amd import mix
from pan_cases import planted as pan_planted

RING = 8192
SPEAKERS = {2: [[-1.0, 0.0], [1.0, 0.0]], 3: [[-1.0, 0.0], [1.0, 0.0], [0.0, 2.5]],
            6: [[-1.0, 1.0], [1.0, 1.0], [0.0, 1.5], [0.0, -1.0], [-1.5, -1.0], [1.5, -1.0]]}
SDPM = 128.0  # samples of delay a metre in the layouts: a place 2 m from a speaker is a WHOLE delay of 256 samples
EDGE_DELAYS = [0.0, 0.5, 2.0 ** -24, 1.0 - 2.0 ** -53, 255.0, 256.25, 1300.5]  # (1300.5: past a timeline of 1301 samples for all but its first)


@functools.lru_cache(maxsize=None)
def layout(n, n_speakers=2):
    """-> onsets int64 [n], gains float32 [n] (sv.layout's), places float32 [n, 2] within 3 m of the origin, speakers, and the taps of
    mix.space_taps at SDPM samples a metre: delays and tap gains float64 [n, C].  Voice 0 sits ON speaker 0 (delay 0, 0 dB); from two
    voices on, voice 1 sits 2 m above speaker 1 (a whole delay of 256 samples); the others have fractional delays up to ~700 samples."""
    onsets, _, gains = sv.layout(n)
    speakers = SPEAKERS[n_speakers]
    places = np.random.RandomState(300 + n).uniform(-3, 3, (n, 2)).astype(np.float32)
    places[0] = speakers[0]
    if n > 1:
        places[1] = [speakers[1][0], speakers[1][1] + 2.0]
    delays, tap_gains = mix.space_taps(places, speakers, sample_delay_per_metre=SDPM)
    assert delays[0, 0] == 0 and tap_gains[0, 0] == 1 and (n < 2 or delays[1, 1] == 256) and delays.max() < 800
    assert n < 3 or ((delays != np.floor(delays)).sum() >= delays.size - 4)
    assert np.array_equal(delays.astype(np.float32).astype(np.float64), delays), "a delay is an f32"
    for a in (places, delays, tap_gains):
        a.setflags(write=False)
    return onsets, gains, places, speakers, delays, tap_gains


def decibels(places, speakers, decibels_per_metre=-3):
    """the dB a SpaceChannel's attenuationScaler hands its Gain, per voice and speaker: f32(dist * dBpm), as floats (mix.space_taps' own
    intermediate, restated here so that the anchor circuit is built from numbers the test made itself)"""
    f32, f64 = np.float32, np.float64
    out = np.zeros((len(places), len(speakers)))
    for k, p in enumerate(np.asarray(places, dtype=f32)):
        for c, q in enumerate(np.asarray(speakers, dtype=f32)):
            dist = f32(math.sqrt(sum(float(f32(f64(a) - f64(b))) ** 2 for a, b in zip(p, q))))
            out[k, c] = float(f32(f64(dist) * f64(f32(decibels_per_metre))))
    return out


def anchor_circuit(voices, onsets, db, delays, channel, gains=None):
    """channel `channel` of the placed piece as ONE one-channel reference circuit (the module's docstring)"""
    units = []
    for k, v in enumerate(voices):
        if gains is not None:
            v = d.Multiply(v, float(gains[k]))
        if int(onsets[k]) != 0:
            v = d.Delay(v, int(onsets[k]), RING)
        g = d.Gain(float(db[k, channel]))
        g.IN = v
        v = g
        D = float(delays[k, channel])
        if D != 0:
            v = d.MonoDelay(v, int(D) if D == int(D) else D)
        units.append(v)
    return d.Sum.many(units)


def edge_taps(n, n_speakers):
    """-> delays, gains float64 [n, C]: EDGE_DELAYS in turn over voices and speakers (every voice meets whole and fractional taps); gains
    1, -0.75, 0.1 and 10^(-3 / 20) in turn; from two speakers on, voice 2 is 2000 samples late at speaker 1 alone: its span there lies
    wholly outside a timeline of 1301 samples while its other channels are inside"""
    delays = np.array([[EDGE_DELAYS[(k + 3 * c) % len(EDGE_DELAYS)] for c in range(n_speakers)] for k in range(n)], dtype=np.float64)
    gains = np.array([[[1.0, -0.75, 0.1, math.pow(10, -3 / 20)][(k + c) % 4] for c in range(n_speakers)] for k in range(n)], dtype=np.float64)
    if n > 2 and n_speakers > 1:
        delays[2, 1] = 2000.0
    for a in (delays, gains):
        a.setflags(write=False)
    return delays, gains


@functools.lru_cache(maxsize=None)
def planted(n, n_speakers, n_total=1301):
    """pan_cases.planted — mono rows of 773, 1, 255, 0, 257 and 3 samples in turn with -0, NaN, +-inf, subnormals and the largest f32 among
    them, onsets of both signs, lengths, gains — with edge_taps and an init of n_speakers channels (with -0, inf and NaN).
    -> rows, onsets, lengths, gains, delays, tap_gains, init"""
    rows, onsets, lengths, gains, _, init2 = pan_planted(n, n_total)
    delays, tap_gains = edge_taps(n, n_speakers)
    init = (30 * np.random.RandomState(8000 + n + n_speakers).standard_normal((n_speakers, n_total))).astype(np.float32)
    init[:min(2, n_speakers)] = init2[:min(2, n_speakers)]
    init[n_speakers - 1, 9] = np.nan
    init.setflags(write=False)
    return rows, onsets, lengths, gains, delays, tap_gains, init


__all__ = ["RING", "SPEAKERS", "SDPM", "EDGE_DELAYS", "layout", "decibels", "anchor_circuit", "edge_taps", "planted"]
