"""Sample t without walking there: an exact model of what the time-parallel paths compute deep in a timeline.  A helper module of the
tests (tests/test_deep_time_model.py pins it to the oracle on the CPU, tests/test_gpu_deep_time.py drives the kernels); plain Python
integers and numpy f64 on top of tests/edge_values.py, nothing from the library.

A constant f32 increment f in the exact regime (every `phase += f` of Osc.js:39 an exact f64 sum: f on the 2^-36 grid and the phases it
reaches representable) makes the phase after sample t the rational (phase0 + (t + 1) f) mod sampleRate.  Here that is an integer in units
of 2^-36 reduced mod sampleRate * 2^36 — Python integers for the jump to a window's first sample, int64 inside the window — and the
reference's lookup (Osc.js:43-45, three roundings) is run on it.  A triggered Ramp is t(n) = min(t0 + n + 1, duration) (Ramp.js:25-40).
A voice is lookup x envelope or gain, one f32 rounding (Multiply.js:31); a chain is left-deep f32 adds (Sum.js:18-29, 41); the outlet is
`x || 0` (renderChannelData.js:44) unless the window is a raw partial sum."""
import numpy as np

import edge_values as ev

CHUNK = ev.CHUNK
FRAC = 36
ONE = 1 << FRAC


def fixed(x):
    """x (a float on the 2^-36 grid) as an integer in units of 2^-36."""
    x = float(x)
    scaled = x * float(ONE)  # a power-of-two scaling: exact
    assert scaled == int(scaled) and abs(scaled) < 2.0 ** 62, ("not on the 2^-36 grid", x)
    return int(scaled)


def phase_units(f, sr, a, n, phase0=0.0):
    """Phases of samples [a, a + n) of an oscillator with the constant f32 increment f, as int64 in units of 2^-36, each in [0, sr 2^36)."""
    S = int(sr) << FRAC
    F = fixed(np.float32(f))
    P = np.empty(n, np.int64)
    if n == 0:
        return P
    P[0] = (fixed(phase0) + (int(a) + 1) * F) % S
    Fm = F % S
    have, step = 1, Fm  # step = have * F mod S
    while have < n:     # P[have : 2 have] = P[0 : have] + have F: every sum below 2^55
        m = min(have, n - have)
        P[have:have + m] = (P[:m] + step) % S
        have += m
        step = (step * 2) % S
    return P


def phases(f, sr, a, n, phase0=0.0):
    """... as the f64 the reference holds: exact, or f was not in the exact regime."""
    P = phase_units(f, sr, a, n, phase0)
    low = int(np.bitwise_or.reduce(P)) if n else 0
    assert low < (1 << 53) or low % (1 << (low.bit_length() - 53)) == 0, ("phases finer than f64 holds", f, sr)
    return P.astype(np.float64) / float(ONE)


def end_phase(f, sr, n_ticked, phase0=0.0):
    """The phase an oscillator holds after n_ticked samples (the reference ticks whole chunks)."""
    S = int(sr) << FRAC
    return ((fixed(phase0) + int(n_ticked) * fixed(np.float32(f))) % S) / float(ONE)


def osc_window(f, sr, a, n, waveform="sin", phase0=0.0):
    return ev.osc_lookup(phases(f, sr, a, n, phase0), ev.table(waveform, sr), sr)


def ramp_window(duration, y0, y1, a, n, t0=0.0):
    """A Ramp triggered at sample 0 of the timeline: samples [a, a + n).  t0 + n + 1 is exact in f64 far beyond any timeline here."""
    t = np.minimum(float(t0) + (np.arange(a, a + n, dtype=np.float64) + 1.0), float(duration))
    return ev.f32(float(y0) + (t / float(duration)) * (float(y1) - float(y0)))


def ramp_end(duration, n_ticked, t0=0.0):
    """[t, playing] after n_ticked samples."""
    return [min(float(t0) + float(n_ticked), float(duration)), 1.0 if float(t0) + float(n_ticked) <= float(duration) else 0.0]


# A voice: ("osc", f) | ("gain", f, k) | ("ramp", f, (duration, y0, y1)) — the fused shapes osc(k), mul(osc(k),k), mul(osc(k),ramp)
def voice_window(voice, sr, first, n, waveform="sin"):
    """One voice's samples [first, first + n) before the outlet."""
    x = osc_window(voice[1], sr, first, n, waveform)
    if voice[0] == "osc":
        return x
    if voice[0] == "gain":
        return ev.multiply(x, np.full(n, voice[2], np.float32))
    if voice[0] == "ramp":
        return ev.multiply(x, ramp_window(*voice[2], a=first, n=n))
    raise KeyError(voice[0])


def chain_window(voices, sr, first, n, init=None, raw=False, waveform="sin"):
    """Samples [first, first + n) of Sum.many(voices); init: the sums the voices in front of these left (a raw window); raw: no `x || 0`."""
    acc = None if init is None else np.asarray(init, np.float32)
    for v in voices:
        x = voice_window(v, sr, first, n, waveform)
        acc = x if acc is None else ev.add(acc, x)
    return acc if raw else ev.outlet(acc)


def whole_chunks(n):
    return -(-int(n) // CHUNK) * CHUNK
