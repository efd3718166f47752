"""Edge values for every signal inlet: the f32 set, the streams that carry it, a plain f64 model of each operation, and
the distance the comparisons use.  A helper module of the tests (tests/test_edge_model.py pins the model to the oracle
on the CPU, tests/test_gpu_edge_values.py drives the engines); nothing here touches a device.

The model restates the reference's `_tick` of each unit (file:line under src/ in the comments, as oracle/dusp_oracle.c
does) in Python floats / numpy f64 — JS evaluates every sub-expression as a separately rounded f64 operation — with ONE
np.float32 rounding where JS stores into the Float32Array chunk.  numpy's f64 +, -, *, /, sqrt, floor, ceil and fmod are
IEEE-exact; pow is the host libm's, called through ctypes (numpy's own pow need not be libm's)."""
import ctypes
import ctypes.util
import math

import numpy as np

CHUNK = 256
F32_MAX = float(np.finfo(np.float32).max)
F32_MIN = float(np.finfo(np.float32).tiny)  # FLT_MIN, the smallest normal


def f32(x):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(x, dtype=np.float64).astype(np.float32)


def _next(x, toward):
    return float(np.nextafter(np.float32(x), np.float32(toward)))


def edge(sr):
    """The f32 edge set at sample rate sr (the members around sr move with it)."""
    just_below = _next(2.0 ** -13, 0.0)
    v = [0.0, -0.0,
         1e-45, -1e-45, 1e-40, -1e-40, F32_MIN, -F32_MIN,           # subnormals (1e-45 rounds to the smallest one) and FLT_MIN
         2.0 ** -13, -2.0 ** -13, just_below, -just_below,           # the oscillators' exactness bound (SURVEY.md §8a note ii)
         0.5, -0.5, 1.0, -1.0, _next(1.0, 0.0), _next(1.0, 2.0),
         2.0, -2.0, 3.0, -3.0, 20.0, 69.0, -127.5, 128.25,
         sr - 0.5, _next(sr, 0.0), float(sr), _next(sr, math.inf), -float(sr),
         65536.0, 131072.375, float(np.float32(3e5 + 0.37)), 1e6, 1e9, 2.0 ** 40, 1e18, -1e18, 1e19, F32_MAX, -F32_MAX,
         math.inf, -math.inf, math.nan]
    return f32(v)


EDGE = edge(48000)

# samples at which single values are planted: a lane of the wave engines owns samples 4l..4l+3 and a chunk is 256 samples, so
# these are the first / last sample of a lane, of a chunk and of a wavefront's scan, both sides of two chunk boundaries, and one
# sample in a later chunk
PLANT_POSITIONS = (0, 1, 3, 4, 251, 252, 255, 256, 257, 511, 512, 5 * CHUNK + 77)


def mild(n, seed, lo=-1.0, hi=1.0):
    """A seeded uniform carrier, f32."""
    return np.random.RandomState(seed).uniform(lo, hi, n).astype(np.float32)


def pairs(E):
    """Two streams that walk every ordered pair of E, padded (with 0.5 / 0.25) to whole chunks, then the same walk rotated by 1, 2
    and 3 samples: every pair meets every position within a lane."""
    E = f32(E)
    a, b = np.repeat(E, len(E)), np.tile(E, len(E))
    pad = -len(a) % CHUNK
    a = np.concatenate([a, np.full(pad, 0.5, np.float32)])
    b = np.concatenate([b, np.full(pad, 0.25, np.float32)])
    return (np.concatenate([np.roll(a, r) for r in range(4)]), np.concatenate([np.roll(b, r) for r in range(4)]))


def planted(carrier, positions, values):
    """The carrier with values[k] at sample positions[k]."""
    out = np.array(carrier, dtype=np.float32, copy=True)
    for p, v in zip(positions, values):
        out[p] = np.float32(v)
    return out


WALK_SEED = 20240613


def walk(E, k, n, seed=WALK_SEED):
    """k streams of n samples: a seeded sample of k-tuples of E (CrossFader: k = 3, Rescale: k = 5)."""
    E = f32(E)
    return E[np.random.RandomState(seed + k).randint(0, len(E), (k, n))]


def batch(streams, n, fill=0.25):
    """[k, total] (or a list of equally long streams) -> [k, V, n]: the streams cut into V instances of n samples, the last one
    filled up."""
    s = np.atleast_2d(np.asarray(streams, dtype=np.float32))
    v = -(-s.shape[1] // n)
    out = np.full((s.shape[0], v * n), fill, np.float32)
    out[:, :s.shape[1]] = s
    return np.ascontiguousarray(out.reshape(s.shape[0], v, n))


# --------------------------------------------------------------------------- distance
def _ordered(x):
    """f32 bit patterns on a line: -Inf < ... < -0 = +0 < ... < +Inf, neighbours one apart."""
    i = np.ascontiguousarray(x, dtype=np.float32).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7FFFFFFF), i)


def ulp_distance(a, b):
    """Steps between a and b on the ordered-integer image of the f32 bit patterns (FLT_MAX to Inf is one step, -0 to +0 none).
    NaN matches only NaN: distance 0 to a NaN, 2^40 to anything else."""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    d = np.abs(_ordered(np.where(na, 0, a)) - _ordered(np.where(nb, 0, b)))
    return np.where(na & nb, 0, np.where(na | nb, 1 << 40, d))


def same_bits(a, b):
    """Bit-equal f32 arrays, any NaN equal to any NaN (the engines and JS agree on where NaN sits, not on its payload)."""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return a.shape == b.shape and bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


# --------------------------------------------------------------------------- the model
_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.pow.restype = ctypes.c_double
_libm.pow.argtypes = [ctypes.c_double, ctypes.c_double]


def js_pow(x, y):
    """Math.pow (ECMA-262 Number::exponentiate) = C pow with two deviations: an exponent of NaN gives NaN even for base 1
    (C: pow(1, NaN) = 1), and a base of +-1 with an exponent of +-Inf gives NaN (C: 1)."""
    x, y = float(x), float(y)
    if y != y:
        return math.nan
    if abs(x) == 1.0 and math.isinf(y):
        return math.nan
    return _libm.pow(x, y)


_vpow = np.frompyfunc(js_pow, 2, 1)


def _pow(x, y):
    x, y = np.broadcast_arrays(np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64))
    with np.errstate(all="ignore"):
        return _vpow(x, y).astype(np.float64)


def outlet(x):
    """renderChannelData.js:44 `chunk.channelData[channel][t] || 0`: NaN and -0 leave as +0."""
    x = np.asarray(x, dtype=np.float32)
    return np.where(np.isnan(x) | (x == 0), np.float32(0), x)


def _d(x):
    return np.asarray(x, dtype=np.float32).astype(np.float64)


# The thirteen two-operand maps (map_ops.hpp map_apply).  a, b: f32 arrays; k: the unit's plain-number attribute (FixedMultiply's sf;
# SecondsToSamples' sample rate).
def m_subtract(a, b, k=None):                                                # Subtract.js:26
    with np.errstate(invalid="ignore", over="ignore"):
        return f32(_d(a) - _d(b))
def m_divide(a, b, k=None):                                                  # Divide.js:21
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        return f32(_d(a) / _d(b))
def m_pow(a, b, k=None): return f32(_pow(_d(a), _d(b)))                      # Pow.js:27
def m_polarity_invert(a, b=None, k=None): return -np.asarray(a, np.float32)  # PolarityInvert.js:15
def m_abs(a, b=None, k=None): return f32(np.abs(_d(a)))                      # Abs.js:19
def m_decibel_to_scaler(a, b=None, k=None): return f32(_pow(10.0, _d(a) / 20.0))   # DecibelToScaler.js:16
def m_semitone_to_ratio(a, b=None, k=None): return f32(_pow(2.0, _d(a) / 12.0))    # SemitoneToRatio.js:16
def m_scale(a, b=None, k=1.0):                                               # SecondsToSamples.js:19, FixedMultiply.js:20
    with np.errstate(over="ignore", invalid="ignore"):
        return f32(_d(a) * float(k))
def m_clip(a, b, k=None):                                                    # Clip.js:18-19
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.where(np.abs(_d(a)) > np.abs(_d(b)), b, a)
def m_hard_clip_above(a, b, k=None):                                         # HardClipAbove.js:18-22
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.where(a > b, b, a)
def m_hard_clip_below(a, b, k=None):                                         # HardClipBelow.js:18-22
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.where(a < b, b, a)
def m_gain(a, b, k=None):                                                    # Gain.js:22,26-28: dB(gain[t]) * in[c][t]
    with np.errstate(over="ignore", invalid="ignore"):
        return f32(_pow(10.0, _d(b) / 20.0) * _d(a))


# The five wider maps (map_ops.hpp map_wide)
def w_pan(x, pan, comp_db=1.5):                                              # Pan.js:19-23 -> [2, n]
    x, p = _d(x), _d(pan)
    with np.errstate(over="ignore", invalid="ignore"):
        comp = _pow(10.0, ((1 - np.abs(p)) * comp_db) / 20.0)
        return np.stack([f32(x * (1 - p) / 2 * comp), f32(x * (1 + p) / 2 * comp)])
def w_midi_to_frequency(m):                                                  # MidiToFrequency.js:20
    with np.errstate(over="ignore", invalid="ignore"):
        return f32(_pow(2.0, (_d(m) - 69) / 12.0) * 440)
def w_rescale(x, il, iu, ol, ou):                                            # Rescale.js:33-34
    x, il, iu, ol, ou = (_d(v) for v in (x, il, iu, ol, ou))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        return f32((x - il) / (iu - il) * (ou - ol) + ol)
def w_cross_fader(a, b, dial):                                               # CrossFader.js:26
    a, b, dial = _d(a), _d(b), _d(dial)
    with np.errstate(invalid="ignore", over="ignore"):
        return f32((1 - dial) * a + dial * b)
def w_vector_magnitude(channels):                                            # VectorMagnitude.js:17-29
    with np.errstate(invalid="ignore", over="ignore"):
        s = np.zeros(np.asarray(channels[0]).shape, np.float64)
        for c in channels:
            s = s + _d(c) * _d(c)
        return f32(np.sqrt(s))


def multiply(a, b):                                                          # Multiply.js:31
    with np.errstate(invalid="ignore", over="ignore"):
        return f32(_d(a) * _d(b))
def add(a, b):                                                               # Sum.js:41
    with np.errstate(invalid="ignore", over="ignore"):
        return f32(_d(a) + _d(b))


def pick_channel(channels, c):
    """PickChannel.js:19 `this.in[this.c[t] % this.in.length][t]`.  An index that is not one of 0..n-1 (a fraction, a negative,
    NaN, Inf % n = NaN) makes the reference throw a TypeError in mid-render; oracle and engines give NaN there."""
    n = len(channels)
    with np.errstate(invalid="ignore"):
        k = np.fmod(_d(c), float(n))
    ok = (k >= 0) & (k < n) & (k == np.floor(k))
    idx = np.where(ok, k, 0).astype(np.int64)
    return np.where(ok, np.stack(channels)[idx, np.arange(len(idx))], np.float32(np.nan)).astype(np.float32)


def sample_rate_redux(x, amount, tslu=math.inf, val=0.0):
    """SampleRateRedux.js:20-36, one channel: -> (out, timeSinceLastUpdate, val).  `tslu > amount` is false for NaN."""
    x, amount = np.asarray(x, np.float32), _d(amount)
    out = np.empty(len(x), np.float32)
    val = np.float32(val)
    for t in range(len(x)):
        tslu += 1
        if tslu > amount[t]:
            val = x[t]
            tslu = 0
        out[t] = val
    return out, tslu, val


def delay(x, d, max_delay, clock0=0):
    """Delay.js:20-41, one channel.  Typed-array stores at an index that is out of range, negative or NaN are dropped (no wrap at
    ceil(tWrite) == length); Math.ceil of a tWrite in (-1, 0) is -0, which indexes slot 0."""
    x, d = _d(x), _d(d)
    buf = np.zeros(max_delay, np.float32)
    out = np.empty(len(x), np.float32)
    L = float(max_delay)
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(len(x)):
            tb = (clock0 + t) % max_delay
            out[t] = buf[tb]
            buf[tb] = 0
            tw = math.fmod(tb + d[t], L) if math.isfinite(d[t]) else math.nan
            if tw != tw:
                continue
            lo, hi, frac = math.floor(tw), math.ceil(tw), math.fmod(tw, 1.0)
            if 0 <= lo < max_delay:
                buf[lo] = np.float32(float(buf[lo]) + x[t] * (1 - frac))
            if 0 <= hi < max_delay:
                buf[hi] = np.float32(float(buf[hi]) + x[t] * frac)
    return out


def ramp(duration, y0, y1, n, t=0.0, playing=True):
    """Ramp.js:25-40."""
    out = np.empty(n, np.float32)
    for i in range(n):
        if playing:
            t += 1
            if t > duration:
                playing, t = False, duration
            if t < 0:
                playing, t = False, 0
        out[i] = np.float32(y0 + (t / duration) * (y1 - y0))
    return out


def osc_phases(f, sr, phase=0.0, multi=False):
    """The sequential phase loop: Osc.js:39-42 `phase += f[t]; phase %= sampleRate; if(phase < 0) phase += sampleRate`, and
    MultiChannelOsc.js:23,31-32 (no `phase < 0` fix-up; `phase || 0` at the start of every chunk, which also clears a NaN).
    -> the f64 phase of every sample."""
    f = _d(f)
    srd = float(sr)
    out = np.empty(len(f), np.float64)
    for t in range(len(f)):
        if multi and t % CHUNK == 0 and (phase != phase or phase == 0):
            phase = 0.0
        phase = phase + f[t]
        phase = math.fmod(phase, srd) if math.isfinite(phase) else math.nan
        if not multi and phase < 0:
            phase += srd
        out[t] = phase
    return out


def osc_phases_modular(f, sr, phase=0.0):
    """What the parallel engines computed before they knew the second bound — the identity (a + b) % m == (a + b % m) % m on
    exact 2^-36 fixed point, true of real numbers but not of the reference's rounded f64 sum once |phase + f| >= 2^17.  Kept so
    that the CPU suite can show the oscillator tests telling the two apart (tests/test_edge_model.py)."""
    S = int(sr) << 36
    P = int(phase * 2.0 ** 36)
    out = np.empty(len(f), np.float64)
    dead = False
    for t, v in enumerate(_d(f)):
        if not math.isfinite(v):
            dead = True
        if dead:
            out[t] = math.nan
            continue
        if abs(v) >= sr:
            v = math.fmod(v, float(sr))
        P = (P + int(v * 2.0 ** 36)) % S
        out[t] = P / 2.0 ** 36
    return out


def osc_lookup(phases, table, sr):
    """Osc.js:43-45: waveTable[floor(phase)] * (1 - phase % 1) + waveTable[ceil(phase)] * (phase % 1); an index outside the table
    (or NaN) reads undefined, which makes the sample NaN."""
    p = np.asarray(phases, np.float64)
    with np.errstate(invalid="ignore"):
        frac = np.fmod(p, 1.0)
        lo, hi = np.floor(p), np.ceil(p)
        ok_lo, ok_hi = (lo >= 0) & (lo <= sr), (hi >= 0) & (hi <= sr)
        t = np.asarray(table, np.float32).astype(np.float64)
        a = np.where(ok_lo, t[np.where(ok_lo, lo, 0).astype(np.int64)], np.nan)
        b = np.where(ok_hi, t[np.where(ok_hi, hi, 0).astype(np.int64)], np.nan)
        return f32(a * (1 - frac) + b * frac)


_tables = {}


def table(waveform, sr):
    """The oscillator table as the product computes it (dusp_amd/wavetables.py, pinned to the reference's hashes elsewhere)."""
    from dusp_amd import wavetables
    key = (waveform, sr)
    if key not in _tables:
        _tables[key] = wavetables.make_table(wavetables.WAVEFORMS[waveform], sr)
    return _tables[key]


def osc(f, waveform, sr, phase=0.0, multi=False):
    """-> (chunk output before the outlet's `|| 0`, phase after the last sample)."""
    ph = osc_phases(f, sr, phase, multi)
    return osc_lookup(ph, table(waveform, sr), sr), (ph[-1] if len(ph) else phase)


# --------------------------------------------------------------------------- circuits: what both test files render
# Every case is a descriptor, its streams / parameter columns, and the model's output for it.  tests/test_edge_model.py renders the
# cases on the oracle (CPU), tests/test_gpu_edge_values.py on the engines.
STREAM_N = 9 * CHUNK + 37       # samples per instance of a stream case: nine chunks and a ragged tail
GRID_N = 2 * CHUNK + 5          # ... of a parameter grid
POW_FAMILY = ("Pow", "DecibelToScaler", "SemitoneToRatio", "Gain", "MidiToFrequency", "Pan")
FIXED_SF = -2.5                 # FixedMultiply's plain-number factor


def _set_in(unit, x):
    unit.IN = x
    return unit


def _map_units():
    import dusp_amd as d
    # name -> (number of operands, circuit from operands, model from f32 arrays -> [channels][n])
    return {
        "Subtract": (2, lambda a, b: d.Subtract(a, b), lambda sr, a, b: [m_subtract(a, b)]),
        "Divide": (2, lambda a, b: d.Divide(a, b), lambda sr, a, b: [m_divide(a, b)]),
        "Pow": (2, lambda a, b: d.Pow(a, b), lambda sr, a, b: [m_pow(a, b)]),
        "PolarityInvert": (1, lambda a: d.PolarityInvert(a), lambda sr, a: [m_polarity_invert(a)]),
        "Abs": (1, lambda a: d.Abs(a), lambda sr, a: [m_abs(a)]),
        "DecibelToScaler": (1, lambda a: d.DecibelToScaler(a), lambda sr, a: [m_decibel_to_scaler(a)]),
        "SemitoneToRatio": (1, lambda a: d.SemitoneToRatio(a), lambda sr, a: [m_semitone_to_ratio(a)]),
        "SecondsToSamples": (1, lambda a: _set_in(d.SecondsToSamples(), a), lambda sr, a: [m_scale(a, k=sr)]),
        "FixedMultiply": (1, lambda a: d.FixedMultiply(FIXED_SF, a), lambda sr, a: [m_scale(a, k=FIXED_SF)]),
        "Clip": (2, lambda a, b: _set_in(d.Clip(b), a), lambda sr, a, b: [m_clip(a, b)]),
        "HardClipAbove": (2, lambda a, b: d.HardClipAbove(a, b), lambda sr, a, b: [m_hard_clip_above(a, b)]),
        "HardClipBelow": (2, lambda a, b: d.HardClipBelow(a, b), lambda sr, a, b: [m_hard_clip_below(a, b)]),
        "Gain": (2, lambda a, b: _set_in(d.Gain(b), a), lambda sr, a, b: [m_gain(a, b)]),
        "Pan": (2, lambda a, b: d.Pan(a, b), lambda sr, a, b: list(w_pan(a, b))),
        "MidiToFrequency": (1, lambda a: d.MidiToFrequency(a), lambda sr, a: [w_midi_to_frequency(a)]),
        "Rescale": (5, lambda x, il, iu, ol, ou: _set_in(d.Rescale(il, iu, ol, ou), x), lambda sr, *v: [w_rescale(*v)]),
        "CrossFader": (3, lambda a, b, dial: d.CrossFader(a, b, dial), lambda sr, a, b, dial: [w_cross_fader(a, b, dial)]),
        "VectorMagnitude": (2, lambda a, b: _set_in(d.VectorMagnitude(), d.ConcatChannels(a, b) if getattr(a, "isUnit", False) else [a, b]),
                            lambda sr, a, b: [w_vector_magnitude([a, b])]),
        "Multiply": (2, lambda a, b: d.Multiply(a, b), lambda sr, a, b: [multiply(a, b)]),
        "Sum": (2, lambda a, b: d.Sum(a, b), lambda sr, a, b: [add(a, b)]),
    }


MAP_NAMES = ["Subtract", "Divide", "Pow", "PolarityInvert", "Abs", "DecibelToScaler", "SemitoneToRatio", "SecondsToSamples", "FixedMultiply",
             "Clip", "HardClipAbove", "HardClipBelow", "Gain", "Pan", "MidiToFrequency", "Rescale", "CrossFader", "VectorMagnitude"]


class Case:
    """words: the descriptor; inputs: f32 [n_streams, n_inst, n] or None; params: f32 [n_params, n_inst] or None;
    model: f32 [n_inst, channels, n] as the outlet delivers it; pow: a pow-family unit is in it; behind: the unit under test feeds
    Divide(1, .) — `raw` is then the model's output of the unit itself, [n_inst, channels, n]."""

    def __init__(self, name, words, n, n_inst, model, inputs=None, params=None, pow=False, behind=False, raw=None, sr=48000):
        self.name, self.words, self.n, self.n_inst, self.model = name, words, n, n_inst, model
        self.inputs, self.params, self.pow, self.behind, self.raw, self.sr = inputs, params, pow, behind, raw, sr


def _streams_for(arity):
    if arity <= 2:
        return np.stack(pairs(EDGE))[:arity]
    return walk(EDGE, arity, 16 * CHUNK)  # (seed WALK_SEED + arity)


_case_cache = {}


def map_stream_case(name, behind, sr=48000):
    """Unit(HostSource a, HostSource b, ...) over pairs(EDGE) (three and five operands: the seeded walk), cut into instances of
    STREAM_N samples; behind: rendered through Divide(1, .), which tells -0 (-> -Inf), +0 (-> +Inf) and NaN (-> 0 at the outlet)
    apart where the bare outlet's `|| 0` shows +0 for all three."""
    key = ("stream", name, behind, sr)
    if key in _case_cache:
        return _case_cache[key]
    import dusp_amd as d
    from dusp_amd import descriptor
    d.configure(sr)
    arity, build, model = _map_units()[name]
    x = batch(_streams_for(arity), STREAM_N)  # [arity, V, n]
    unit = build(*[d.HostSource(x[k, 0]) for k in range(arity)])
    ex = descriptor.extract(d.Divide(1, unit) if behind else unit)
    assert len(ex.sources) == arity
    flat = [x[k].reshape(-1) for k in range(arity)]
    raw = np.stack([np.asarray(c, np.float32).reshape(x.shape[1], STREAM_N) for c in model(sr, *flat)], axis=1)
    out = m_divide(np.ones_like(raw), raw) if behind else raw
    c = Case("%s%s" % (name, "_behind_divide" if behind else ""), ex.words, STREAM_N, x.shape[1], outlet(out), inputs=x,
             pow=name in POW_FAMILY, behind=behind, raw=raw, sr=sr)
    _case_cache[key] = c
    return c


def map_grid_case(name, behind, sr=48000):
    """Unit(a_k, b_k) as ONE program whose operands are per-instance parameters, over the EDGE x EDGE grid (one operand: EDGE; three
    and five: the first two operands over the grid, the others at the unit's defaults)."""
    key = ("grid", name, behind, sr)
    if key in _case_cache:
        return _case_cache[key]
    import dusp_amd as d
    from dusp_amd import descriptor
    d.configure(sr)
    arity, build, model = _map_units()[name]
    rest = {"Rescale": [1.0, 0.0, 1.0], "CrossFader": [0.25]}.get(name, [])  # (Rescale: inUpper, outLower, outUpper; CrossFader: dial)
    if name == "CrossFader":  # the grid goes over a and dial; b is the constant
        make = lambda a, b: build(a, 0.75, b)  # noqa: E731
        mdl = lambda a, b: model(sr, a, np.full_like(a, 0.75), b)  # noqa: E731
        live = 2
    elif name == "Rescale":
        make = lambda a, b: build(a, b, *rest)  # noqa: E731
        mdl = lambda a, b: model(sr, a, b, *[np.full_like(a, v) for v in rest])  # noqa: E731
        live = 2
    else:
        make, mdl, live = build, (lambda *v: model(sr, *v)), arity
    # structure from three circuits whose constants all differ; the columns are then written directly
    seeds = [[10.0 + 16 * k + j for k in range(live)] for j in range(3)]
    exs = []
    for s in seeds:
        unit = make(*s)
        exs.append(descriptor.extract(d.Divide(1, unit) if behind else unit))
    uni = descriptor.unify(exs)
    assert uni.n_params == live, (name, uni.n_params)
    cols = [np.repeat(EDGE, len(EDGE)), np.tile(EDGE, len(EDGE))] if live == 2 else [EDGE.copy()]
    order = [int(round((float(uni.params[p, 0]) - 10.0) / 16)) for p in range(live)]  # which operand each column is
    assert sorted(order) == list(range(live)), order
    params = np.ascontiguousarray(np.stack([cols[k] for k in order]).astype(np.float32))
    v = params.shape[1]
    raw = np.stack([np.repeat(np.asarray(c, np.float32)[:, None], GRID_N, axis=1) for c in mdl(*cols)], axis=1)
    out = m_divide(np.ones_like(raw), raw) if behind else raw
    c = Case("%s_grid%s" % (name, "_behind_divide" if behind else ""), uni.words, GRID_N, v, outlet(out), params=params,
             pow=name in POW_FAMILY, behind=behind, raw=raw, sr=sr)
    _case_cache[key] = c
    return c


# ---- oscillators
def fold_values(sr):
    return f32([sr, -sr, _next(sr, math.inf), 65536.0, 131072.375, float(np.float32(3e5 + 0.37)), 1e6, 1e9, 2.0 ** 40, 1e18, -1e18,
                F32_MAX, -F32_MAX])


MILD_INCREMENTS = (0.37, 440.5, -3.25)
TINY_INCREMENTS = (1e-30, 1e-45, 3e-5)


def folding_streams(sr):
    """[V, STREAM_N]: constant mild increments with single large values planted.  Instance i of a carrier plants value (i + j) mod 13
    at PLANT_POSITIONS[j], so every value meets every position; then two and three values inside one chunk, and one in each of
    two neighbouring chunks."""
    vals = fold_values(sr)
    rows = []
    for inc in MILD_INCREMENTS:
        carrier = np.full(STREAM_N, inc, np.float32)
        for i in range(len(vals)):
            rows.append(planted(carrier, PLANT_POSITIONS, [vals[(i + j) % len(vals)] for j in range(len(PLANT_POSITIONS))]))
        rows.append(planted(carrier, (3 * CHUNK + 100, 3 * CHUNK + 101), (vals[9], vals[4])))                       # two in one chunk
        rows.append(planted(carrier, (2 * CHUNK + 7, 2 * CHUNK + 130, 2 * CHUNK + 255), (vals[8], vals[10], vals[5])))  # three
        rows.append(planted(carrier, (4 * CHUNK - 1, 4 * CHUNK), (vals[11], vals[9])))                              # neighbouring chunks
        rows.append(planted(carrier, (6 * CHUNK + 10, 7 * CHUNK + 200), (vals[6], vals[12])))
    return np.stack(rows)


def poison_streams(sr):
    """[V, STREAM_N] and the plant position of every instance: a finite stream with NaN, +Inf or -Inf at one position."""
    carrier = planted(np.full(STREAM_N, 440.5, np.float32), (40, 700), (-3.25, 0.37))
    rows, at = [], []
    for bad in (math.nan, math.inf, -math.inf):
        for p in PLANT_POSITIONS:
            rows.append(planted(carrier, (p,), (bad,)))
            at.append(p)
    return np.stack(rows), at


def tiny_streams(sr):
    """[V, STREAM_N]: increments with 0 < |f| < 2^-13, where the reference's own f64 sum rounds (tolerance-level on the parallel
    engines): a 440.5 carrier (full-scale output) with the tiny value at the plant positions and as a run of 300 samples."""
    rows = []
    for tiny in TINY_INCREMENTS:
        s = planted(np.full(STREAM_N, 440.5, np.float32), PLANT_POSITIONS, [tiny] * len(PLANT_POSITIONS))
        s[600:900] = np.float32(tiny)
        rows.append(s)
        rows.append(-s)
    return np.stack(rows)


OSC_WAVEFORMS = ("sin", "saw", "8bit")  # sin: the LDS image; saw: gathered from L2 by the interpreter kernel, a closed form in compiled ones;
#                                         8bit: derived from the image.  MultiChannelOsc gathers every table from L2.


def is_tiny(f):
    a = np.abs(np.asarray(f, np.float64))
    return (a > 0) & (a < 2.0 ** -13)


def osc_stream_case(kind, waveform, multi, sr):
    """Osc(HostSource f, waveform) / MultiChannelOsc(...) over the folding, poison or tiny streams, one instance per stream.
    -> Case with .phase: the model's written-back phase of every instance (after the last whole chunk; the streams end in zeros)."""
    key = ("osc", kind, waveform, multi, sr)
    if key in _case_cache:
        return _case_cache[key]
    import dusp_amd as d
    from dusp_amd import descriptor
    d.configure(sr)
    streams = {"folding": folding_streams, "tiny": tiny_streams, "poison": lambda s: poison_streams(s)[0]}[kind](sr)
    src = d.HostSource(streams[0])
    ex = descriptor.extract((d.MultiChannelOsc if multi else d.Osc)(src, waveform))
    whole = -(-STREAM_N // CHUNK) * CHUNK
    outs, phases = [], []
    for s in streams:
        out, ph = osc(np.concatenate([s, np.zeros(whole - STREAM_N, np.float32)]), waveform, sr, multi=multi)
        outs.append(out[:STREAM_N])
        phases.append(ph)
    c = Case("%s_%s_%s_sr%d" % ("multiosc" if multi else "osc", kind, waveform, sr), ex.words, STREAM_N, len(streams),
             outlet(np.stack(outs))[:, None, :], inputs=streams[None], sr=sr)
    c.phase = np.array(phases)
    c.osc_unit = [type(u).__name__ for u in ex.circuit.units].index("MultiChannelOsc" if multi else "Osc")
    c.streams = streams
    _case_cache[key] = c
    return c


RAMP = (4000, 1, 0)
GAIN = 0.625                       # Multiply(Osc, k): the fused engine's gain shape
SHAPE = ("decay", 0.04, 0.25, 1)   # Multiply(Osc, Shape): 25 table steps a sample, past the table's end after 1920 samples


def shape(name, duration, lo, hi, n, sr, t=0.0):
    """Shape/index.js:28-59, triggered, constant inlets, the default edges (left 0, right "shape")."""
    from dusp_amd import wavetables
    data = wavetables.make_table(wavetables.SHAPES[name], sr).astype(np.float64)
    step = 1 / float(np.float32(duration))
    lo, hi = float(np.float32(lo)), float(np.float32(hi))
    out = np.empty(n, np.float32)
    for i in range(n):
        t += step
        if t <= 0:
            v = 0 * (hi - lo) + lo
        elif t > sr:
            v = data[sr] * (hi - lo) + lo
        else:
            frac = math.fmod(t, 1)
            v = lo + (hi - lo) * (data[math.ceil(t)] * frac + data[math.floor(t)] * (1 - frac))
        out[i] = np.float32(v)
    return out


def osc_constant_case(with_ramp, sr, waveform="sin"):
    """Osc(f_k) — or the fused engine's voice shape Multiply(Osc(f_k), Ramp) — as one batch with f over EDGE."""
    key = ("oscconst", with_ramp, sr, waveform)
    if key in _case_cache:
        return _case_cache[key]
    import dusp_amd as d
    from dusp_amd import descriptor
    d.configure(sr)
    E = edge(sr)

    def voice(f):
        o = d.Osc(f, waveform)
        if with_ramp == "gain":
            return d.Multiply(o, GAIN)
        if with_ramp == "shape":
            return d.Multiply(o, d.Shape(*SHAPE).trigger())
        return d.Multiply(o, d.Ramp(*RAMP).trigger()) if with_ramp else o
    exs = [descriptor.extract(voice(f)) for f in (100.0, 200.0, 300.0)]
    uni = descriptor.unify(exs)
    assert uni.n_params == 1
    params = np.ascontiguousarray(E[None, :])
    whole = -(-STREAM_N // CHUNK) * CHUNK
    env = (np.full(STREAM_N, GAIN, np.float32) if with_ramp == "gain" else shape(*SHAPE, n=STREAM_N, sr=sr) if with_ramp == "shape"
           else ramp(*RAMP, n=STREAM_N))
    outs, phases = [], []
    for f in E:
        out, ph = osc(np.full(whole, f, np.float32), waveform, sr)
        outs.append(multiply(out[:STREAM_N], env) if with_ramp else out[:STREAM_N])
        phases.append(ph)
    c = Case("osc_constant%s_%s_sr%d" % ("_" + with_ramp if isinstance(with_ramp, str) else "_ramp" if with_ramp else "", waveform, sr), uni.words, STREAM_N, len(E), outlet(np.stack(outs))[:, None, :],
             params=params, sr=sr)
    c.phase = np.array(phases)
    c.osc_unit = [type(u).__name__ for u in exs[0].circuit.units].index("Osc")
    c.f = E
    _case_cache[key] = c
    return c


# ---- the other stateful inlets
def delay_case(max_delay, sr=48000):
    """Delay(HostSource x, HostSource d, maxDelay): a mild input, delay times from a mild carrier with edge values planted —
    one instance per planted value (at every plant position), plus one with all of them in turn."""
    key = ("delay", max_delay, sr)
    if key in _case_cache:
        return _case_cache[key]
    import dusp_amd as d
    from dusp_amd import descriptor
    d.configure(sr)
    L = float(max_delay)
    vals = f32([-7.5, -L - 3.25, math.nan, math.inf, -math.inf, L, L - 0.5, 2 * L + 0.25, 1e18, -0.0, 0.625, 3e-5])
    x = mild(STREAM_N, 11)
    carrier = mild(STREAM_N, 12, 1.0, L - 1.0)
    carrier[::5] = np.floor(carrier[::5])  # whole delays too (both taps on one slot)
    rows = [planted(carrier, PLANT_POSITIONS, [v] * len(PLANT_POSITIONS)) for v in vals]
    rows.append(planted(carrier, PLANT_POSITIONS, [vals[j % len(vals)] for j in range(len(PLANT_POSITIONS))]))
    ds = np.stack(rows)
    xs = np.repeat(x[None], len(ds), axis=0)
    ex = descriptor.extract(d.Delay(d.HostSource(x), d.HostSource(ds[0]), max_delay))
    assert [type(s).__name__ for s in ex.sources] == ["HostSource", "HostSource"]
    # which stream is x: the extraction lists the sources in circuit order
    first_is_x = np.array_equal(ex.sources[0].samples, x)
    inputs = np.stack([xs, ds] if first_is_x else [ds, xs])
    out = np.stack([delay(x, row, max_delay) for row in ds])
    c = Case("delay_%d" % max_delay, ex.words, STREAM_N, len(ds), outlet(out)[:, None, :], inputs=inputs, sr=sr)
    _case_cache[key] = c
    return c


SRR_AMOUNTS = (math.nan, math.inf, -math.inf, 0.0, -3.0, 0.5, 1e9)


def srr_case(sr=48000):
    """SampleRateRedux(HostSource x, HostSource amount): amount a mild carrier (0..6 samples) with NaN, +-Inf, 0, -3, 0.5 and 1e9 planted,
    singly at the plant positions and as runs."""
    key = ("srr", sr)
    if key in _case_cache:
        return _case_cache[key]
    import dusp_amd as d
    from dusp_amd import descriptor
    d.configure(sr)
    x = mild(STREAM_N, 21)
    carrier = mild(STREAM_N, 22, 0.0, 6.0)
    rows = []
    for v in SRR_AMOUNTS:
        s = planted(carrier, PLANT_POSITIONS, [v] * len(PLANT_POSITIONS))
        s[800:1100] = np.float32(v)
        rows.append(s)
    rows.append(np.full(STREAM_N, math.inf, np.float32))  # never updates: timeSinceLastUpdate starts at Infinity
    rows.append(f32(np.resize(np.array(SRR_AMOUNTS), STREAM_N)))
    am = np.stack(rows)
    xs = np.repeat(x[None], len(am), axis=0)
    ex = descriptor.extract(d.SampleRateRedux(d.HostSource(x), d.HostSource(am[0])))
    first_is_x = np.array_equal(ex.sources[0].samples, x)
    inputs = np.stack([xs, am] if first_is_x else [am, xs])
    out = np.stack([sample_rate_redux(x, row)[0] for row in am])
    c = Case("sample_rate_redux", ex.words, STREAM_N, len(am), outlet(out)[:, None, :], inputs=inputs, sr=sr)
    _case_cache[key] = c
    return c


PICK_INDICES = (0.0, 1.0, 2.0, 3.0, 4.0, 5.0)                       # channels c % 3
PICK_NON_INDICES = (1.5, -1.0, math.nan, math.inf, -math.inf, 0.5)  # the reference throws a TypeError in mid-render
PICK_NOT_AN_INDEX = "PickChannel index is not a channel number"
PICK_REFUSAL = "PickChannel with a signal-rate or per-instance channel index is not supported on the GPU path"


def pick_circuit(chans, c):
    import dusp_amd as d
    srcs = [d.HostSource(x) for x in chans]
    return d.PickChannel(d.ConcatChannels(d.ConcatChannels(srcs[0], srcs[1]), srcs[2]), c), srcs


def pick_case(c, sr=48000):
    """PickChannel of three channels (ConcatChannels of three streams) at the constant index c.  (The library takes a channel index as a
    constant of the circuit only — a stream or a per-instance parameter there is refused at build time with PICK_REFUSAL, on every engine —
    so the values 0, 1, 2, 3, 4, ... are planted as constants, one circuit each; a constant that is no channel number — 1.5, -1, NaN,
    Inf: the reference throws there, the oracle and the model give NaN — is refused at build time as well, with PICK_NOT_AN_INDEX.)"""
    key = ("pick", repr(c), sr)
    if key in _case_cache:
        return _case_cache[key]
    import dusp_amd as d
    from dusp_amd import descriptor
    d.configure(sr)
    v = 3
    chans = [mild(v * STREAM_N, 31 + k, 0.1 + k, 0.9 + k).reshape(v, STREAM_N) for k in range(3)]  # (never 0: a picked channel is told from the `|| 0`)
    unit, srcs = pick_circuit([x[0] for x in chans], c)
    ex = descriptor.extract(unit)
    by_unit = {id(u): k for k, u in enumerate(srcs)}
    inputs = np.stack([chans[by_unit[id(u)]] for u in ex.sources])
    out = np.stack([pick_channel([x[i] for x in chans], np.full(STREAM_N, c, np.float32)) for i in range(v)])
    case = Case("pick_channel_%r" % (c,), ex.words, STREAM_N, v, outlet(out)[:, None, :], inputs=inputs, sr=sr)
    _case_cache[key] = case
    return case


# ---- time-split circuits (one instance, 32 chunks)
SPLIT_N = 32 * CHUNK


def split_circuit(which):
    import dusp_amd as d
    if which == "wide_fm":          # increments up to 3e5: above 2^17 - sr
        return d.Osc(d.Multiply(d.Osc(70), 3e5))
    if which == "ratio_fm":         # Osc(3) / Osc(3): 1 wherever Osc(3) is not 0 — its phase first returns to 0 after sr / 3 samples
        return d.Osc(d.Multiply(d.Osc(70), d.Divide(d.Osc(3), d.Osc(3))))
    if which == "narrow_fm":        # increments within 440 +- 300: provably below 2^17 - sampleRate, the circuit whose render IS cut in time
        return d.Osc(d.Sum(d.Multiply(d.Osc(70), 300), 440))
    if which == "ratio_fm_poisoned":  # Osc(12)'s phase is 0 at sample sr / 12 - 1 (inside the render at 48 kHz): 0 / 0 = NaN from there on
        return d.Osc(d.Multiply(d.Osc(70), d.Divide(d.Osc(12), d.Osc(12))))
    raise KeyError(which)


def split_model(which, sr=48000, n=SPLIT_N):
    inner, _ = osc(np.full(n, 70.0, np.float32), "sin", sr)
    if which == "wide_fm":
        f = multiply(inner, np.full(n, 3e5, np.float32))
    elif which == "narrow_fm":
        f = add(multiply(inner, np.full(n, 300.0, np.float32)), np.full(n, 440.0, np.float32))
    else:
        o, _ = osc(np.full(n, 3.0 if which == "ratio_fm" else 12.0, np.float32), "sin", sr)
        f = multiply(inner, m_divide(o, o))
    out, ph = osc(f, "sin", sr)
    return outlet(out), ph, bool(is_tiny(f).any())


# --------------------------------------------------------------------------- the oracle on a case
_oracle_kept = {}


def oracle_render(oracle, case, with_state=False):
    """Every instance of a case on the CPU oracle -> f32 [n_inst, channels, n] (and every instance's unit states).  Kept per case: the
    engine columns of one case compare against the same render."""
    key = (case.name, case.sr, with_state)
    if key not in _oracle_kept:
        from concurrent.futures import ThreadPoolExecutor
        import os
        try:
            usable = len(os.sched_getaffinity(0))
        except AttributeError:
            usable = os.cpu_count() or 1

        def one(v):
            kw = {}
            if case.inputs is not None:
                kw["inputs"] = np.ascontiguousarray(case.inputs[:, v, :])
            if case.params is not None:
                kw.update(params=case.params, n_instances=case.n_inst, instance=v)
            return oracle.render(case.words, case.n, return_state=with_state, **kw)
        with ThreadPoolExecutor(max(1, min(16, usable))) as pool:
            got = list(pool.map(one, range(case.n_inst)))
        if with_state:
            _oracle_kept[key] = (np.stack([g[0] for g in got]), [g[1] for g in got])
        else:
            _oracle_kept[key] = np.stack(got)
        if len(_oracle_kept) > 6:
            _oracle_kept.pop(next(iter(_oracle_kept)))
    return _oracle_kept[key]
