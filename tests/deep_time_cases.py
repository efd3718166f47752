"""The voices of the deep-timeline tests (tests/test_deep_time_model.py on the CPU, tests/test_gpu_deep_time.py on the kernels) in the
model's notation (tests/deep_time.py), and the circuits that go with them."""
import numpy as np

RATES = (44100, 48000, 96000, 192000)
DEEPEST_FIRST = 1 << 40
RAMP = (2 * DEEPEST_FIRST + 12345, 1, 0)  # twice the deepest window start, no power of two: still playing everywhere


def f32(x):
    return float(np.float32(x))


def frequencies(kind, sr):
    """int: every phase a whole table step (the sum chain's INT path); frac: 32.32 fixed point."""
    if kind == "int":
        return [10.0 * k for k in range(1, 6)]
    return [20 + k / 8 for k in range(1, 4)] + [440.5, f32(12345.678), -3.25, sr - 0.5]


def voices(kind, env, sr):
    """env 0: bare oscillators; 1: each times a constant; 2: each times an equal triggered Ramp."""
    fs = frequencies(kind, sr)
    if env == 0:
        return [("osc", f) for f in fs]
    if env == 1:
        return [("gain", f, 0.25 + k / 16) for k, f in enumerate(fs)]
    return [("ramp", f, RAMP) for f in fs]


SETS = [(kind, env) for kind in ("int", "frac") for env in (0, 1, 2)]


def unit_of(voice):
    import dusp_amd as d
    o = d.Osc(voice[1])
    if voice[0] == "gain":
        return d.Multiply(o, voice[2]), o
    if voice[0] == "ramp":
        return d.Multiply(o, d.Ramp(*voice[2]).trigger()), o
    return o, o


def chain(vs, sr):
    """Sum.many over the voices -> (descriptor words, the unit index of every voice's Osc in chain order)."""
    import dusp_amd as d
    from dusp_amd import descriptor
    d.configure(sr)
    built = [unit_of(v) for v in vs]
    ex = descriptor.extract(d.Sum.many([b[0] for b in built]) if len(built) > 1 else built[0][0])
    units = list(ex.circuit.units)
    return ex.words, [[id(u) for u in units].index(id(b[1])) for b in built]
