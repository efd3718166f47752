"""The render path at sample rates other than 44.1 and 48 kHz, on the device, against the reference's goldens and the oracle.

What depends on the rate (tests/test_sample_rates.py has the host side): whether the oscillators' half-table image goes into LDS
(even rates whose image fits: up to about 85 kHz; above that the compiled kernels gather their lookups from global memory), which
tables have closed forms (the square at every rate, the triangle where 4 | sr), and which engines take the rate at all (the wave
engine and the circuit compiler stop at 2^17: AUTO renders on the chunk engine there)."""
import numpy as np
import pytest

import dusp_amd as d
from conftest import Golden, golden_names, knob_context
from dusp_amd import descriptor, render, runtime
from test_gpu_parity import ENGINES, check, engine_context

pytestmark = pytest.mark.gpu

GOLDEN_RATES = [8000, 11025, 22050, 32000, 96000, 192000]
RATE_GOLDEN = [name for sr in GOLDEN_RATES for name in golden_names(sr)]
MATRIX_RATES = [8000, 11025, 22050, 32000, 88200, 96000, 192000]
WAVE_MAX_RATE = 131072
REL_TOL = 1e-5


@pytest.mark.parametrize("engine", ["auto", "chunk", "wave", "interp"])
@pytest.mark.parametrize("name", RATE_GOLDEN)
def test_golden_at_other_rates(name, engine, oracle):
    """Every golden at the new rates through each engine column of test_gpu_parity.py: bit-exact (Filters: 1e-5 of full scale);
    above 2^17 the wave engine refuses with -2 and AUTO still renders."""
    g = Golden(name)
    base = name[: name.rindex("_sr")]
    ctx = engine_context(g.sample_rate, engine)
    if engine in ("wave", "interp") and g.sample_rate > WAVE_MAX_RATE:
        with pytest.raises(runtime.DuspHipError) as e:
            ctx.build(g.desc, ENGINES[engine])
        assert e.value.status == -2 and "sample rate above 2^17" in e.value.message
        return
    prog = ctx.build(g.desc, ENGINES[engine])
    assert prog.n_out_channels == g.n_channels
    pcm = prog.render(g.n_samples)[0]
    shape = prog.read_shape()
    if engine == "wave":
        assert "compiled kernel" in shape, shape  # (the compiler takes every one of these circuits up to 2^17)
    if engine == "interp":
        assert "compiled kernel" not in shape
    if engine == "auto" and g.sample_rate > WAVE_MAX_RATE:
        assert prog.engine in ("fused", "chunk"), prog.engine
    check(base, g.windowed(pcm), g.pcm, engine)
    check(base, pcm, oracle.render(g.desc, g.n_samples), engine)
    prog.close()


def _batch(builders, V):
    """A batch of V instances of one structure: the per-instance constants run linearly from the first builder's to the last's."""
    uni = descriptor.unify([descriptor.extract(b()) for b in builders])
    k = uni.n_instances - 1
    if k == 0:
        return uni.words, uni.params
    params = (uni.params[:, :1] + (uni.params[:, k:k + 1] - uni.params[:, :1]) * np.arange(V)[None, :] / k).astype(np.float32)
    return uni.words, params


# rows of the rate-by-path matrix: (name, builder of instance k, instances, the engine AUTO must pick, within tolerance)
ROWS = {
    "osc": (lambda k: d.Osc(110.5 + 7 * k), 1024, "fused", False),
    "osc_ramp": (lambda k: d.Multiply(d.Osc(110.5 + 7 * k), d.Ramp(1500, 1, 0).trigger()), 1024, "fused", False),
    "osc_gain": (lambda k: d.Multiply(d.Osc(110.5 + 7 * k), 0.5 + 0.25 * k), 1024, "fused", False),
    "osc_shape": (lambda k: d.Multiply(d.Osc(110.5 + 7 * k), d.Shape("semiSine", 0.03).trigger()), 1024, "fused", False),
    "summany": (lambda k: d.Sum.many([d.Osc(10.25 * (j + 1)) for j in range(64)]), 1, "fused", False),  # (one mix-down: constant f)
    "fm_pair": (lambda k: d.Osc(d.Sum(d.Multiply(d.Osc(3 + k), 200), 440 + 5 * k)), 256, "wave", False),
    "four_osc": (lambda k: d.Sum.many([d.Osc(f + k) for f in (110.25, 220.5, 331.0, 441.75)]), 256, "wave", False),
    "filter_const": (lambda k: d.Filter(d.Osc(150 + k, "saw"), 3000), 256, "wave", True),
    "filter_mod": (lambda k: d.Filter(d.Osc(150 + k, "saw"), d.Sum(d.Multiply(d.Osc(5), 800), 1000)), 256, "wave", True),
    "delay_300": (lambda k: d.Delay(d.Osc(500 + k), 300, 1024), 256, "wave", False),
    "delay_300p5": (lambda k: d.Delay(d.Osc(500 + k), 300.5, 1024), 256, "wave", False),
    "osc_ahd": (lambda k: d.Multiply(d.Osc(440.5 + k), d.AHD(0.01, 0.02, 0.03).trigger()), 256, "wave", False),
    "circlebuffer": (lambda k: _taps(330 + k), 256, "wave", False),
}


def _taps(f):
    buffer = d.CircleBuffer(1, 0.05)
    writer = d.CircleBufferWriter(buffer)
    writer.preWipe = True
    writer.IN = d.Osc(f)
    tap = d.CircleBufferReader(buffer, 0.01)
    tap.chain(writer)
    fb_tap = d.CircleBufferReader(buffer, 0.02)
    fb_tap.chain(writer)
    fb_writer = d.CircleBufferWriter(buffer, 0.005)
    fb_writer.IN = d.quick.multiply(fb_tap, 0.5)
    fb_writer.chain(writer)
    return d.Sum(tap, fb_tap)


@pytest.mark.parametrize("row", list(ROWS))
@pytest.mark.parametrize("sr", MATRIX_RATES)
def test_rate_by_path_matrix(sr, row, oracle):
    """Batches with per-instance parameters at every rate, instance by instance against the oracle.  Up to 2^17 the wave-engine
    circuits run on their compiled kernels (where the table image does not fit, with gathered lookups: the compiler stays on)."""
    build, V, engine, tolerant = ROWS[row]
    d.configure(sr)
    try:
        words, params = _batch([lambda: build(0), lambda: build(1)] if V > 1 else [lambda: build(0)], V)
    finally:
        d.configure(48000)
    n = 4096 + 37
    prog = render.context(sr).build(words, runtime.ENGINE_AUTO)
    got = prog.render(n, V, params)
    shape = prog.read_shape()
    if row == "summany" and sr % 2:  # (the sum chain's 32.32 phases need every nonzero |T| >= 2^-20: at an odd rate the sine's T[N/2] is sin(pi))
        engine = "wave"
    if engine == "wave" and sr > WAVE_MAX_RATE:
        assert prog.engine == "chunk", (prog.engine, shape)
    else:
        assert prog.engine == engine, (prog.engine, shape)
    if prog.engine == "wave":
        assert "compiled kernel" in shape, shape
    want = oracle.render_instances(words, n, params, V, range(V))
    for i in range(V):
        if tolerant:
            scale = max(1e-30, float(np.max(np.abs(want[i]))))
            err = float(np.max(np.abs(got[i].astype(np.float64) - want[i])))
            assert err <= REL_TOL * scale, (i, err, scale)
        else:
            assert np.array_equal(got[i], want[i]), (i, int(np.argmax(got[i] != want[i])))
    prog.close()


def test_product_default_short_then_long_render_at_96k(oracle):
    """DUSP_WAVE_JIT=1: a short first render of a new structure runs on the interpreter while its kernel compiles in the background;
    the renders after it are right whichever kernel they find, and once the compile is done a program of the structure runs on its
    compiled kernel.  At 96 kHz that kernel must be one that compiles (no 198 KB table image in LDS)."""
    import time
    d.configure(96000)
    try:  # (a structure no other test builds)
        words, params = _batch([lambda k=k: d.Multiply(d.Osc(d.Sum(d.Multiply(d.Osc(2.75 + k), 150), 330.5 + 3 * k)), 0.75) for k in (0, 1)], 256)
    finally:
        d.configure(48000)
    ctx = knob_context(96000, DUSP_WAVE_JIT=1)

    def run(V, n):
        prog = ctx.build(words, runtime.ENGINE_WAVE)
        got = prog.render(n, V, params[:, :V])
        shape = prog.read_shape()
        prog.close()
        want = oracle.render_instances(words, n, params[:, :V], V, range(V))
        for i in range(V):
            assert np.array_equal(got[i], want[i]), (n, i, shape)
        return shape

    assert "kernel compiling" in run(2, 256 * 3 + 5)
    run(256, 96000)  # (a second of every instance: on the kernel if the compile is done by now, else on the interpreter)
    deadline = time.perf_counter() + 60
    while True:  # a fresh program of the structure finds the kernel once the background compile is done
        shape = run(2, 256 * 3 + 5)
        if "compiled kernel" in shape or time.perf_counter() > deadline:
            break
        time.sleep(0.1)
    assert "compiled kernel" in shape, shape


def _f32_below(x):
    return float(np.nextafter(np.float32(x), np.float32(0)))


@pytest.mark.parametrize("sr", MATRIX_RATES)
def test_oscillator_phase_edges(sr, oracle):
    """The gates of the phase forms (LEAN: every phase on the 2^-28 grid, |f| >= 2^-4; FX: 2^-32, |f| >= 2^-8) and one f32 step
    below each, an increment one half below the rate, a negative third of it and a tiny one: on the compiled and the fused kernel."""
    freqs = [2.0 ** -4, _f32_below(2.0 ** -4), 2.0 ** -8, _f32_below(2.0 ** -8), sr - 0.5, -sr / 3, 3e-5]
    n = 4096 + 37
    d.configure(sr)
    try:
        descs = [descriptor.extract(d.Osc(f)).words for f in freqs]
    finally:
        d.configure(48000)
    ctx = render.context(sr)
    for f, words in zip(freqs, descs):
        want = oracle.render(words, n)
        fused = ctx.build(words, runtime.ENGINE_AUTO)
        assert fused.engine == "fused", fused.engine
        assert np.array_equal(fused.render(n)[0], want), ("fused", f)
        fused.close()
        if sr > WAVE_MAX_RATE:
            with pytest.raises(runtime.DuspHipError) as e:
                ctx.build(words, runtime.ENGINE_WAVE)
            assert e.value.status == -2
            continue
        wave = ctx.build(words, runtime.ENGINE_WAVE)
        got = wave.render(n)[0]
        assert "compiled kernel" in wave.read_shape()
        if abs(f) < 2.0 ** -13:  # (the reference's own f64 accumulation rounds there: the wave engine is within tolerance, test_gpu_parity.py)
            assert float(np.max(np.abs(got.astype(np.float64) - want))) <= REL_TOL * float(np.max(np.abs(want)))
        else:
            assert np.array_equal(got, want), ("compiled", f, int(np.argmax(got != want)))
        wave.close()


def test_continued_render_across_an_event_at_an_odd_rate(oracle):
    """renderChannelData at 11025 Hz with a scheduled event: the render is cut at the event's chunk and ONE device program continued
    across it (a 300.5-sample delay line and a triangle oscillator, whose table at this rate is the reference's partial one)."""
    def voice():
        osc = d.Osc(330.25, "triangle")
        return osc, d.Sum(d.Delay(osc, 300.5, 1024), d.Multiply(d.Osc(3, "square"), 0.25))

    d.configure(11025)
    try:
        seen = []
        osc, out = voice()
        osc.schedule(0.05, lambda u: seen.append(u.circuit.clock))
        split = np.stack(d.renderChannelData(out, 0.2))
        _, plain = voice()
        words = descriptor.extract(plain).words
        whole = np.stack(d.renderChannelData(plain, 0.2))
    finally:
        d.configure(48000)
    assert len(seen) == 1 and 0 < seen[0] < 2205
    assert split.shape == whole.shape == (1, 2205)
    assert np.array_equal(split, whole)
    assert np.array_equal(whole[0], oracle.render(words, 2205)[0])
