"""Edge values at every signal inlet, on every engine, against the CPU oracle — which tests/test_edge_model.py pins to a plain f64 model
of the reference at exactly these streams and grids.  The reference vectors and the fuzz corpus keep their signals in [-1, 1] times a
modest gain; here NaN, +-Inf, -0, subnormals, negative bases, overflowing exponents and oscillator increments far above the sample rate
reach the maps, the oscillators, the delay taps, SampleRateRedux's comparison and PickChannel's index — as host streams (one per
instance) and as per-instance parameters.

Bit-equal to the oracle (NaN at the same samples) everywhere but:
  * the pow family (Pow, DecibelToScaler, SemitoneToRatio, Gain, MidiToFrequency, Pan's compensation): ulp_distance <= 1 against the
    model, NaN / non-NaN class equal, subnormal results not flushed.  Derived, not measured: the device's f64 pow is within 16 f64 ulp
    (the OpenCL bound its math library keeps), the host's within 1, so the two f64 results differ by less than 2^-48 relative; one
    rounding to f32 — for Gain / MidiToFrequency / Pan one exact-operand f64 multiply before it — lands on neighbouring f32 values at
    most.  Behind Divide(1, .) the same bound is carried through the division exactly: the result must be 1 / y for y the model's value
    or one of its two f32 neighbours of the same sign.
  * oscillator increments with 0 < |f| < 2^-13 ("tiny"), where the reference's own f64 sum rounds: the chunk engine stays bit-equal, the
    parallel engines are within REL_TOL of full scale, as tests/test_gpu_parity.py grants (BELOW_EXACT_REGIME).

Engines: chunk; interp (the wave engine's interpreter kernel, DUSP_WAVE_JIT=0); wave (compiled circuit kernels); auto where the circuit
is one of the fused shapes."""
import numpy as np
import pytest

import edge_values as ev
from conftest import knob_context
from dusp_amd import descriptor, render, runtime

pytestmark = pytest.mark.gpu

REL_TOL = 1e-5
ENGINES = ["chunk", "interp", "wave"]
ENGINE_ID = {"chunk": runtime.ENGINE_CHUNK, "interp": runtime.ENGINE_WAVE, "wave": runtime.ENGINE_WAVE, "auto": runtime.ENGINE_AUTO}

# Units an engine may refuse (status -2), with the library's message.  The chunk engine may refuse nothing; every unit must run on the
# interpreter kernel or on a compiled one.
REFUSED = {
    # ("Unit", "engine"): "message",
}
# Circuits the wave engine takes but the circuit compiler does not: they render on the interpreter kernel under "wave" as well.
NOT_COMPILED = set()

worst_pow = {"distance": 0, "where": None}


def context(engine, sr, **knobs):
    if engine == "interp":
        return knob_context(sr, DUSP_WAVE_JIT=0, **knobs)
    return knob_context(sr, **knobs) if knobs else render.context(sr)


def build(engine, case, unit=None, **knobs):
    try:
        return context(engine, case.sr, **knobs).build(case.words, ENGINE_ID[engine])
    except runtime.DuspHipError as e:
        assert e.status == -2, e
        assert engine != "chunk", "the chunk engine refused %s: %s" % (case.name, e.message)
        assert (unit, engine) in REFUSED and REFUSED[(unit, engine)] in e.message, "%s refused %s: %s" % (engine, case.name, e.message)
        pytest.skip(e.message)


def rendered(engine, prog, case, unit=None):
    got = prog.render(case.n, case.n_inst, case.params, inputs=case.inputs)
    shape = prog.read_shape()
    if engine == "interp":
        assert "compiled kernel" not in shape, shape
    if engine == "wave" and (unit or case.name) not in NOT_COMPILED:
        assert "compiled kernel" in shape, shape
    return got


def first_difference(got, want):
    bad = np.argwhere((got.view(np.uint32) != want.view(np.uint32)) & ~(np.isnan(got) & np.isnan(want)))
    at = tuple(int(i) for i in bad[0])
    return "%d samples differ, first at [instance, channel, sample][-%d:] = %r: got %r want %r" % (len(bad), len(at), at, got[at], want[at])


def assert_same(got, want, what):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert ev.same_bits(got, want), "%s: %s" % (what, first_difference(got, want))


def check_pow(got, case, what):
    """The pow family's bound against the model (module docstring)."""
    got = np.asarray(got, np.float32)
    assert got.shape == case.model.shape
    if not case.behind:
        dist = ev.ulp_distance(got, case.model)
        worst = int(dist.max())
        if worst > worst_pow["distance"] and worst < 1 << 30:
            at = np.unravel_index(int(np.argmax(dist)), dist.shape)
            worst_pow.update(distance=worst, where="%s instance %d channel %d sample %d: got %r model %r" % ((what,) + tuple(int(i) for i in at) + (got[at], case.model[at])))
        print("pow distance %s: worst %d" % (what, worst))
        assert worst <= 1, "%s: %s" % (what, first_difference(got, case.model))
        # subnormal results survive: where the model is at least two subnormal steps from zero, the device's is not zero
        sub = (np.abs(case.model) >= np.float32(2.8e-45)) & (np.abs(case.model) < np.float32(ev.F32_MIN))
        assert not (got[sub] == 0).any(), "%s: %d subnormal results flushed to zero" % (what, int((got[sub] == 0).sum()))
        return
    # behind Divide(1, .): 1 / y for y the model's own value of the unit or one of its f32 neighbours on the same side of zero
    raw = case.raw
    ok = np.zeros(raw.shape, bool)
    for toward in (None, -np.inf, np.inf):
        y = raw if toward is None else np.nextafter(raw, np.float32(toward))
        keep = np.signbit(y) == np.signbit(raw)
        cand = ev.outlet(ev.m_divide(np.ones_like(y), y))
        ok |= keep & ((cand.view(np.uint32) == got.view(np.uint32)) | (np.isnan(cand) & np.isnan(got)))
    assert ok.all(), "%s: %d samples are not 1 / (the model's value or a neighbour), first %s" % (what, int((~ok).sum()), np.argwhere(~ok)[0])


def check_map(engine, case, unit, oracle):
    prog = build(engine, case, unit)
    got = rendered(engine, prog, case, unit)
    prog.close()
    what = "%s on %s" % (case.name, engine)
    if case.pow:
        check_pow(got, case, what)
    else:
        assert_same(got, ev.oracle_render(oracle, case), what)


# ---- a. maps, through both operand channels
@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("behind", [False, True], ids=["bare", "behind_divide"])
@pytest.mark.parametrize("unit", ev.MAP_NAMES)
def test_map_streams(unit, behind, engine, oracle):
    check_map(engine, ev.map_stream_case(unit, behind), unit, oracle)


@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("behind", [False, True], ids=["bare", "behind_divide"])
@pytest.mark.parametrize("unit", ev.MAP_NAMES)
def test_map_parameter_grids(unit, behind, engine, oracle):
    check_map(engine, ev.map_grid_case(unit, behind), unit, oracle)


def test_every_map_runs_on_a_wave_engine_kernel():
    for unit in ev.MAP_NAMES + ["Multiply", "Sum"]:
        assert not ((unit, "interp") in REFUSED and (unit, "wave") in REFUSED), unit
        assert (unit, "chunk") not in REFUSED, unit


# ---- b. oscillators
def check_osc(engine, case, oracle, tiny_rows=None):
    """tiny_rows: instances in the tiny regime (None: none; an index array)."""
    prog = build(engine, case)
    got = rendered(engine, prog, case)
    want = ev.oracle_render(oracle, case)
    what = "%s on %s" % (case.name, engine)
    exact = np.ones(case.n_inst, bool)
    if tiny_rows is not None and engine != "chunk":
        exact[tiny_rows] = False
    assert_same(np.where(exact[:, None, None], got, 0), np.where(exact[:, None, None], want, 0), what)
    if not exact.all():
        scale = float(np.max(np.abs(want)))
        assert scale > 0.99, scale  # full-scale output next to the tiny increments
        err = float(np.max(np.abs(got[~exact].astype(np.float64) - want[~exact])))
        assert np.array_equal(np.isnan(got[~exact]), np.isnan(want[~exact])) and err <= REL_TOL * scale, "%s: max abs err %.3g vs full scale %.3g" % (what, err, scale)
    _, states = ev.oracle_render(oracle, case, with_state=True)
    for v in range(case.n_inst):
        w = states[v][case.osc_unit]
        g = prog.state(case.osc_unit, v)
        assert g.size == w.size, (v, g, w)
        if exact[v]:
            assert np.array_equal(g, w, equal_nan=True), "%s: state of instance %d: got %r want %r" % (what, v, g, w)
        else:  # every tiny increment is cut to the 2^-36 grid (< 2^-36 each) where the reference rounds its sum (<= 2^-37 each)
            assert np.allclose(g, w, rtol=0, atol=2 * case.n * 2.0 ** -36, equal_nan=True), (v, g, w)
    prog.close()


@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("sr", [48000, 44100])
@pytest.mark.parametrize("multi", [False, True], ids=["osc", "multiosc"])
@pytest.mark.parametrize("waveform", ev.OSC_WAVEFORMS)
@pytest.mark.parametrize("kind", ["folding", "poison", "tiny"])
def test_oscillator_streams(kind, waveform, multi, sr, engine, oracle):
    case = ev.osc_stream_case(kind, waveform, multi, sr)
    check_osc(engine, case, oracle, tiny_rows=np.arange(case.n_inst) if kind == "tiny" else None)


@pytest.mark.parametrize("engine", ["auto"] + ENGINES)
@pytest.mark.parametrize("sr", [48000, 44100])
@pytest.mark.parametrize("with_ramp", [False, True, "gain", "shape"], ids=["osc", "osc_x_ramp", "osc_x_gain", "osc_x_shape"])
def test_oscillator_constants(with_ramp, sr, engine, oracle):
    case = ev.osc_constant_case(with_ramp, sr)
    if engine == "auto":
        prog = context(engine, sr).build(case.words, runtime.ENGINE_AUTO)
        assert prog.engine == "fused", prog.engine
        prog.close()
    # (bit-equal for every member, the ones below 2^-13 included: an oscillator whose f is a constant or a per-instance parameter beyond
    # the exact regime runs the reference's loop with its f64 phase for the whole render, on every engine)
    check_osc(engine, case, oracle)


@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("kind", ["folding", "poison"])
def test_oscillator_stream_as_a_continued_chain(kind, engine, oracle):
    """One folding and one poison stream rendered in pieces (dusp_program_continue), cut at the chunk boundaries right behind planted
    values: the pieces equal the one-shot render, which equals the oracle."""
    sr = 48000
    case = ev.osc_stream_case(kind, "sin", False, sr)
    row = 0 if kind == "folding" else ev.PLANT_POSITIONS.index(255)  # folding: values at every plant position; poison: NaN at sample 255
    stream = case.streams[row]
    want = ev.oracle_render(oracle, case)[row]
    ctx = context(engine, sr)
    whole = ctx.build(case.words, ENGINE_ID[engine] | runtime.ENGINE_RESUMABLE)
    assert_same(whole.render(case.n, 1, inputs=stream[None, None, :])[0], want, "%s row %d on %s, one shot" % (case.name, row, engine))
    whole.close()
    cuts = [0, 256, 512, 6 * ev.CHUNK, case.n]  # behind the plants at 255, 511 and 5 * 256 + 77
    prog = ctx.build(case.words, ENGINE_ID[engine] | runtime.ENGINE_RESUMABLE)
    parts, words = [], case.words
    for a, b in zip(cuts[:-1], cuts[1:]):
        if a:
            words = descriptor.continued(case.words, a, [prog.state(u) for u in range(prog.n_units)])
            prog.continue_with(words)
        parts.append(prog.render(b - a, 1, inputs=stream[None, None, a:b])[0])
    prog.close()
    assert_same(np.concatenate(parts, axis=1), want, "%s row %d on %s, continued" % (case.name, row, engine))


# ---- c. time-split
@pytest.mark.parametrize("segments", [4, None], ids=["four_segments", "default"])
@pytest.mark.parametrize("engine", ["interp", "wave"])
@pytest.mark.parametrize("which", ["wide_fm", "ratio_fm", "ratio_fm_poisoned", "narrow_fm"])
def test_time_split(which, engine, segments, oracle):
    """One instance, 32 chunks, asked to be cut in time.  Segment totals cannot stand in for a phase the reference has rounded, so a render
    is cut only where the modulated oscillator's increments are provably below 2^17 - sampleRate (fused_plan.hpp wave_split_exact):
    narrow_fm (440 +- 300) is; wide_fm (up to 3e5) is not; nor are ratio_fm and ratio_fm_poisoned, whose Divide(Osc, Osc) no bound
    analysis can hold (it is 1 — until 0 / 0, which ratio_fm_poisoned meets in mid-render, at sample 3999).  Those render unsplit, their
    kernels running the reference's own loop on a chunk beyond the exact regime."""
    import dusp_amd as d
    d.configure(48000)
    ex = descriptor.extract(ev.split_circuit(which))
    knobs = {"DUSP_WAVE_SEGMENTS": segments} if segments else {}
    prog = context(engine, 48000, **knobs).build(ex.words, runtime.ENGINE_WAVE)
    got = prog.render(ev.SPLIT_N)[0]
    shape = prog.read_shape()
    assert ("compiled kernel" in shape) == (engine == "wave"), shape
    if which == "narrow_fm":  # (the default cuts one instance's 32 chunks into four segments as well: at least eight chunks each)
        assert shape.endswith(", 4 seg"), shape
    else:
        assert " seg" not in shape, shape
    want, states = oracle.render(ex.words, ev.SPLIT_N, return_state=True)
    what = "%s on %s (%s)" % (which, engine, shape)
    if not ev.split_model(which)[2] or which == "ratio_fm_poisoned":
        assert_same(got, want, what)
        for u, w in enumerate(states):
            assert np.array_equal(prog.state(u), w, equal_nan=True), (u, prog.state(u), w)
    else:
        # ratio_fm: Osc(70) reads 6.5e-5 at table index 24000, so the modulated oscillator meets increments below 2^-13 — the tiny regime,
        # where the parallel forms are within REL_TOL of full scale and their phase within 2^-36 per sample (module docstring)
        # (with increments of at most 1 the render's own full scale is 0.029 here, not the table's: the bound is taken of that, the smaller)
        scale = float(np.max(np.abs(want)))
        assert 0.02 < scale < 0.03 and np.array_equal(np.isnan(got), np.isnan(want))
        err = float(np.max(np.abs(got.astype(np.float64) - want)))
        print("%s: max abs err %.3g vs full scale %.3g" % (what, err, scale))
        assert err <= REL_TOL * scale, "%s: max abs err %.3g vs full scale %.3g" % (what, err, scale)
        for u, w in enumerate(states):
            assert np.allclose(prog.state(u), w, rtol=0, atol=2 * ev.SPLIT_N * 2.0 ** -36, equal_nan=True), (u, prog.state(u), w)
    prog.close()


def test_the_baseline_sweep_keeps_its_time_split():
    """BASELINE configs[1], Multiply(Osc(Ramp(200, 100, 2)), Osc(3)): its modulated oscillator's increments are a Ramp's, at most 200 —
    provably below 2^17 - sampleRate — so a long single render is still cut into segments."""
    import dusp_amd as d
    d.configure(48000)
    ex = descriptor.extract(d.Multiply(d.Osc(d.Ramp(96000, 200, 100).trigger()), d.Osc(3)))
    prog = render.context(48000).build(ex.words, runtime.ENGINE_WAVE)
    prog.render(64 * ev.CHUNK)
    shape = prog.read_shape()
    prog.close()
    assert "compiled kernel" in shape and shape.endswith(" seg"), shape


@pytest.mark.parametrize("which", ["wide_fm", "narrow_fm"])
def test_segments_that_warm_up_stand_on_bounded_increments_too(which, oracle):
    """A Filter behind the modulated oscillator: a long single render of such a circuit is cut into segments that warm up, and those take
    the oscillator's start phase from segment totals as well.  Filter(narrow_fm, 1000) is cut (DUSP_FILTER_WARM=2: segments of two chunks);
    Filter(wide_fm, 1000), whose increments reach 3e5, is not.  Either way: the chunk engine's samples bit for bit (the sequential loop
    with the same Filter coefficients; DUSP_FILTER_SCAN=0: the recurrence as written), and the oracle's within the 1e-5 of full scale that
    every Filter graph is granted (its coefficients come through libm's tan)."""
    import dusp_amd as d
    d.configure(48000)
    ex = descriptor.extract(d.Filter(ev.split_circuit(which), 1000))
    ctx = knob_context(48000, DUSP_FILTER_WARM=2, DUSP_FILTER_SCAN=0)
    prog = ctx.build(ex.words, runtime.ENGINE_WAVE)
    got = prog.render(ev.SPLIT_N)[0]
    shape = prog.read_shape()
    prog.close()
    assert "compiled kernel" in shape and (" seg" in shape) == (which == "narrow_fm"), shape
    chunk = ctx.build(ex.words, runtime.ENGINE_CHUNK)
    want = chunk.render(ev.SPLIT_N)[0]
    chunk.close()
    assert_same(got, want, "Filter(%s) against the chunk engine (%s)" % (which, shape))
    ref = oracle.render(ex.words, ev.SPLIT_N)
    err, scale = float(np.max(np.abs(got.astype(np.float64) - ref))), float(np.max(np.abs(ref)))
    print("Filter(%s): max abs err against the oracle %.3g of full scale %.3g" % (which, err, scale))
    assert err <= REL_TOL * scale, (err, scale)


def test_fm_voices_with_parameters_keep_their_time_split(oracle):
    """A few FM voices whose increments hang on per-instance parameters: a host render brings its parameter table, the planner bounds the
    columns (largest magnitude of each) and the render is still cut in time; with a parameter of 3e5 in the table it is not — and both equal
    the oracle."""
    import dusp_amd as d
    d.configure(48000)
    voice = lambda k: d.Multiply(d.Osc(d.Sum(d.Multiply(d.Osc(3 + k / 4), 40), 220.5 + 10 * k)), d.Ramp(4000, 1, 0.25).trigger())  # noqa: E731
    uni = descriptor.unify([descriptor.extract(voice(k)) for k in range(5)])
    wide = uni.params.copy()
    wide[int(np.argmax(uni.params.max(axis=1))), 3] = 3e5  # the base frequency of voice 3
    for params, split in ((uni.params, True), (wide, False)):
        prog = knob_context(48000, DUSP_WAVE_SEGMENTS=4).build(uni.words, runtime.ENGINE_WAVE)
        got = prog.render(ev.SPLIT_N, uni.n_instances, params)
        shape = prog.read_shape()
        prog.close()
        assert "compiled kernel" in shape and shape.endswith(", 4 seg") == split, shape
        for v in (0, 3, 4):
            want = oracle.render(uni.words, ev.SPLIT_N, params=params, n_instances=uni.n_instances, instance=v)
            assert_same(got[v], want, "voice %d (%s)" % (v, shape))


# ---- d. other stateful inlets, on streams
def check_plain(engine, case, oracle, **knobs):
    prog = build(engine, case, **knobs)
    got = rendered(engine, prog, case)
    prog.close()
    assert_same(got, ev.oracle_render(oracle, case), "%s on %s" % (case.name, engine))


@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("max_delay", [300, 2048])
def test_delay_times(max_delay, engine, oracle):
    """Delay(x, d, maxDelay) with d negative, NaN, +-Inf, exactly maxDelay, maxDelay - 0.5, 2 maxDelay + 0.25, 1e18, -0 and a fraction, under
    the suite's DUSP_GUARD=1 and with poisoned rings.  Every conversion of a tap position to a ring index sits behind its range test
    (read before the first run): chunk_engine.hip `if (lo >= 0.0 && lo < dlen)` / `if (hi >= 0.0 && hi < dlen)` in front of the two
    `(int64_t)` casts of the signal-rate path (its constant-delay fast path needs `dconst >= kBatch`, which NaN and negatives fail);
    wave_engine.hip ordered slot operations and jit_prelude.hpp JitRingOps `slo = (lo >= 0.0 && lo < dlen) ? (int32_t)lo : -1` (and `shi`
    alike; a slot of -1 is never pending); JitDelayGather `valid = lo >= 0.0 && lo < dlen` in front of `(int32_t)lo`, and the gather runs
    only where every lane's tap is valid (`__all(ok)`), else the chunk goes to JitRingOps.  NaN and Inf fail every one of these
    comparisons (fmod(Inf, len) is NaN).  The write-once rings and LDS lines take constant delays only: a stream does not reach them."""
    check_plain(engine, ev.delay_case(max_delay), oracle, DUSP_RING_POISON=1)


@pytest.mark.parametrize("engine", ENGINES)
def test_sample_rate_redux_amounts(engine, oracle):
    check_plain(engine, ev.srr_case(), oracle)


@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("c", ev.PICK_INDICES, ids=[repr(c) for c in ev.PICK_INDICES])
def test_pick_channel_indices(c, engine, oracle):
    check_plain(engine, ev.pick_case(c), oracle)


@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("c", ev.PICK_NON_INDICES, ids=[repr(c) for c in ev.PICK_NON_INDICES])
def test_pick_channel_non_indices_are_refused(c, engine):
    """An index that is no channel number makes the reference throw in mid-render; the library says so when the program is built."""
    with pytest.raises(runtime.DuspHipError) as e:
        context(engine, 48000).build(ev.pick_case(c).words, ENGINE_ID[engine])
    assert e.value.status == -1 and ev.PICK_NOT_AN_INDEX in e.value.message, e.value


@pytest.mark.parametrize("engine", ENGINES)
def test_pick_channel_takes_no_index_stream(engine):
    """A channel index is a constant of the circuit: as a stream it is refused when the program is built, whatever the engine."""
    import dusp_amd as d
    d.configure(48000)
    x = ev.mild(600, 5)
    ex = descriptor.extract(ev.pick_circuit([x, x, x], d.HostSource(x))[0])
    with pytest.raises(runtime.DuspHipError) as e:
        context(engine, 48000).build(ex.words, ENGINE_ID[engine])
    assert e.value.status == -2 and ev.PICK_REFUSAL in e.value.message, e.value


@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("behind", [False, True], ids=["bare", "behind_divide"])
@pytest.mark.parametrize("unit", ["Multiply", "Sum"])
def test_multiply_and_sum_streams(unit, behind, engine, oracle):
    check_map(engine, ev.map_stream_case(unit, behind), unit, oracle)
