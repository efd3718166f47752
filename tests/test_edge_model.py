"""The f64 model of tests/edge_values.py against the CPU oracle, bit for bit, on every stream and parameter grid that
tests/test_gpu_edge_values.py renders on the engines — the pow family included: both use this host's libm.  The reference vectors
never reach these values (NaN, +-Inf, -0, subnormals, negative bases, overflowing exponents, oscillator increments far above the
sample rate), and new reference-generated vectors are out of reach; two independent restatements of the reference's `_tick`s that
agree to the bit are what makes the oracle a judge there.

The last tests show that the oscillator cases tell the reference's rounded f64 phase loop from the modular identity
(a + b) % m == (a + b % m) % m that the parallel engines used to apply to increments of any size."""
import numpy as np
import pytest

import edge_values as ev


def agree(case, oracle):
    got = ev.oracle_render(oracle, case)
    assert got.shape == case.model.shape, (got.shape, case.model.shape)
    if not ev.same_bits(got, case.model):
        bad = np.argwhere((got.view(np.uint32) != case.model.view(np.uint32)) & ~(np.isnan(got) & np.isnan(case.model)))
        v, c, t = bad[0]
        raise AssertionError("%s: %d samples differ, first at instance %d channel %d sample %d: oracle %r model %r"
                             % (case.name, len(bad), v, c, t, got[v, c, t], case.model[v, c, t]))


@pytest.mark.parametrize("behind", [False, True], ids=["bare", "behind_divide"])
@pytest.mark.parametrize("name", ev.MAP_NAMES + ["Multiply", "Sum"])
def test_map_streams(name, behind, oracle):
    agree(ev.map_stream_case(name, behind), oracle)


@pytest.mark.parametrize("behind", [False, True], ids=["bare", "behind_divide"])
@pytest.mark.parametrize("name", ev.MAP_NAMES)
def test_map_parameter_grids(name, behind, oracle):
    agree(ev.map_grid_case(name, behind), oracle)


def test_the_grid_and_the_streams_hold_every_ordered_pair_at_every_lane_position():
    a, b = ev.pairs(ev.EDGE)
    n = len(ev.EDGE)
    assert len(a) % (4 * ev.CHUNK) == 0
    key = lambda x: np.where(np.isnan(x), np.uint32(0x7FC00000), x.view(np.uint32)).astype(np.uint64)  # noqa: E731
    want = {(int(p), int(q)) for p in key(ev.EDGE) for q in key(ev.EDGE)}
    assert len(want) == n * n
    for pos in range(4):
        assert want <= {(int(p), int(q)) for p, q in zip(key(a[pos::4]), key(b[pos::4]))}, pos
    assert set(ev.PLANT_POSITIONS) >= {0, 1, 3, 4, 251, 252, 255, 256, 257, 511, 512} and max(ev.PLANT_POSITIONS) >= 2 * ev.CHUNK + ev.CHUNK


def test_ulp_distance():
    f = np.float32
    assert ev.ulp_distance(f(ev.F32_MAX), f(np.inf)) == 1 and ev.ulp_distance(f(-np.inf), f(-ev.F32_MAX)) == 1
    assert ev.ulp_distance(f(0.0), f(-0.0)) == 0 and ev.ulp_distance(f(1e-45), f(-1e-45)) == 2
    assert ev.ulp_distance(f(1.0), np.nextafter(f(1.0), f(2.0))) == 1
    assert ev.ulp_distance(f(np.nan), f(np.nan)) == 0 and ev.ulp_distance(f(np.nan), f(1.0)) > 1 << 30 and ev.ulp_distance(f(np.inf), f(np.nan)) > 1 << 30


def test_math_pow_deviations_from_c_pow():
    assert np.isnan(ev.js_pow(1.0, np.nan)) and np.isnan(ev.js_pow(1.0, np.inf)) and np.isnan(ev.js_pow(-1.0, -np.inf))
    assert ev.js_pow(np.nan, 0.0) == 1.0 and ev.js_pow(-8.0, 1.0 / 3) != ev.js_pow(-8.0, 1.0 / 3) and ev.js_pow(-2.0, 3.0) == -8.0


@pytest.mark.parametrize("sr", [48000, 44100])
@pytest.mark.parametrize("multi", [False, True], ids=["osc", "multiosc"])
@pytest.mark.parametrize("waveform", ev.OSC_WAVEFORMS)
@pytest.mark.parametrize("kind", ["folding", "poison", "tiny"])
def test_oscillator_streams(kind, waveform, multi, sr, oracle):
    case = ev.osc_stream_case(kind, waveform, multi, sr)
    agree(case, oracle)
    _, states = ev.oracle_render(oracle, case, with_state=True)
    for v in range(case.n_inst):
        want = states[v][case.osc_unit]
        phase = want[-1]  # (MultiChannelOsc: [n, phase of channel 0])
        assert phase == case.phase[v] or (phase != phase and case.phase[v] != case.phase[v]), (v, phase, case.phase[v])
    if kind == "poison" and not multi:  # NaN from the planted sample on, through every later chunk — hidden behind the outlet's `|| 0`
        _, at = ev.poison_streams(sr)
        assert np.isnan(case.phase).all()
        for v, p in enumerate(at):
            assert not case.model[v, 0, p:].any() and case.model[v, 0, :p].any() == (p > 0)
    if kind == "tiny":  # the streams hold full-scale output next to the tiny increments
        assert float(np.max(np.abs(case.model))) > 0.99


@pytest.mark.parametrize("sr", [48000, 44100])
@pytest.mark.parametrize("with_ramp", [False, True, "gain", "shape"], ids=["osc", "osc_x_ramp", "osc_x_gain", "osc_x_shape"])
def test_oscillator_constants(with_ramp, sr, oracle):
    case = ev.osc_constant_case(with_ramp, sr)
    agree(case, oracle)
    _, states = ev.oracle_render(oracle, case, with_state=True)
    for v in range(case.n_inst):
        phase = states[v][case.osc_unit][0]
        assert phase == case.phase[v] or (phase != phase and case.phase[v] != case.phase[v]), (v, case.f[v], phase, case.phase[v])


@pytest.mark.parametrize("which", ["wide_fm", "ratio_fm", "ratio_fm_poisoned", "narrow_fm"])
def test_time_split_circuits(which, oracle):
    import dusp_amd as d
    from dusp_amd import descriptor
    d.configure(48000)
    ex = descriptor.extract(ev.split_circuit(which))
    want, phase, tiny = ev.split_model(which)
    got, states = oracle.render(ex.words, ev.SPLIT_N, return_state=True)
    assert ev.same_bits(got[0], want)
    # Osc(70) reads sin(pi * 48000 / 48001) = 6.5e-5 at table index 24000 (sample 2399): times 1 that is an increment below 2^-13
    assert tiny == which.startswith("ratio_fm")
    # ratio_fm never meets 0 / 0 within these 32 chunks (Osc(3) returns to phase 0 after 16000 samples); its faster twin does, in mid-render
    assert np.isnan(phase) == (which == "ratio_fm_poisoned")
    if which == "ratio_fm_poisoned":
        first = 48000 // 12 - 1
        assert want[:first].any() and not want[first:].any() and 0 < first < ev.SPLIT_N


@pytest.mark.parametrize("max_delay", [300, 2048])
def test_delay(max_delay, oracle):
    agree(ev.delay_case(max_delay), oracle)


def test_sample_rate_redux(oracle):
    agree(ev.srr_case(), oracle)


@pytest.mark.parametrize("c", ev.PICK_INDICES + ev.PICK_NON_INDICES, ids=[repr(c) for c in ev.PICK_INDICES + ev.PICK_NON_INDICES])
def test_pick_channel(c, oracle):
    case = ev.pick_case(c)
    agree(case, oracle)
    assert bool(case.model.any()) == (c in ev.PICK_INDICES)  # a channel's samples, or NaN (+0 at the outlet) throughout


# ---- the oscillator cases tell the rounded f64 loop from the modular identity
@pytest.mark.parametrize("sr", [48000, 44100])
def test_folding_streams_expose_the_modular_identity(sr):
    """Feeding the parallel engines' former arithmetic (ev.osc_phases_modular) through the assertion the GPU test makes: it must FAIL
    on the folding streams, and on the large constants, wherever a planted increment makes the reference's `phase + f` round."""
    streams = ev.folding_streams(sr)
    tbl = ev.table("saw", sr)  # (saw: every phase step shows)
    differing = 0
    for s in streams:
        ref = ev.outlet(ev.osc_lookup(ev.osc_phases(s, sr), tbl, sr))
        dev = ev.outlet(ev.osc_lookup(ev.osc_phases_modular(s, sr), tbl, sr))
        differing += not ev.same_bits(ref, dev)
    assert differing >= len(streams) - 2, differing  # (every stream holds one of 1e9 .. FLT_MAX)
    # one mild phase, one huge increment: the reference loses the phase it had (37 table steps here), the identity keeps it
    f = np.concatenate([np.full(100, 0.37, np.float32), ev.f32([1e18])])
    lost = ev.osc_phases(f, sr)[-1] - ev.osc_phases_modular(f, sr)[-1]
    assert abs(abs(lost) - 37.0000005) < 1e-4 or abs(abs(lost) - (sr - 37.0000005)) < 1e-4, lost
    # below the bound the two agree to the bit
    mild = ev.planted(np.full(ev.STREAM_N, 440.5, np.float32), ev.PLANT_POSITIONS, [sr, -sr, 65536.0, 2.0 ** 17 - sr - 0.5] * 3)
    assert np.array_equal(ev.osc_phases(mild, sr), ev.osc_phases_modular(mild, sr))


def test_large_constants_expose_the_modular_identity():
    sr = 48000
    wrong = []
    for f in ev.edge(sr):
        if not np.isfinite(f) or ev.is_tiny(f):
            continue
        s = np.full(ev.STREAM_N, f, np.float32)
        if not np.array_equal(ev.osc_phases(s, sr), ev.osc_phases_modular(s, sr)):
            wrong.append(float(f))
    # the constants whose steps the f64 sum cannot hold: 1e19 and +-FLT_MAX, where the phase sticks at f mod sr.  (A constant +-1e18 stays
    # exact: every phase it reaches is a multiple of 128, the f64 spacing at 1e18; 131072.375 and 3e5 + 0.37 stay on a grid that 53 bits hold.)
    assert sorted(wrong) == sorted(float(v) for v in ev.f32([1e19, ev.F32_MAX, -ev.F32_MAX])), wrong
