"""Deep in the timeline: every time-parallel path jumps to sample t by arithmetic, and here t is large — past 2^24 (where an index that
slipped through an f32 first shows), past the points where the sum chain's 64-bit block product used to wrap, and up to the 2^40 that
dusp_render_chain_window accepts.  Bit for bit against the exact model of tests/deep_time.py (tests/test_deep_time_model.py pins the
model to the oracle on the CPU) or, for circuits the model does not cover, the oracle's sequential render."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import deep_time as dt  # noqa: E402
import deep_time_cases as dc  # noqa: E402
import edge_values as ev  # noqa: E402
from conftest import knob_context  # noqa: E402

pytestmark = pytest.mark.gpu

NAN = float("nan")
WINDOW_N = (2048, 2048 * 2 + 256 * 3 + 37)  # whole blocks, and a partial last group
GUARD = 256                                  # floats behind every window that must stay as they were


def _ctx(sr):
    from dusp_amd import render
    return render.context(sr)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _window(prog, first, n, init=None, raw=False):
    """One chain window -> (f32 [n], whether the floats behind it are untouched)."""
    out = torch.full((n + GUARD,), NAN, dtype=torch.float32, device="cuda")
    d_init = None
    if init is not None:
        d_init = torch.from_numpy(np.ascontiguousarray(init, dtype=np.float32)).cuda()
    prog.render_chain_window(first, n, None if d_init is None else d_init.data_ptr(), raw, out.data_ptr(), _stream())
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    return got[:n], bool(np.all(np.isnan(got[n:])))


def wrap_firsts(fs, sr):
    """Where `blk * bs` of blocks counted from sample 0 passes 2^64, for every voice and both block sizes (4 and 8 groups): bs = (F * block)
    mod S in 32.32 fixed point, the first block past the wrap is 2^64 // bs.  -> window starts (multiples of 2048) that end on the last
    block before it and that begin on the first block after it, where the timeline up to 2^40 reaches them."""
    S = sr << 32
    firsts = set()
    for f in fs:
        F = int(float(np.float32(f)) * 2.0 ** 32) % S
        for block in (4 * 256, 8 * 256):
            bs = F * block % S
            if bs == 0:
                continue
            at = (2 ** 64 // bs) * block  # first sample of the first wrapped block
            before, after = at // 2048 * 2048 - 2048, -(-at // 2048) * 2048
            for first in (before, after):
                if 0 <= first <= dc.DEEPEST_FIRST:
                    firsts.add(first)
    return sorted(firsts)


def test_wrap_points_are_inside_the_accepted_timeline():
    """The derivation above finds the documented first wrong blocks: 192 kHz, f = 191999.5, 8 groups a block -> block 22489."""
    S = 192000 << 32
    bs = int(191999.5 * 2 ** 32) * 2048 % S
    assert 2 ** 64 // bs == 22489
    assert len(wrap_firsts(dc.frequencies("frac", 192000), 192000)) >= 4
    assert len(wrap_firsts(dc.frequencies("frac", 48000), 48000)) >= 4


# ------------------------------------------------------------------ a. chain windows deep in the timeline
@pytest.mark.parametrize("sr", dc.RATES)
@pytest.mark.parametrize("kind,env", dc.SETS)
def test_chain_windows_deep_in_the_timeline_equal_the_model(kind, env, sr):
    vs = dc.voices(kind, env, sr)
    words, _ = dc.chain(vs, sr)
    prog = _ctx(sr).build(words)
    assert "sumchain" in prog.shape, prog.shape
    firsts = sorted(set([0, 2048, 1 << 24, 1 << 32, 1 << 36, (1 << 40) - 2048, 1 << 40] + wrap_firsts([v[1] for v in vs], sr)))
    bad = []
    for first in firsts:
        for n in WINDOW_N:
            got, clean = _window(prog, first, n)
            want = dt.chain_window(vs, sr, first, n)
            if not clean:
                bad.append((first, n, "wrote behind the window"))
            elif not ev.same_bits(got, want):
                k = int(np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))[0])
                bad.append((first, n, "first wrong sample %d: %r, model %r" % (first + k, float(got[k]), float(want[k]))))
    prog.close()
    assert not bad, (kind, env, sr, len(bad), bad[:6])


@pytest.mark.parametrize("kind,env", dc.SETS)
def test_a_chain_of_two_programs_at_two_to_the_32_equals_the_model(kind, env):
    """The first voices in one program, the rest in another that continues the first one's raw window (init), at first = 2^32."""
    sr, first, n = 96000, 1 << 32, WINDOW_N[1]
    vs = dc.voices(kind, env, sr)
    cut = 2
    head, tail = _ctx(sr).build(dc.chain(vs[:cut], sr)[0]), _ctx(sr).build(dc.chain(vs[cut:], sr)[0])
    part, clean = _window(head, first, n, raw=True)
    assert clean and np.array_equal(part, dt.chain_window(vs[:cut], sr, first, n, raw=True))  # (raw: -0 and +0 are one value here)
    got, clean = _window(tail, first, n, init=part)
    assert clean and ev.same_bits(got, dt.chain_window(vs, sr, first, n))
    head.close()
    tail.close()


# ------------------------------------------------------------------ b. a plain render that crosses the wrap
CROSSING_SR, CROSSING_N = 192000, 46_080_000 + 3


@pytest.mark.parametrize("fs", [(191999.5, dc.f32(12345.678), 440.5), (187.0, 12345.0, 440.0)], ids=["frac", "int"])
def test_a_plain_render_across_the_wrap_equals_the_model(fs):
    """192 kHz, 240 s, Sum.many of three oscillators: 22,501 blocks of 8 groups; the first voice's block product passes 2^64 at block
    22489 (sample 46,057,472) — for 191999.5, and for the integer 187 as well (187 * 2048 mod 192000 = 190976 table steps a block).  The
    integer voices leave the INT path at this length ((blocks + 1) * sampleRate >= 2^32)."""
    sr, n = CROSSING_SR, CROSSING_N
    vs = [("osc", f) for f in fs]
    words, osc_units = dc.chain(vs, sr)
    prog = _ctx(sr).build(words)
    assert "sumchain" in prog.shape, prog.shape
    out = torch.full((n + GUARD,), NAN, dtype=torch.float32, device="cuda")
    prog.render_device(n, 1, None, out.data_ptr(), _stream())
    torch.cuda.synchronize()
    S = sr << 32
    wrap = 2 ** 64 // (int(float(np.float32(fs[0])) * 2 ** 32) * 2048 % S) * 2048
    assert wrap == 22489 * 2048 and wrap < n - 8192, wrap
    assert bool(torch.isnan(out[n:]).all())
    for first, count in ((0, 4096), (wrap - 2048, 4096), (n - 4099, 4099)):
        got = out[first:first + count].cpu().numpy()
        want = dt.chain_window(vs, sr, first, count)
        same = got.view(np.uint32) == want.view(np.uint32)
        assert same.all(), ("first wrong sample", first + int(np.flatnonzero(~same)[0]))
    for v, u in zip(vs, osc_units):
        assert prog.state(u)[0] == dt.end_phase(v[1], sr, dt.whole_chunks(n)), v
    prog.close()
    del out


# ------------------------------------------------------------------ c. past 2^24 on every jump-ahead path
DEEP_N = (1 << 24) + 4096 + 3
DEEP_WINDOWS = ((0, 2048), ((1 << 24) - 2048, 4096), (DEEP_N - 4099, 4099))
RAMP_LONG = ((1 << 25) + 12345, 1, 0)   # longer than the render
RAMP_ENDS = ((1 << 24) + 1000, 1, 0)    # ends inside the window across 2^24
TINY36 = float(np.float32(2.0 ** -13 * (1 + 2.0 ** -23)))  # lsb 2^-36: neither INT nor 32.32

FUSED_BATCHES = {
    # five voices: a block of four and a ragged one.  A block takes the path its finest f needs.
    "osc_int": [("osc", f) for f in (10.0, 440.0, 12345.0, 47999.0, 20000.0)],
    "osc_fx32": [("osc", f) for f in (20.125, 440.5, dc.f32(12345.678), -3.25, 47999.5)],
    "osc_f64": [("osc", f) for f in (440.5, dc.f32(12345.678), TINY36, -3.25, dc.f32(3 * TINY36))],
    "ramp_long": [("ramp", f, RAMP_LONG) for f in (20.125, 440.5, dc.f32(12345.678), -3.25, 440.0)],
    "ramp_ends": [("ramp", f, RAMP_ENDS) for f in (20.125, 440.5, dc.f32(12345.678), -3.25, 440.0)],
    "gain": [("gain", f, 0.25 + k / 16) for k, f in enumerate((20.125, 440.5, dc.f32(12345.678), -3.25, 440.0))],
}


def _unified(vs, sr):
    import dusp_amd as d
    from dusp_amd import descriptor
    d.configure(sr)
    exs = [descriptor.extract(dc.unit_of(v)[0]) for v in vs]
    osc_unit = [type(u).__name__ for u in exs[0].circuit.units].index("Osc")
    return descriptor.unify(exs), osc_unit


@pytest.mark.parametrize("batch", sorted(FUSED_BATCHES))
def test_fused_voices_past_two_to_the_24_equal_the_model(batch):
    sr, n, vs = 48000, DEEP_N, FUSED_BATCHES[batch]
    uni, osc_unit = _unified(vs, sr)
    prog = _ctx(sr).build(uni.words)
    assert prog.engine == "fused", (prog.engine, prog.shape)
    params = torch.from_numpy(np.ascontiguousarray(uni.params, dtype=np.float32)).cuda()
    out = torch.full((len(vs) * n + GUARD,), NAN, dtype=torch.float32, device="cuda")
    prog.render_device(n, len(vs), params.data_ptr(), out.data_ptr(), _stream())
    torch.cuda.synchronize()
    assert bool(torch.isnan(out[len(vs) * n:]).all())
    for i, v in enumerate(vs):
        for first, count in DEEP_WINDOWS:
            got = out[i * n + first:i * n + first + count].cpu().numpy()
            want = ev.outlet(dt.voice_window(v, sr, first, count))
            same = got.view(np.uint32) == want.view(np.uint32)
            assert same.all(), (batch, v, "first wrong sample", first + int(np.flatnonzero(~same)[0]))
        assert prog.state(osc_unit, i)[0] == dt.end_phase(v[1], sr, dt.whole_chunks(n)), (batch, v)
    prog.close()
    del out


WAVE_VOICES = {
    "osc": ("osc", dc.f32(12345.678)),
    "ramp_long": ("ramp", 440.5, RAMP_LONG),
    "ramp_ends": ("ramp", -3.25, RAMP_ENDS),
    "gain": ("gain", 20.125, 0.625),
}


@pytest.mark.parametrize("kernel", ["compiled", "interpreter"])
@pytest.mark.parametrize("name", sorted(WAVE_VOICES))
def test_one_wave_engine_voice_cut_in_time_past_two_to_the_24_equals_the_model(name, kernel):
    """One instance on ENGINE_WAVE: the planner cuts the render into time segments, each of which jumps to its first sample."""
    from dusp_amd import runtime
    sr, n, v = 48000, DEEP_N, WAVE_VOICES[name]
    words, osc_units = dc.chain([v], sr)
    ctx = _ctx(sr) if kernel == "compiled" else knob_context(sr, DUSP_WAVE_JIT=0)
    prog = ctx.build(words, runtime.ENGINE_WAVE)
    assert prog.engine == "wave"
    out = torch.full((n + GUARD,), NAN, dtype=torch.float32, device="cuda")
    prog.render_device(n, 1, None, out.data_ptr(), _stream())
    torch.cuda.synchronize()
    assert ("compiled kernel" in prog.read_shape()) == (kernel == "compiled"), prog.shape
    assert bool(torch.isnan(out[n:]).all())
    for first, count in DEEP_WINDOWS:
        got = out[first:first + count].cpu().numpy()
        want = ev.outlet(dt.voice_window(v, sr, first, count))
        same = got.view(np.uint32) == want.view(np.uint32)
        assert same.all(), (name, kernel, "first wrong sample", first + int(np.flatnonzero(~same)[0]))
    assert prog.state(osc_units[0])[0] == dt.end_phase(v[1], sr, dt.whole_chunks(n))
    prog.close()
    del out


def _oracle_circuit(which):
    import dusp_amd as d
    d.configure(48000)
    if which == "fm_pair":       # increments within 220.5 +- 40: the render is cut in time
        return d.Osc(d.Sum(d.Multiply(d.Osc(5), 40), 220.5))
    if which == "timer_times_k":
        return d.Multiply(d.Timer(), 0.625)
    if which == "osc_shape_400s":
        return d.Multiply(d.Osc(440.5), d.Shape("decay", 400, 0.25, 1).trigger())
    raise KeyError(which)


@pytest.mark.parametrize("which", ["fm_pair", "timer_times_k", "osc_shape_400s"])
def test_circuits_past_two_to_the_24_equal_the_oracles_sequential_render(which, oracle):
    """An FM pair and Multiply(Timer, k) on the compiled kernel, mul(osc, shape) with a Shape of 400 s on the fused kernel: one instance,
    windows and end state against the oracle walking there sample by sample."""
    from dusp_amd import descriptor
    sr, n = 48000, DEEP_N
    ex = descriptor.extract(_oracle_circuit(which))
    want, states = oracle.render(ex.words, n, max_channels=1, return_state=True)
    prog = _ctx(sr).build(ex.words)
    out = torch.full((n + GUARD,), NAN, dtype=torch.float32, device="cuda")
    prog.render_device(n, 1, None, out.data_ptr(), _stream())
    torch.cuda.synchronize()
    shape = prog.read_shape()
    assert (prog.engine == "fused") if which == "osc_shape_400s" else ("compiled kernel" in shape), (prog.engine, shape)
    assert bool(torch.isnan(out[n:]).all())
    for first, count in DEEP_WINDOWS:
        got = out[first:first + count].cpu().numpy()
        same = got.view(np.uint32) == want[0, first:first + count].view(np.uint32)
        assert same.all(), (which, "first wrong sample", first + int(np.flatnonzero(~same)[0]))
    for u in range(prog.n_units):
        assert np.array_equal(prog.state(u), states[u], equal_nan=True), (which, u, prog.state(u), states[u])
    prog.close()
    del out


# ------------------------------------------------------------------ d. refusals
def test_windows_and_renders_outside_the_served_range_are_refused_before_any_launch():
    """Every window with first_sample a multiple of 2048 up to 2^40 and up to 65535 blocks of samples is served exactly; what lies outside
    is refused by name, before anything is launched (the buffer here is far too small for what is asked)."""
    from dusp_amd import runtime
    sr = 48000
    prog = _ctx(sr).build(dc.chain(dc.voices("frac", 0, sr), sr)[0])
    out = torch.full((4096,), NAN, dtype=torch.float32, device="cuda")
    most = 65535 * 2048
    with pytest.raises(ValueError) as e:
        prog.render_chain_window((1 << 40) + 2048, 2048, None, False, out.data_ptr(), _stream())
    assert str(e.value) == "dusp-hip: first_sample of a chain window must be in 0 .. 2^40, not %d" % ((1 << 40) + 2048)
    with pytest.raises(ValueError) as e:
        prog.render_chain_window(-2048, 2048, None, False, out.data_ptr(), _stream())
    assert str(e.value) == "dusp-hip: first_sample of a chain window must be in 0 .. 2^40, not -2048"
    with pytest.raises(ValueError) as e:
        prog.render_chain_window(0, most + 1, None, False, out.data_ptr(), _stream())
    assert str(e.value) == "dusp-hip: n_samples of a chain window must be in 1 .. 134215680 (65535 blocks of 2048 samples), not 134215681"
    # the library's own refusals, for callers of the C ABI
    L = prog._L
    assert L.dusp_render_chain_window(prog._h, (1 << 40) + 2048, 2048, None, 0, out.data_ptr(), _stream()) < 0
    assert L.dusp_last_error(prog.ctx._h).decode() == "dusp_render_chain_window: first_sample must be at most 2^40"
    with pytest.raises(runtime.DuspHipError) as e:
        prog.render_device(most + 1, 1, None, out.data_ptr(), _stream())
    assert e.value.message == ("render: too many samples for the fused sum chain (at most 65535 blocks of 2048 samples: 134215680 samples a launch); "
                               "use DUSP_ENGINE_CHUNK")
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    prog.close()
