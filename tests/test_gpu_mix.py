"""The mix of a batch on the device (dusp_mix_device, dusp_render_host_mix): bit for bit the numpy statement of the contract
(dusp_amd/mix.py mix_chain — Sum.many's left-deep chain, one f32 rounding per add).  The kernel tests feed seeded tensors and need
no render; the render tests hold Program.render_mix to mix_chain over the SAME program's render(), whatever the voice's tolerance
against the oracle, and — for voices the device renders bit for bit — to the oracle's render of Sum.many as one circuit."""
import functools

import numpy as np
import pytest

import dusp_amd as d
from conftest import knob_context
from dusp_amd import descriptor, render, runtime, wav
from dusp_amd.mix import mix_chain
from mix_voices import KINDS, voice

pytestmark = pytest.mark.gpu

# (instances, channels, samples): one sample; rows off every 16-byte phase; remainders of the 8-deep instance loop (1, 2, 3, 9, 17);
# more than 32 channels; several workgroups; rows of whole float4s — and one wide enough for the float4 form by the launcher's own choice
SHAPES = [(1, 1, 1), (2, 1, 255), (3, 2, 257), (9, 1, 1001), (17, 3, 513), (5, 33, 300), (300, 1, 4099), (64, 2, 4096), (5, 2, 131076)]
VARIANTS = ["plain", "gains", "init", "in_place", "offsets"]
GUARD = 64  # floats in front of and behind the output (a multiple of 4: the output's 16-byte phase is the offset's)
SENTINEL = np.float32(-12345.678)
FMAX = np.finfo(np.float32).max
PLANTED = [0.0, -0.0, np.inf, -np.inf, FMAX, -FMAX, 1e-45, -1e-40, 5e-39, 1.0, -1.0]


@functools.lru_cache(maxsize=None)
def batch(shape, special=None):
    """Seeded planar PCM: normal samples, the instances' scales spanning 1e-3 .. 1e3; planted in it signed zeros, infinities, the
    largest f32, subnormals and pairs that cancel in neighbouring instances, and one position where every instance holds -0.
    special "nan": no infinities (so that every NaN of the mix is a planted one) and NaNs at known positions."""
    n_inst, n_ch, n = shape
    rng = np.random.RandomState(n_inst * 100003 + n_ch * 1009 + n)
    x = rng.standard_normal(shape).astype(np.float32)
    x *= np.logspace(-3, 3, n_inst, dtype=np.float32)[:, None, None] if n_inst > 1 else np.float32(1)
    rows = x.reshape(n_inst, -1)
    row = rows.shape[1]
    vals = [v for v in PLANTED if special != "nan" or np.isfinite(v) and abs(v) < FMAX]
    spots = rng.choice(row, min(row, 3 * len(vals)), replace=False)
    for j, p in enumerate(spots[:len(vals)]):
        rows[rng.randint(n_inst), p] = vals[j]
    if n_inst > 1:
        for j, p in enumerate(spots[len(vals):2 * len(vals)]):  # v then -v: the chain passes through an exact cancellation
            i = rng.randint(n_inst - 1)
            rows[i, p] = vals[j]
            rows[i + 1, p] = -np.float32(vals[j])
    if row > 4:
        rows[:, spots[-1]] = -0.0
    nan_at = None
    if special == "nan":
        nan_at = np.unique(rng.choice(row, min(row, 5), replace=False))
        for p in nan_at:
            rows[rng.randint(n_inst), p] = np.nan
    x.setflags(write=False)
    return x, nan_at


@functools.lru_cache(maxsize=None)
def gains_of(n_inst):
    g = (0.05 + 1.9 * np.random.RandomState(n_inst).random_sample(n_inst)).astype(np.float32)
    g[n_inst // 2] = 1.0
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def init_of(shape):
    """a second seeded buffer [channels, samples] to continue from: a partial sum as a raw mix leaves it (a -0 and an infinity included)"""
    rng = np.random.RandomState(shape[1] * 7919 + shape[2])
    a = (30 * rng.standard_normal(shape[1:])).astype(np.float32)
    a.reshape(-1)[rng.choice(a.size, min(a.size, 2), replace=False)] = [-0.0, np.inf][:min(a.size, 2)]
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def expected(shape, special, with_gains, with_init, raw):
    x, _ = batch(shape, special)
    want = mix_chain(x, gains_of(shape[0]) if with_gains else None, init_of(shape) if with_init else None, raw)
    want.setflags(write=False)
    return want


def same(got, want, what):
    """bit patterns; for NaN, the positions"""
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what
    g, w = got.view(np.uint32)[~nan], want.view(np.uint32)[~nan]
    assert np.array_equal(g, w), "%s: first differing sample %d of %d" % (what, int(np.argmax(g != w)), g.size)


def run_mix(ctx, shape, special=None, with_gains=False, init=None, raw=False, out_offset=0, in_offset=0):
    """init: None | "buffer" | "in_place".  out_offset / in_offset: floats past a 16-byte boundary."""
    import torch
    x, _ = batch(shape, special)
    n_inst, n_ch, n = shape
    row = n_ch * n
    d_in = torch.zeros(in_offset + x.size, dtype=torch.float32, device="cuda")
    d_in[in_offset:] = torch.from_numpy(np.array(x).reshape(-1)).cuda()
    d_out = torch.full((GUARD + out_offset + row + GUARD,), float(SENTINEL), dtype=torch.float32, device="cuda")
    lo = GUARD + out_offset
    assert d_out.data_ptr() % 16 == 0 and d_in.data_ptr() % 16 == 0
    d_gains = torch.from_numpy(np.array(gains_of(n_inst))).cuda() if with_gains else None
    d_init, p_init = None, None
    if init == "in_place":
        d_out[lo:lo + row] = torch.from_numpy(np.array(init_of(shape)).reshape(-1)).cuda()
        p_init = d_out.data_ptr() + 4 * lo
    elif init == "buffer":
        d_init = torch.from_numpy(np.array(init_of(shape)).reshape(-1)).cuda()
        p_init = d_init.data_ptr()
    stream = torch.cuda.current_stream().cuda_stream
    torch.cuda.synchronize()
    ctx.mix(d_in.data_ptr() + 4 * in_offset, n_inst, n_ch, n, d_out.data_ptr() + 4 * lo, d_gains.data_ptr() if with_gains else None, p_init, raw, stream)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    what = (shape, special, with_gains, init, raw, out_offset, in_offset)
    assert np.array_equal(out[:lo].view(np.uint32), np.full(lo, SENTINEL).view(np.uint32)), "floats in front of the output were written: %r" % (what,)
    assert np.array_equal(out[lo + row:].view(np.uint32), np.full(GUARD, SENTINEL).view(np.uint32)), "floats behind the output were written: %r" % (what,)
    assert np.array_equal(d_in[in_offset:].cpu().numpy().view(np.uint32), x.reshape(-1).view(np.uint32)), "the input was written to"
    if d_init is not None:
        assert np.array_equal(d_init.cpu().numpy().view(np.uint32), init_of(shape).reshape(-1).view(np.uint32)), "d_init was written to"
    got = out[lo:lo + row].reshape(n_ch, n)
    same(got, expected(shape, special, with_gains, init is not None, bool(raw)), what)
    return got


# the launcher's own choice (every shape but the last: one float a lane, 32 rows in flight; the last: four floats a lane), four floats
# a lane wherever bases and row length allow 16-byte accesses, and one float a lane with 8 rows in flight (what a wide grid of odd rows takes)
FORMS = {"by_grid": {}, "float4": {"DUSP_MIX_WIDTH": 4}, "dword8": {"DUSP_MIX_WIDTH": 1, "DUSP_MIX_DEPTH": 8}}


def mix_context(form):
    return knob_context(48000, **FORMS[form]) if FORMS[form] else render.context(48000)


@pytest.mark.parametrize("width", list(FORMS))
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_mix_device_equals_the_chain(shape, variant, width):
    ctx = mix_context(width)
    for raw in (0, 1):
        if variant == "plain":
            run_mix(ctx, shape, raw=raw)
        elif variant == "gains":
            run_mix(ctx, shape, with_gains=True, raw=raw)
        elif variant == "init":
            run_mix(ctx, shape, with_gains=True, init="buffer", raw=raw)
            run_mix(ctx, shape, init="buffer", raw=raw)
        elif variant == "in_place":
            run_mix(ctx, shape, init="in_place", raw=raw)
            run_mix(ctx, shape, with_gains=True, init="in_place", raw=raw, out_offset=3)
        else:  # the output 4, 8 and 12 bytes past a 16-byte boundary; the input too
            for off in (1, 2, 3):
                run_mix(ctx, shape, with_gains=bool(off & 1), init="buffer" if off == 2 else None, raw=raw, out_offset=off)
            run_mix(ctx, shape, raw=raw, in_offset=1)
            run_mix(ctx, shape, raw=raw, out_offset=2, in_offset=2)


def test_planted_values_do_what_the_chain_says():
    """What the batches are built to hold: -0 survives a raw chain of -0s and leaves as +0 otherwise, cancelling pairs and infinities
    are in the expected mix (so the device met them)."""
    shape = (17, 3, 513)
    x, _ = batch(shape)
    raw, cooked = expected(shape, None, False, False, True), expected(shape, None, False, False, False)
    zero = (raw == 0)
    assert (np.signbit(raw) & zero).any() and not (np.signbit(cooked) & (cooked == 0)).any()
    assert np.isinf(raw).any() and (np.abs(x.reshape(17, -1)) < 1.2e-38).any() and (x == FMAX).any()
    assert (x[:-1] == -x[1:]).any()


@pytest.mark.parametrize("width", list(FORMS))
@pytest.mark.parametrize("shape", [(3, 2, 257), (17, 3, 513), (64, 2, 4096)], ids=lambda s: "x".join(map(str, s)))
def test_nan_travels_through_a_raw_mix_and_leaves_as_zero_otherwise(shape, width):
    ctx = mix_context(width)
    _, nan_at = batch(shape, "nan")
    for with_gains in (False, True):
        raw = run_mix(ctx, shape, "nan", with_gains, raw=1)
        assert np.array_equal(np.flatnonzero(np.isnan(raw.reshape(-1))), nan_at)
        cooked = run_mix(ctx, shape, "nan", with_gains, raw=0)
        assert not np.isnan(cooked).any() and (cooked.reshape(-1)[nan_at].view(np.uint32) == 0).all()


def test_mix_device_argument_errors_are_messages():
    import torch
    ctx = render.context(48000)
    buf = torch.zeros(4096, dtype=torch.float32, device="cuda")
    p = buf.data_ptr()
    for call, needle in [
        (lambda: ctx.mix(None, 2, 1, 8, p + 8192), "NULL"),
        (lambda: ctx.mix(p, 2, 1, 8, None), "NULL"),
        (lambda: ctx.mix(p, 0, 1, 8, p + 8192), "instances"),
        (lambda: ctx.mix(p, (1 << 24) + 1, 1, 8, p + 8192), "instances"),
        (lambda: ctx.mix(p, 2, 65, 8, p + 8192), "1..64 channels"),
        (lambda: ctx.mix(p, 2, 0, 8, p + 8192), "1..64 channels"),
        (lambda: ctx.mix(p, 2, 1, 0, p + 8192), "samples"),
        (lambda: ctx.mix(p, 2, 1, (1 << 31) + 1, p + 8192), "samples"),
        (lambda: ctx.mix(p, 2, 1, 8, p + 8194), "4-byte aligned"),
        (lambda: ctx.mix(p + 1, 2, 1, 8, p + 8192), "4-byte aligned"),
    ]:
        with pytest.raises(runtime.DuspHipError, match=needle) as e:
            call()
        assert e.value.status == -1


# ---- dusp_render_host_mix ---------------------------------------------------------------------------------------------------

N_SAMPLES = 1357
ENGINES = {"auto": runtime.ENGINE_AUTO, "chunk": runtime.ENGINE_CHUNK, "wave": runtime.ENGINE_WAVE}
FORMATS = {"s16": 16, "s24": 24, "f32": 32}


@functools.lru_cache(maxsize=None)
def unified(kind, n):
    d.configure(48000)
    return descriptor.unify([descriptor.extract(voice(kind, k)) for k in range(n)])


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("n", [1, 2, 37, 65])
@pytest.mark.parametrize("engine", list(ENGINES))
@pytest.mark.parametrize("kind", list(KINDS))
def test_render_mix_is_the_chain_over_the_programs_own_render(kind, engine, n, oracle):
    """The contract: render_mix == mix_chain(render()), with and without gains, whatever the tile; a plain render afterwards is what it
    was before; unit state is refused right after a mix.  Voices the device renders bit for bit also equal the oracle's Sum.many."""
    uni = unified(kind, n)
    prog = render.context(48000).build(uni.words, ENGINES[engine])
    if engine == "auto" and kind == "osc":
        assert prog.engine == "fused", prog.engine
    planar = prog.render(N_SAMPLES, n, uni.params)
    assert planar.shape[1] == (2 if kind == "pan" else 1)
    gains = gains_of(n)
    want, want_g = mix_chain(planar), mix_chain(planar, gains)
    got = prog.render_mix(N_SAMPLES, n, uni.params)
    assert got.dtype == np.float32 and got.shape == want.shape
    assert np.array_equal(bits(got), bits(want)), "first differing sample %d" % int(np.argmax((got != want).any(axis=0)))
    with pytest.raises(runtime.DuspHipError, match="last render was a mix") as e:
        prog.state(0)
    assert e.value.status == -4  # DUSP_ERR_STATE
    for tile in sorted({1, 3, 64, n}):  # tiles of one instance, ragged last tiles, one tile: the same bytes
        assert np.array_equal(bits(prog.render_mix(N_SAMPLES, n, uni.params, tile_instances=tile)), bits(want)), tile
        assert np.array_equal(bits(prog.render_mix(N_SAMPLES, n, uni.params, gains, tile_instances=tile)), bits(want_g)), tile
    again = prog.render(N_SAMPLES, n, uni.params)
    assert np.array_equal(bits(again), bits(planar)), "a render after a mix differs from the one before it"
    if kind in ("bright_saw", "feedback") and engine == "wave":  # (what these two are here for: the scan's bits across tiles and launch geometries)
        assert prog.read_shape().endswith(", scan"), prog.read_shape()
    prog.state(0)  # ... and the state is there again
    if n == 37:
        once = planar.astype(np.float64).sum(axis=0).astype(np.float32)
        assert float(np.mean(once != want)) >= 0.5  # (the voices keep the test order-sensitive)
    if KINDS[kind]:
        d.configure(48000)
        ref = np.asarray(oracle.render(descriptor.extract(d.Sum.many([voice(kind, k) for k in range(n)])).words, N_SAMPLES), dtype=np.float32)
        assert np.array_equal(bits(got), bits(ref)), "differs from the oracle's Sum.many at sample %d" % int(np.argmax((got != ref).any(axis=0)))
    prog.close()


def scan_voice(k):
    """A structure no other test of the session renders (the session's code-object cache has no kernel for it), scan-eligible:
    two oscillators into a Filter whose cutoff column lies wholly above the scan's lower bound."""
    return d.Filter(d.Sum(d.Osc(110 + 3.25 * k, "saw"), d.Multiply(d.Osc(55 + k, "triangle"), 0.25)), 2400 + 35 * k)


def test_a_mix_under_the_default_jit_knob_runs_every_tile_on_the_compiled_kernel():
    """DUSP_WAVE_JIT=1, the product default: a plain short render of a new structure runs on the interpreter — the Filter stage's
    arithmetic — while its kernel compiles, and later ones on the kernel, whose Filter is a scan: within the scan's bound of each
    other, not the same bits.  A mix that did the same would sum tiles of both kinds, split wherever the compile finished.  It
    waits for the kernel instead: whatever the tile, the bytes are mix_chain over the render of a context that always waits
    (DUSP_WAVE_JIT=2, rendered AFTER the mixes so that the kernel is not at hand when the first mix starts)."""
    n = 37
    d.configure(48000)
    uni = descriptor.unify([descriptor.extract(scan_voice(k)) for k in range(n)])
    prog = knob_context(48000, DUSP_WAVE_JIT=1).build(uni.words, runtime.ENGINE_WAVE)
    mixes = {tile: prog.render_mix(N_SAMPLES, n, uni.params, tile_instances=tile) for tile in (3, 1, n, 0)}
    assert prog.read_shape().endswith(", scan"), prog.read_shape()
    prog.close()
    ref = render.context(48000).build(uni.words, runtime.ENGINE_WAVE)
    planar = ref.render(N_SAMPLES, n, uni.params)
    assert ref.read_shape().endswith(", scan"), ref.read_shape()
    ref.close()
    want = mix_chain(planar)
    for tile, got in mixes.items():
        assert np.array_equal(bits(got), bits(want)), "tiles of %d: first differing sample %d" % (tile, int(np.argmax((got != want).any(axis=0))))


def test_tiles_decide_on_warming_segments_as_the_whole_batch_does():
    """A few long instances of a feed-forward Filter voice render in segments that warm up, on the Filter stage; a batch beyond 8
    instances a CU renders unsplit, its Filter a scan — not the same bits.  A tile of such a batch is few instances: it must still
    render as the batch does.  (The first assertion keeps the case meaningful: the tile's instances, rendered alone, do warm up.)"""
    import torch
    n = 8 * torch.cuda.get_device_properties(0).multi_processor_count + 1
    n_samples, tile = 32 * 256 + 77, 1024
    d.configure(48000)
    uni = descriptor.unify([descriptor.extract(d.Filter(d.Osc(110 + k / 8, "saw"), 3000)) for k in (0, 1)])
    params = np.ascontiguousarray((110 + np.arange(n, dtype=np.float64) / 8).astype(np.float32).reshape(1, n))
    assert uni.params.shape == (1, 2) and np.array_equal(uni.params, params[:, :2])
    prog = render.context(48000).build(uni.words, runtime.ENGINE_WAVE)
    prog.render(n_samples, tile, np.ascontiguousarray(params[:, :tile]))
    assert " seg" in prog.read_shape(), prog.read_shape()
    planar = prog.render(n_samples, n, params)
    assert prog.read_shape().endswith(", scan"), prog.read_shape()
    want = mix_chain(planar)
    for t in (tile, 0):
        got = prog.render_mix(n_samples, n, params, tile_instances=t)
        assert np.array_equal(bits(got), bits(want)), "tiles of %d: first differing sample %d" % (t, int(np.argmax((got != want).any(axis=0))))
    prog.close()


@pytest.mark.parametrize("kind", ["pan", "feedback"])
def test_render_mix_pcm_delivery(kind):
    """s16 / s24 / f32 frames and the peak of the MIX: wav.encode_frames over the f32 mix, for every normalise mode."""
    n = 37
    uni = unified(kind, n)
    prog = render.context(48000).build(uni.words)
    mix = prog.render_mix(N_SAMPLES, n, uni.params, tile_instances=16)
    assert float(np.abs(mix).max()) > 1.0  # (37 voices: normalise = 1 has something to shrink)
    for fmt, depth in FORMATS.items():
        for normalise in (0, 1, 2):
            data, peak = prog.render_mix(N_SAMPLES, n, uni.params, tile_instances=16, format=fmt, normalise=normalise)
            want, want_peak = wav.encode_frames(mix, depth, normalise)
            assert data.dtype == want.dtype and data.shape == want.shape, (fmt, data.shape, want.shape)
            assert np.array_equal(data.view(np.uint8), want.view(np.uint8)), (fmt, normalise)
            assert np.float32(peak).view(np.uint32) == np.float32(want_peak).view(np.uint32)
    prog.close()


def test_render_mix_refusals():
    d.configure(48000)
    ctx = render.context(48000)
    noisy = ctx.build(descriptor.extract(d.Multiply(d.HostSource(np.zeros(64, dtype=np.float32)), 0.5)).words)
    assert noisy.n_inputs == 1
    with pytest.raises(runtime.DuspHipError, match="input streams") as e:
        noisy.render_mix(64, 1)
    assert e.value.status == -2
    noisy.close()
    uni = unified("fm", 2)
    resumable = ctx.build(uni.words, runtime.ENGINE_AUTO | runtime.ENGINE_RESUMABLE)
    with pytest.raises(runtime.DuspHipError, match="resumable"):
        resumable.render_mix(64, 2, uni.params)
    resumable.close()
    prog = ctx.build(uni.words)
    with pytest.raises(ValueError, match="gains must have shape"):
        prog.render_mix(64, 2, uni.params, gains=[1.0, 2.0, 3.0])
    with pytest.raises(ValueError, match="params must have shape"):
        prog.render_mix(64, 3, uni.params)
    with pytest.raises(runtime.DuspHipError, match="n_instances") as e:
        prog.ctx._check(prog._L.dusp_render_host_mix(prog._h, 0, 64, uni.params.ctypes.data, None, 0, 0, 0, np.empty(64, np.float32).ctypes.data, None))
    assert e.value.status == -1
    with pytest.raises(ValueError, match="format"):  # (refused in front of the library, as render_pcm does ...)
        prog.render_mix(64, 2, uni.params, format=7)
    with pytest.raises(runtime.DuspHipError, match="format") as e:  # ... and by the library itself
        prog.ctx._check(prog._L.dusp_render_host_mix(prog._h, 2, 64, uni.params.ctypes.data, None, 0, 7, 0, np.empty(64, np.float32).ctypes.data, None))
    assert e.value.status == -1
    with pytest.raises(ValueError, match="normalise"):
        prog.render_mix(64, 2, uni.params, format="s16", normalise=3)
    prog.close()


def test_render_py_surface():
    """render_mix / render_mix_pcm / render_mix_wav: what renderChannelData(Sum.many(voices)) computes, as ChannelData, frames and a file."""
    d.configure(48000)
    dur, n = 0.02, 9
    voices = lambda: [voice("fm", k) for k in range(n)]
    ref = d.renderChannelData(d.Sum.many(voices()), dur)
    mix = render.render_mix(voices(), dur)
    assert mix.sampleRate == 48000 and len(mix) == 1 and np.array_equal(bits(mix[0]), bits(np.asarray(ref[0])))
    gains = gains_of(n)
    ref_g = d.renderChannelData(d.Sum.many([d.Multiply(v, float(g)) for v, g in zip(voices(), gains)]), dur)
    assert np.array_equal(bits(render.render_mix(voices(), dur, gains, tile_instances=4)[0]), bits(np.asarray(ref_g[0])))
    planar = np.stack([np.asarray(c) for c in ref])
    for depth in (16, 24, 32):
        res = render.render_mix_pcm(voices(), dur, depth, 2)
        want, peak = wav.encode_frames(planar, depth, 2)
        assert np.array_equal(res.data.view(np.uint8), want.view(np.uint8)) and res.peak == peak and res.bitDepth == depth and res.numberOfChannels == 1
        assert render.render_mix_wav(voices(), dur, depth) == wav.encode_wav(ref, 48000, depth)
    assert len(render.render_mix(voices(), 0)) == 0
