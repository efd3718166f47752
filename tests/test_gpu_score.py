"""Scores on the device (dusp_score_device, dusp_render_host_score): voices mixed at per-voice onsets into a timeline longer than a
voice, bit for bit the numpy statement of the contract (dusp_amd/mix.py score_chain).  The kernel tests feed seeded tensors and need no
render; the render tests hold Program.render_score to score_chain over the SAME program's render(), whatever the voice's tolerance
against the oracle, and — for the score voice, which the device renders bit for bit — to the oracle's render of
Sum.many(Delay(voice_k, onset_k, 4096)) as one circuit."""
import functools
import struct

import numpy as np
import pytest

import dusp_amd as d
import mix_voices
import score_voices as sv
from conftest import knob_context
from dusp_amd import descriptor, render, runtime, wav
from dusp_amd.mix import score_chain

pytestmark = pytest.mark.gpu

GUARD = 64  # floats in front of and behind the output
SENTINEL = np.float32(-12345.678)
FMAX = np.finfo(np.float32).max
PLANTED = [0.0, -0.0, np.inf, -np.inf, FMAX, -FMAX, 1e-45, -1e-40, 5e-39, 1.0, -1.0, np.nan]

# (voices, channels, voice samples, timeline samples): one sample of everything; timelines and voices at every residue mod 4; 9 and 37
# voices (no multiples of the kernel's depth of 8); one and two channels; a timeline of several workgroups and one shorter than a voice
CASES = [(1, 1, 1, 1), (2, 1, 255, 300), (9, 2, 257, 1023), (13, 2, 300, 2049), (37, 1, 773, 2317), (37, 2, 254, 1022), (9, 1, 1001, 600)]
VARIANTS = ["plain", "gains", "init", "in_place", "offsets"]
# the kernel has one form (one float a lane, 8 entries in flight; with and without gains); what the launcher varies beyond that is the
# block of the plan: 256 samples by default, doubled under a small byte budget until one block covers the timeline
FORMS = {"block256": {}, "doubled_blocks": {"DUSP_SCORE_PLAN_KB": 1}}


def score_context(form):
    return knob_context(48000, **FORMS[form]) if FORMS[form] else render.context(48000)


@functools.lru_cache(maxsize=None)
def batch(case):
    """-> voices, onsets, lengths, gains, init, covered (the timeline samples some voice covers).  Seeded voices (scales spanning 1e-3 .. 1e3, planted signed zeros, infinities, the largest f32, subnormals and a NaN), onsets of
    both signs and every residue mod 4 — in front of the timeline, on and next to block boundaries, straddling its end, past it — and
    lengths that include 0, 1 and the whole voice (spans end inside a 16-byte unit, inside a block and on a block boundary)."""
    n, n_ch, nv, nt = case
    rng = np.random.RandomState(n * 100003 + n_ch * 1009 + nv * 31 + nt)
    x = rng.standard_normal((n, n_ch, nv)).astype(np.float32)
    x *= np.logspace(-3, 3, n, dtype=np.float32)[:, None, None] if n > 1 else np.float32(1)
    flat = x.reshape(-1)
    for j, p in enumerate(rng.choice(flat.size, min(flat.size, len(PLANTED)), replace=False)):
        flat[p] = PLANTED[j]
    if nv > 4:
        x[:, :, 3] = -0.0
    onsets = rng.randint(-nv, nt + 2, n).astype(np.int64)
    lengths = rng.randint(0, nv + 1, n).astype(np.int64)
    for k in range(n):
        kind = k % 9
        if kind == 1:
            onsets[k] = 256 * rng.randint(0, max(1, nt // 256) + 1) - (k % 4)  # next to a block boundary
        elif kind == 2 and nv <= 256:
            onsets[k], lengths[k] = 256 * rng.randint(0, max(1, nt // 256)) + 256 - nv, nv  # the span ends ON a block boundary
        elif kind == 3:
            lengths[k] = nv
        elif kind == 4:
            lengths[k] = min(1, nv)
        elif kind == 5:
            lengths[k] = 0
        elif kind == 6:
            onsets[k] = (1 << 62) * (1 if k % 2 else -1)
    if n > 2:
        onsets[0], lengths[0] = nt - min(nv, 3), nv  # straddles the end
    gains = (0.05 + 1.9 * rng.random_sample(n)).astype(np.float32)
    if n > 2:
        gains[1] = -gains[1]
    init = (30 * rng.standard_normal((n_ch, nt))).astype(np.float32)
    init.reshape(-1)[rng.choice(init.size, min(init.size, 3), replace=False)] = [-0.0, np.inf, np.nan][:min(init.size, 3)]
    covered = np.zeros(nt, dtype=bool)
    for k in range(n):
        covered[max(int(onsets[k]), 0):max(int(min(onsets[k], nt) + lengths[k]), 0)] = True
    if (~covered).any():
        init[:, np.flatnonzero(~covered)[-1]] = -0.0  # a -0 partial sum where no voice of this batch comes: a raw chain keeps it
    for a in (x, onsets, lengths, gains, init, covered):
        a.setflags(write=False)
    return x, onsets, lengths, gains, init, covered


@functools.lru_cache(maxsize=None)
def expected(case, with_lengths, with_gains, with_init, raw):
    x, onsets, lengths, gains, init, _ = batch(case)
    want = score_chain(x, onsets, case[3], lengths if with_lengths else None, gains if with_gains else None, init if with_init else None, raw)
    want.setflags(write=False)
    return want


def same(got, want, what):
    """bit patterns; for NaN, the positions"""
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what
    g, w = got.view(np.uint32)[~nan], want.view(np.uint32)[~nan]
    assert np.array_equal(g, w), "%s: first differing sample %d of %d" % (what, int(np.argmax(g != w)), g.size)


def run_score(ctx, case, with_lengths=True, with_gains=False, init=None, raw=False, out_offset=0, in_offset=0):
    """init: None | "buffer" | "in_place".  out_offset / in_offset: floats past a 16-byte boundary."""
    import torch
    x, onsets, lengths, gains, init_host, _ = batch(case)
    n, n_ch, nv, nt = case
    row = n_ch * nt
    d_in = torch.zeros(in_offset + x.size, dtype=torch.float32, device="cuda")
    d_in[in_offset:] = torch.from_numpy(np.array(x).reshape(-1)).cuda()
    d_out = torch.full((GUARD + out_offset + row + GUARD,), float(SENTINEL), dtype=torch.float32, device="cuda")
    lo = GUARD + out_offset
    d_gains = torch.from_numpy(np.array(gains)).cuda() if with_gains else None
    d_init, p_init = None, None
    if init == "in_place":
        d_out[lo:lo + row] = torch.from_numpy(np.array(init_host).reshape(-1)).cuda()
        p_init = d_out.data_ptr() + 4 * lo
    elif init == "buffer":
        d_init = torch.from_numpy(np.array(init_host).reshape(-1)).cuda()
        p_init = d_init.data_ptr()
    stream = torch.cuda.current_stream().cuda_stream
    torch.cuda.synchronize()
    ctx.score_device(d_in.data_ptr() + 4 * in_offset, n, n_ch, nv, onsets, nt, d_out.data_ptr() + 4 * lo, lengths if with_lengths else None,
                     d_gains.data_ptr() if with_gains else None, p_init, raw, stream)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    what = (case, with_lengths, with_gains, init, raw, out_offset, in_offset)
    assert np.array_equal(out[:lo].view(np.uint32), np.full(lo, SENTINEL).view(np.uint32)), "floats in front of the output were written: %r" % (what,)
    assert np.array_equal(out[lo + row:].view(np.uint32), np.full(GUARD, SENTINEL).view(np.uint32)), "floats behind the output were written: %r" % (what,)
    assert np.array_equal(d_in[in_offset:].cpu().numpy().view(np.uint32), x.reshape(-1).view(np.uint32)), "the input was written to"
    if d_init is not None:
        assert np.array_equal(d_init.cpu().numpy().view(np.uint32), init_host.reshape(-1).view(np.uint32)), "d_init was written to"
    got = out[lo:lo + row].reshape(n_ch, nt)
    same(got, expected(case, with_lengths, with_gains, init is not None, bool(raw)), what)
    return got


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("case", CASES, ids=lambda s: "x".join(map(str, s)))
def test_score_device_equals_the_chain(case, variant, form):
    ctx = score_context(form)
    for raw in (0, 1):
        if variant == "plain":
            run_score(ctx, case, raw=raw)
            run_score(ctx, case, with_lengths=False, raw=raw)
        elif variant == "gains":
            run_score(ctx, case, with_gains=True, raw=raw)
        elif variant == "init":
            run_score(ctx, case, with_gains=True, init="buffer", raw=raw)
            run_score(ctx, case, init="buffer", raw=raw)
        elif variant == "in_place":
            run_score(ctx, case, init="in_place", raw=raw)
            run_score(ctx, case, with_gains=True, init="in_place", raw=raw, out_offset=3)
        else:  # the output 4, 8 and 12 bytes past a 16-byte boundary; the input too
            for off in (1, 2, 3):
                run_score(ctx, case, with_gains=bool(off & 1), init="buffer" if off == 2 else None, raw=raw, out_offset=off)
            run_score(ctx, case, raw=raw, in_offset=1)
            run_score(ctx, case, raw=raw, out_offset=2, in_offset=3)


def test_the_batches_hold_what_they_are_built_to_hold():
    """... so that the device met it: samples no voice covers (+0, or init with its -0 and NaN), -0 partial sums that survive a raw chain
    and leave as +0 otherwise, NaN and infinities in the expected timeline, voices on both sides of the timeline and far outside it."""
    case = (37, 2, 254, 1022)
    x, onsets, lengths, gains, init, covered = batch(case)
    raw, cooked = expected(case, True, False, True, True), expected(case, True, False, True, False)
    assert (~covered).any() and np.array_equal(raw[:, ~covered].view(np.uint32), init[:, ~covered].view(np.uint32))
    assert (np.signbit(raw) & (raw == 0)).any() and not (np.signbit(cooked) & (cooked == 0)).any()
    assert np.isnan(raw).any() and not np.isnan(cooked).any() and np.isinf(cooked).any()
    assert (onsets < 0).any() and (onsets >= case[3]).any() and (np.abs(onsets) == 1 << 62).any() and (lengths == 0).any() and (onsets + lengths > case[3]).any()
    assert {int(o) % 4 for o in onsets} == {0, 1, 2, 3}
    plain = expected(case, True, False, False, True)
    assert not plain[:, ~covered].any() and not np.signbit(plain[:, ~covered]).any()


def test_no_voices_is_the_copy_out_alone():
    import torch
    ctx = render.context(48000)
    init = np.array([[1.0, -0.0, np.nan, 0.0, -2.5, np.inf, 1e-45]], dtype=np.float32)
    d_buf = torch.from_numpy(init.reshape(-1).copy()).cuda()
    d_out = torch.full((7,), 9.0, dtype=torch.float32, device="cuda")
    ctx.score_device(None, 0, 1, 5, [], 7, d_out.data_ptr(), d_init=d_buf.data_ptr(), raw=True, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    same(d_out.cpu().numpy().reshape(1, 7), init, "raw: a copy")
    ctx.score_device(None, 0, 1, 5, [], 7, d_buf.data_ptr(), d_init=d_buf.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    same(d_buf.cpu().numpy().reshape(1, 7), score_chain(np.zeros((0, 1, 5), np.float32), [], 7, init=init), "in place: `|| 0`")
    ctx.score_device(None, 0, 1, 5, [], 7, d_out.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert not d_out.cpu().numpy().view(np.uint32).any()


def test_score_last_ms_times_the_launch_alone():
    """dusp_score_last_ms: the kernel by events around the launch, the plan's host time and its upload beside it; an error before the
    context's first score."""
    import torch
    fresh = runtime.Context(-1, 48000)
    with pytest.raises(runtime.DuspHipError, match="no dusp_score_device call") as e:
        fresh.score_last_ms()
    assert e.value.status == -4
    rows = torch.ones((4, 1, 1000), dtype=torch.float32, device="cuda")
    out = torch.zeros((1, 3000), dtype=torch.float32, device="cuda")
    fresh.score_device(rows.data_ptr(), 4, 1, 1000, [0, 500, 1000, 2500], 3000, out.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    kernel, plan, upload = fresh.score_last_ms()
    assert 0 < kernel < 1000 and 0 <= plan < 1000 and 0 <= upload < 1000, (kernel, plan, upload)
    assert out.cpu().numpy()[0].tolist() == [1.0] * 500 + [2.0] * 500 + [2.0] * 500 + [1.0] * 500 + [0.0] * 500 + [1.0] * 500
    fresh.score_device(None, 0, 1, 1000, [], 3000, out.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)  # no voices: no plan, no upload
    kernel, plan, upload = fresh.score_last_ms()
    assert 0 < kernel < 1000 and plan == 0 and upload == 0, (kernel, plan, upload)
    fresh.close()


def test_score_device_argument_errors_are_messages():
    import torch
    ctx = render.context(48000)
    buf = torch.zeros(4096, dtype=torch.float32, device="cuda")
    p, q = buf.data_ptr(), buf.data_ptr() + 8192
    on = [0, 1]
    for call, needle in [
        (lambda: ctx.score_device(None, 2, 1, 8, on, 16, q), "NULL"),
        (lambda: ctx.score_device(p, 2, 1, 8, on, 16, None), "NULL"),
        (lambda: ctx.score_device(p, (1 << 24) + 1, 1, 8, np.zeros((1 << 24) + 1, np.int64), 16, q), "instances"),
        (lambda: ctx.score_device(p, 2, 65, 8, on, 16, q), "1..64 channels"),
        (lambda: ctx.score_device(p, 2, 0, 8, on, 16, q), "1..64 channels"),
        (lambda: ctx.score_device(p, 2, 1, 0, on, 16, q), "samples"),
        (lambda: ctx.score_device(p, 2, 1, 8, on, 0, q), "samples"),
        (lambda: ctx.score_device(p, 2, 1, (1 << 31) + 1, on, 16, q), "samples"),
        (lambda: ctx.score_device(p, 2, 1, 8, on, (1 << 31) + 1, q), "samples"),
        (lambda: ctx.score_device(p, 2, 2, 8, on, (1 << 30) + 1, q), "channels x timeline samples must not exceed 2\\^31"),  # (sizes only: nothing is allocated or touched)
        (lambda: ctx.score_device(p, 2, 2, (1 << 30) + 1, on, 16, q), "channels x voice samples must not exceed 2\\^31"),
        (lambda: ctx.score_device(p, 2, 1, 8, on, 16, q + 2), "4-byte aligned"),
        (lambda: ctx.score_device(p + 1, 2, 1, 8, on, 16, q), "4-byte aligned"),
        (lambda: ctx.score_device(p, 2, 1, 8, on, 16, q, d_gains=p + 3), "4-byte aligned"),
        (lambda: ctx.score_device(p, 2, 1, 8, on, 16, q, lengths=[8, 9]), "length of voice 1 is 9"),
        (lambda: ctx.score_device(p, 2, 1, 8, on, 16, q, lengths=[-1, 8]), "length of voice 0 is -1"),
    ]:
        with pytest.raises(runtime.DuspHipError, match=needle) as e:
            call()
        assert e.value.status == -1
    for call in (lambda: ctx.score_device(p, 2, 1, 8, [0, 0.5], 16, q), lambda: ctx.score_device(p, 2, 1, 8, [0], 16, q),
                 lambda: ctx.score_device(p, 2, 1, 8, on, 16, q, lengths=[1.25, 2]), lambda: ctx.score_device(p, 2, 1, 8, [0, np.nan], 16, q)):
        with pytest.raises(ValueError, match="dusp-hip"):
            call()
    assert not buf.cpu().numpy().any()  # (nothing ran)


# ---- dusp_render_host_score ---------------------------------------------------------------------------------------------------

KINDS = ["score", "feedback", "filtered_saw", "pan"]
FORMATS = {"s16": 16, "s24": 24}


def make_voice(kind, k):
    return sv.voice(k) if kind == "score" else mix_voices.voice(kind, k)


@functools.lru_cache(maxsize=None)
def unified(kind, n):
    d.configure(sv.SAMPLE_RATE)
    return descriptor.unify([descriptor.extract(make_voice(kind, k)) for k in range(n)])


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def jit_context():
    return knob_context(sv.SAMPLE_RATE, DUSP_WAVE_JIT=2)


@pytest.mark.parametrize("n", [1, 13, 37])
@pytest.mark.parametrize("kind", KINDS)
def test_render_score_is_the_chain_over_the_programs_own_render(kind, n, oracle):
    """The contract: render_score == score_chain(render()), with and without lengths and gains, whatever the tile; a plain render
    afterwards is what it was before; unit state is refused right after a score.  The score voice also equals the oracle's
    Sum.many(Delay ...) circuit."""
    uni = unified(kind, n)
    prog = jit_context().build(uni.words)
    planar = prog.render(sv.NV, n, uni.params)
    assert planar.shape == (n, 2 if kind == "pan" else 1, sv.NV)
    onsets, lengths, gains = sv.layout(n)
    want, want_g = score_chain(planar, onsets, sv.NT, lengths), score_chain(planar, onsets, sv.NT, None, gains)
    got = prog.render_score(sv.NV, sv.NT, n, onsets, lengths, uni.params)
    assert got.dtype == np.float32 and got.shape == want.shape
    assert np.array_equal(bits(got), bits(want)), "first differing sample %d" % int(np.argmax((bits(got) != bits(want)).any(axis=0)))
    with pytest.raises(runtime.DuspHipError, match="last render was a mix") as e:
        prog.state(0)
    assert e.value.status == -4  # DUSP_ERR_STATE
    for tile in sorted({1, 3, 64, n}):  # tiles of one instance, ragged last tiles, one tile: the same bytes
        assert np.array_equal(bits(prog.render_score(sv.NV, sv.NT, n, onsets, lengths, uni.params, tile_instances=tile)), bits(want)), tile
        assert np.array_equal(bits(prog.render_score(sv.NV, sv.NT, n, onsets, None, uni.params, gains, tile_instances=tile)), bits(want_g)), tile
    # voices that began before the timeline, and voices behind its end (a tile of them renders nothing)
    moved = np.array(onsets)
    moved[::3] -= 400
    moved[1::4] += sv.NT
    want_m = score_chain(planar, moved, sv.NT, lengths, gains)
    for tile in (0, 2):
        assert np.array_equal(bits(prog.render_score(sv.NV, sv.NT, n, moved, lengths, uni.params, gains, tile_instances=tile)), bits(want_m)), tile
    again = prog.render(sv.NV, n, uni.params)
    assert np.array_equal(bits(again), bits(planar)), "a render after a score differs from the one before it"
    prog.state(0)  # ... and the state is there again
    if kind == "score":
        d.configure(sv.SAMPLE_RATE)
        for g, mine in ((None, got), (gains, prog.render_score(sv.NV, sv.NT, n, onsets, lengths, uni.params, gains))):
            circuit = sv.as_one_circuit([sv.voice(k) for k in range(n)], onsets, g)
            ref = np.asarray(oracle.render(descriptor.extract(circuit).words, sv.NT), dtype=np.float32)
            assert np.array_equal(bits(mine), bits(ref)), "differs from the oracle's Sum.many of Delays at sample %d" % int(np.argmax((bits(mine) != bits(ref)).any(axis=0)))
    prog.close()


@pytest.mark.parametrize("kind", ["pan", "score"])
def test_render_score_pcm_delivery(kind):
    """s16 / s24 frames and the peak of the PIECE: wav.encode_frames over the f32 timeline, for every normalise mode."""
    n = 37
    uni = unified(kind, n)
    onsets, lengths, gains = sv.layout(n)
    prog = jit_context().build(uni.words)
    piece = prog.render_score(sv.NV, sv.NT, n, onsets, lengths, uni.params, gains, tile_instances=16)
    peak_want = np.float32(np.abs(piece).max())
    assert peak_want > 1.0  # (normalise = 1 has something to shrink)
    for fmt, depth in FORMATS.items():
        for normalise in (0, 1, 2):
            data, peak = prog.render_score(sv.NV, sv.NT, n, onsets, lengths, uni.params, gains, tile_instances=16, format=fmt, normalise=normalise)
            want, want_peak = wav.encode_frames(piece, depth, normalise)
            assert data.dtype == want.dtype and data.shape == want.shape, (fmt, data.shape, want.shape)
            assert np.array_equal(data.view(np.uint8), want.view(np.uint8)), (fmt, normalise)
            assert np.float32(peak).view(np.uint32) == np.float32(want_peak).view(np.uint32) == peak_want.view(np.uint32)
    prog.close()


def test_render_score_refusals():
    d.configure(sv.SAMPLE_RATE)
    ctx = jit_context()
    noisy = ctx.build(descriptor.extract(d.Multiply(d.HostSource(np.zeros(64, dtype=np.float32)), 0.5)).words)
    assert noisy.n_inputs == 1
    with pytest.raises(runtime.DuspHipError, match="input streams") as e:
        noisy.render_score(64, 128, 1, [0])
    assert e.value.status == -2
    noisy.close()
    uni = unified("score", 2)
    resumable = ctx.build(uni.words, runtime.ENGINE_AUTO | runtime.ENGINE_RESUMABLE)
    with pytest.raises(runtime.DuspHipError, match="resumable") as e:
        resumable.render_score(64, 128, 2, [0, 1], params=uni.params)
    assert e.value.status == -2
    resumable.close()
    prog = ctx.build(uni.words)
    for call, needle in [
        (lambda: prog.render_score(64, 128, 2, [0, 1], [64, 65], uni.params), "length of voice 1 is 65"),
        (lambda: prog.render_score(64, 128, 2, [0, 1], [-1, 64], uni.params), "length of voice 0 is -1"),
        (lambda: prog.render_score(64, 0, 2, [0, 1], None, uni.params), "timeline"),
        (lambda: prog.render_score(0, 128, 2, [0, 1], None, uni.params), "n_samples"),
        (lambda: prog.ctx._check(prog._L.dusp_render_host_score(prog._h, 2, 64, (1 << 31) + 1, uni.params.ctypes.data, None, np.zeros(2, np.int64).ctypes.data, None, 0, 0, 0,
                                                                np.empty(4, np.float32).ctypes.data, None)), "2\\^31"),  # (sizes only: refused in front of any allocation)
        (lambda: prog.ctx._check(prog._L.dusp_render_host_score(prog._h, 2, 64, 128, uni.params.ctypes.data, None, None, None, 0, 0, 0, np.empty(128, np.float32).ctypes.data, None)),
         "h_onsets"),
        (lambda: prog.ctx._check(prog._L.dusp_render_host_score(prog._h, 2, 64, 128, uni.params.ctypes.data, None, np.zeros(2, np.int64).ctypes.data, None, 0, 7, 0,
                                                                np.empty(128, np.float32).ctypes.data, None)), "format"),
    ]:
        with pytest.raises(runtime.DuspHipError, match=needle) as e:
            call()
        assert e.value.status == -1
    for call, needle in [
        (lambda: prog.render_score(64, 128, 2, [0, 0.5], None, uni.params), "whole numbers"),
        (lambda: prog.render_score(64, 128, 2, [0, 1], [1.5, 2], uni.params), "whole numbers"),
        (lambda: prog.render_score(64, 128, 2, [0, 1, 2], None, uni.params), "onsets must have shape"),
        (lambda: prog.render_score(64, 128, 2, [0, 1], [1], uni.params), "lengths must have shape"),
        (lambda: prog.render_score(64, 128, 2, [0, 1], None, uni.params, gains=[1.0, 2.0, 3.0]), "gains must have shape"),
        (lambda: prog.render_score(64, 128, 3, [0, 1, 2], None, uni.params), "params must have shape"),
        (lambda: prog.render_score(64, 128, 2, [0, 1], None, uni.params, format=7), "format"),
        (lambda: prog.render_score(64, 128, 2, [0, 1], None, uni.params, format="s16", normalise=3), "normalise"),
    ]:
        with pytest.raises(ValueError, match=needle):
            call()
    assert prog.render_score(64, 128, 2, np.array([0.0, 64.0]), None, uni.params).shape == (1, 128)  # (whole numbers may come as floats)
    prog.close()


def test_render_py_surface():
    """render_score / render_score_pcm / render_score_wav: what renderChannelData(Sum.many(Delay ...)) computes, as ChannelData, frames
    and a file whose header parses back."""
    d.configure(sv.SAMPLE_RATE)
    n = 9
    onsets, lengths, gains = sv.layout(n)
    dur, voice_dur = (sv.NT + 0.5) / sv.SAMPLE_RATE, (sv.NV + 0.5) / sv.SAMPLE_RATE  # (durations are in seconds and truncate to NT and NV samples)
    voices = lambda: [sv.voice(k) for k in range(n)]
    ref = d.renderChannelData(sv.as_one_circuit(voices(), onsets, gains), dur)
    piece = render.render_score(voices(), onsets, voice_dur, dur, lengths, gains, tile_instances=4)
    assert piece.sampleRate == sv.SAMPLE_RATE and len(piece) == 1 and piece[0].shape == (sv.NT,) and np.array_equal(bits(piece[0]), bits(np.asarray(ref[0])))
    planar = np.stack([np.asarray(c) for c in ref])
    res = render.render_score_pcm(voices(), onsets, voice_dur, dur, 24, 2, lengths, gains)
    want, peak = wav.encode_frames(planar, 24, 2)
    assert np.array_equal(res.data.view(np.uint8), want.view(np.uint8)) and res.peak == peak and res.bitDepth == 24 and res.numberOfChannels == 1
    file = render.render_score_wav(voices(), onsets, voice_dur, dur, 16, 0, lengths, gains)
    assert file == wav.encode_wav(ref, sv.SAMPLE_RATE, 16)
    assert file[:4] == b"RIFF" and file[8:16] == b"WAVEfmt " and struct.unpack("<I", file[4:8])[0] == len(file) - 8
    fmt_tag, channels, rate, _, block_align, depth = struct.unpack("<HHIIHH", file[20:36])
    assert (fmt_tag, channels, rate, block_align, depth) == (1, 1, sv.SAMPLE_RATE, 2, 16)
    assert file[36:40] == b"data" and struct.unpack("<I", file[40:44])[0] == 2 * sv.NT == len(file) - 44
    assert len(render.render_score(voices(), onsets, voice_dur, 0)) == 0
    with pytest.raises(ValueError, match="whole numbers"):
        render.render_score(voices(), onsets + 0.5, voice_dur, dur)
    # what is checked does not depend on the durations, and a voice of no samples is refused (as the JavaScript host refuses it)
    for call, needle in [(lambda: render.render_score(voices(), onsets + 0.5, voice_dur, 0), "whole numbers"), (lambda: render.render_score(voices(), onsets[:3], voice_dur, 0), "onsets must have shape"),
                         (lambda: render.render_score(voices(), onsets, voice_dur, 0, lengths + sv.NV), "lengths must lie"),
                         (lambda: render.render_score_pcm(voices(), onsets, voice_dur, 0, gains=[1.0]), "gains must have shape")]:
        with pytest.raises(ValueError, match=needle):
            call()
    for call in (lambda: render.render_score(voices(), onsets, 0, dur), lambda: render.render_score_wav(voices(), onsets, 0, 0)):
        with pytest.raises(descriptor.DuspError, match="voice_duration must cover at least one sample"):
            call()
